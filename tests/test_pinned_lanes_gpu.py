"""GPU: the float kernels where lane-constant values are formed once and then trusted -- for a launch (aec.hip: AecPins, made behind
the barrier of aec_near_kernel) or for a block (everything aec_block derives from the lane between its two launderings) -- against the
oracle port, bit for bit.  The NS kernels form nothing of the kind today (the head of ns_frame says what was tried); their cases are
here so that the next attempt meets them.  The shapes are the smallest at which such a value can be wrong:
(1) the echo canceller at 8 and 16 kHz, 5 streams -- a workgroup carries four, so the second one holds one live wave and three
    without a stream -- with one packet per launch and with two (then the packet loop iterates, 5 blocks per launch at 16 kHz, and
    what was formed at the kernel's entry has to survive it), 200 packets of the two inputs of tests/test_aec_near_gate_gpu.py: a far
    end that falls silent and an echo that breaks off -- the ordered sums, the filter reset and the delay estimate all run, the rare
    paths at which the register pressure peaks;
(2) the same 5 streams with stream 1, in the middle of the first workgroup, switched off (set_active): its wave leaves the kernel at
    the active test, its row and its state stay what they were, and its neighbours' results are the oracle's;
(3) the noise suppressor in its four instantiations (8, 16 and 32 kHz mono, 16 kHz two-channel), 5 streams, 7 packets per launch,
    530 packets: blocks 50, 200 and 500 are crossed (the histogram update, the widest rare path), one stream starts with the
    zero-energy frame of tests/test_ns_idle_lanes_gpu.py (energy zero, buffer not), one has an all-zero packet inside a launch.
The float bar is tests/test_aec_gpu.py::check_float_path (conftest.host_powf_is_the_products)."""
import numpy as np
import pytest

from oracle import loader as L

pytestmark = pytest.mark.gpu

S = 5
OFF = 1  # the stream that (2) switches off: neither the first nor the last wave of the first workgroup
_want = {}


def aec_input(kind, freq):
    from test_aec_near_gate_gpu import broken_echo_input, silent_far_input
    far, near = (silent_far_input if kind == "silent_far" else broken_echo_input)(freq)
    # streams 2 .. 6 of the eight: the broken echo has loud noise on streams 0 .. 3 and a dead microphone on 4 .. 7 -- both kinds
    return far, np.ascontiguousarray(near[2:2 + S])


def aec_oracle(port, kind, freq):
    """The oracle's output [S, samples] for one input, computed once and left unchanged."""
    if (kind, freq) not in _want:
        far, near = aec_input(kind, freq)
        w = np.stack([L.run_aec(port, 1, freq, 10, far, near[s], freq // 100, 0, prefix="orc") for s in range(S)])
        w.setflags(write=False)
        _want[kind, freq] = w
    return _want[kind, freq]


# ---------------------------------------------------------------------------------------------------------------- (1)
@pytest.mark.parametrize("per_launch", [1, 2])
@pytest.mark.parametrize("kind", ["silent_far", "broken_echo"])
@pytest.mark.parametrize("freq", [8000, 16000])
def test_aec_five_streams_rare_paths_vs_oracle(cuda, oracle_port, freq, kind, per_launch):
    from test_aec_gpu import check_float_path, gpu_aec
    far, near = aec_input(kind, freq)
    want = aec_oracle(oracle_port, kind, freq)
    pkg = freq // 100
    assert near.shape[1] >= 70 * pkg and (want[:, 8 * pkg:] != near[:, 8 * pkg:]).any(), "the run never left the pass-through phase"
    got = gpu_aec(cuda, 1, freq, 10, 0, far, near, pkts_per_launch=per_launch)
    check_float_path(got, want)


# ---------------------------------------------------------------------------------------------------------------- (2)
@pytest.mark.parametrize("freq", [8000, 16000])
def test_aec_inactive_stream_inside_the_first_workgroup(cuda, oracle_port, freq):
    import torch
    from test_aec_gpu import check_float_path
    from wmix_amd.aec import AecBatch
    far, near = aec_input("silent_far", freq)
    want = aec_oracle(oracle_port, "silent_far", freq)
    n_packets = 70
    ab = AecBatch(S, 1, freq, 10)
    try:
        n = far.size // ab.pkt
        assert n >= n_packets
        ab.set_active(np.arange(S) != OFF)
        state0 = ab.export_state(OFF).copy()
        dfar = torch.from_numpy(np.ascontiguousarray(far.reshape(n, ab.pkt))).to(cuda)
        d = torch.from_numpy(np.ascontiguousarray(near.reshape(S, n, ab.pkt)[:, :n_packets])).to(cuda)
        for f in range(0, n_packets, 2):
            rc, _ = ab.process2(dfar[f:f + 2], d[:, f:f + 2])
            assert rc == 0
        got = d.cpu().numpy().reshape(S, -1)
        state1 = ab.export_state(OFF)
    finally:
        ab.close()
    on = np.arange(S) != OFF
    m = n_packets * ab.pkt
    assert np.array_equal(got[OFF], near[OFF, :m]), "the row of the stream that is switched off was written"
    assert np.array_equal(state0.view(np.uint32), state1.view(np.uint32)), "the state of the stream that is switched off was written"
    assert (want[on, 8 * ab.pkt:m] != near[on, 8 * ab.pkt:m]).any()
    check_float_path(got[on], want[on, :m])


# ---------------------------------------------------------------------------------------------------------------- (3)
NS_NF = 530


def ns_input(chn, freq):
    from test_ns_idle_lanes_gpu import GATE_PACKET, core_sizes
    from wmix_amd import synth
    pkt = freq // 100
    x = np.stack([synth.ns_input(9500 + 17 * s + chn, chn, NS_NF, pkt).T.reshape(NS_NF, pkt * chn) for s in range(S)]).astype(np.int16)
    # stream 3: the zero-energy frame with a non-zero analysis buffer (test_ns_idle_lanes_gpu.gate_input): zeros, one sample at
    # j = B - (L - B) of packet GATE_PACKET, a packet of zeros -- its frame has energy exactly zero -- then the noise
    Ln, B = core_sizes(freq)
    x[3, :GATE_PACKET + 2] = 0
    x[3, GATE_PACKET, (B - (Ln - B)) * chn] = 12345
    x[1, 31] = 0  # an all-zero packet in the middle of a launch
    return np.ascontiguousarray(x.reshape(S, -1))


@pytest.mark.parametrize("chn,freq", [(1, 8000), (1, 16000), (2, 16000), (1, 32000)])
def test_ns_five_streams_across_the_histogram_update(cuda, oracle_port, chn, freq):
    from test_ns_gpu import run_gpu
    x = ns_input(chn, freq)
    want = np.stack([L.run_ns(oracle_port, chn, freq, x[s], freq // 100, prefix="orc") for s in range(S)])
    # every stream is past its 500th non-zero frame: the thresholds of the histogram update shape the last packets
    assert NS_NF - 6 > 500 and want[:, -freq // 100 * chn:].any()
    got = run_gpu(cuda, chn, freq, x, packets_per_launch=7)
    diff = int((got != want).sum())
    print("%dx%d: %d differing samples of %d" % (chn, freq, diff, want.size))
    assert diff == 0
