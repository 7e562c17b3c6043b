"""Float NS kernel (wmix_amd/csrc/ns.hip) against oracle/orc_ns.c, bit-exact (0 differing samples), on the inputs that reach what the
kernel does with otherwise idle lanes: the sum of the log-likelihood-ratio averages runs as a fourth chain beside FeatureUpdate's three,
the input energy beside the output energy (a chain that is off until block 200 and on after it), the divisions by the bin count in the
lanes that hold the sums, and the frame-energy gate is a ballot over the terms instead of a comparison of their sum.

Nine streams: two full workgroups of four waves and a ragged third.  230 packets: a run crosses block_ind 50 (kStartupShort) and 200
(kStartupLong).  Every stream its own noise, one silent throughout."""
import ctypes as C

import numpy as np
import pytest

from oracle import loader as L
from wmix_amd import synth

S, NF = 9, 230
CASES = [(1, 16000), (2, 16000), (1, 8000), (1, 32000)]
_want = {}


def streams_input(chn, freq):
    pkt = freq // 100
    x = np.stack([synth.ns_input(9100 + 17 * s + chn, chn, NF, pkt).T.reshape(-1) for s in range(S)]).astype(np.int16)
    x[4] = 0  # silent throughout: every frame takes the zero-energy branch
    x[6].reshape(NF, -1)[120:126] = 0  # and one stream with a gap
    return np.ascontiguousarray(x)


def oracle_streams(port, key, x, chn, freq):
    """The oracle's output for x [streams, samples], computed once per case and left unchanged."""
    if key not in _want:
        w = np.stack([L.run_ns(port, chn, freq, row, freq // 100, prefix="orc") for row in x])
        w.setflags(write=False)
        _want[key] = w
    return _want[key]


def run_gpu(cuda, chn, freq, x, packets_per_launch):
    import torch
    from wmix_amd.ns import NsBatch
    n, per = x.shape[0], freq // 100 * chn
    nf = x.shape[1] // per
    nb = NsBatch(n, chn, freq)
    d = torch.from_numpy(np.ascontiguousarray(x.reshape(n, nf, per))).to(cuda)
    for f in range(0, nf, packets_per_launch):
        nb.process(d[:, f:f + packets_per_launch])
    out = d.cpu().numpy().reshape(n, -1)
    nb.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("chn,freq", CASES)
def test_nine_streams_across_both_startup_thresholds(cuda, oracle_port, chn, freq):
    x = streams_input(chn, freq)
    want = oracle_streams(oracle_port, ("streams", chn, freq), x, chn, freq)
    assert (want[4] == 0).all() and want[0].any()
    got = run_gpu(cuda, chn, freq, x, packets_per_launch=64)
    diff = int((got != want).sum())
    print("%dx%d: %d differing samples of %d" % (chn, freq, diff, want.size))
    assert diff == 0


@pytest.mark.gpu
def test_one_packet_per_launch_is_the_same(cuda, oracle_port):
    """The flagship line's shape: one 10 ms packet per launch (the packet loop of a launch runs once)."""
    chn, freq = 1, 16000
    x = streams_input(chn, freq)
    want = oracle_streams(oracle_port, ("streams", chn, freq), x, chn, freq)
    got = run_gpu(cuda, chn, freq, x, packets_per_launch=1)
    assert int((got != want).sum()) == 0


# ---- the zero-frame gate: energy exactly zero with non-zero data in the analysis buffer.
# A packet enters the analysis buffer (L samples) at [L - B, L) and lies at [L - 2B, L - B) one frame later, so sample j = 2B - L of a
# packet is at index 0 of the NEXT frame's buffer, where both windows are 0.0 (tests/test_ns_window_terms.py).
GATE_PACKET, GATE_NF = 3, 225
GATE_CASES = [(1, 16000), (1, 8000), (2, 16000)]


def core_sizes(freq):
    return (128, 80) if freq == 8000 else (256, 160)  # analysis length L, block length B


def gate_input(chn, freq):
    """[2 streams]: zeros, then in packet GATE_PACKET one sample at j = B - (L - B), a packet of zeros, then ordinary noise (past block
    200); the second stream is the same noise from the first packet on."""
    Ln, B = core_sizes(freq)
    pkt = freq // 100
    noise = synth.ns_input(7700 + chn, chn, GATE_NF, pkt).T.reshape(GATE_NF, pkt * chn).astype(np.int16)
    x = np.stack([noise, noise]).copy()
    g = x[0]
    g[:GATE_PACKET + 2] = 0
    g[GATE_PACKET, (B - (Ln - B)) * chn] = 12345
    if chn == 2:
        g[GATE_PACKET + 1, 1::2] = noise[GATE_PACKET + 1, 1::2]  # the high band of a zero frame passes through unscaled
    return np.ascontiguousarray(x.reshape(2, -1))


class _Fft(C.Structure):  # oracle/orc_fft.h, field for field
    _fields_ = [("n", C.c_int), ("nw", C.c_int), ("nc", C.c_int), ("w", C.c_float * 128), ("w2", C.c_float),
                ("W1", C.c_float * 64), ("W2", C.c_float * 64), ("W3", C.c_float * 64)]


class _Core(C.Structure):  # oracle/orc_ns.h: orc_ns_core up to block_ind, field for field
    _fields_ = [("fs", C.c_int), ("block_len", C.c_int), ("ana_len", C.c_int), ("magn_len", C.c_int), ("window", C.c_float * 256),
                ("fft", _Fft), ("analyze_buf", C.c_float * 256), ("data_buf", C.c_float * 256), ("synt_buf", C.c_float * 256),
                ("data_buf_hb", C.c_float * 512), ("density", C.c_float * 387), ("lquantile", C.c_float * 387),
                ("quantile", C.c_float * 129), ("counter", C.c_int * 3), ("updates", C.c_int),
                ("per_bin", C.c_float * (10 * 129)), ("overdrive", C.c_float), ("denoise_bound", C.c_float), ("gainmap", C.c_int),
                ("block_ind", C.c_int)]


@pytest.mark.parametrize("chn,freq", GATE_CASES)
def test_gate_input_takes_the_oracles_zero_energy_branch(oracle_port, chn, freq):
    """No GPU: the oracle, driven packet by packet, leaves block_ind alone in the frame after the lone sample (orc_ns_analyze returns
    before block_ind++) although its analysis buffer is not all zero -- otherwise the GPU test below proves nothing."""
    Ln, B = core_sizes(freq)
    pkt = freq // 100
    x = gate_input(chn, freq)[0].reshape(GATE_NF, pkt * chn)
    oracle_port.orc_ns_init.restype = C.c_void_p
    oracle_port.orc_ns_init.argtypes = [C.c_int, C.c_int]
    oracle_port.orc_ns_run.restype = None
    oracle_port.orc_ns_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    oracle_port.orc_ns_release.restype = None
    oracle_port.orc_ns_release.argtypes = [C.c_void_p]
    h = oracle_port.orc_ns_init(chn, freq)
    assert h
    try:
        core = _Core.from_address(h)  # orc_ns begins with its core
        # the mirror above reads the right words
        assert (core.fs, core.block_len, core.ana_len, core.magn_len) == (freq, B, Ln, Ln // 2 + 1)
        assert (core.overdrive, core.denoise_bound, core.gainmap, core.block_ind) == (np.float32(1.1), 0.125, 1, -1)
        assert core.window[0] == 0.0 and core.window[1] != 0.0
        out = np.empty(pkt * chn, np.int16)
        seen = []
        for f in range(GATE_PACKET + 3):
            oracle_port.orc_ns_run(h, x[f].ctypes.data, out.ctypes.data, pkt)
            buf = np.array(core.analyze_buf[:Ln])
            seen.append((core.block_ind, int(np.count_nonzero(buf)), int(np.flatnonzero(buf)[0]) if buf.any() else -1))
    finally:
        oracle_port.orc_ns_release(h)
    assert [b for b, _, _ in seen[:GATE_PACKET]] == [-1] * GATE_PACKET and all(n == 0 for _, n, _ in seen[:GATE_PACKET])
    assert seen[GATE_PACKET] == (0, 1, B)  # the lone sample's own frame is an ordinary one: block 0
    assert seen[GATE_PACKET + 1] == (0, 1, 0)  # the next: a non-zero sample at index 0 and block_ind NOT advanced -- the zero-energy branch
    assert seen[GATE_PACKET + 2][0] == 1  # noise: block 1


@pytest.mark.gpu
@pytest.mark.parametrize("chn,freq", GATE_CASES)
def test_zero_energy_frame_with_nonzero_buffer(cuda, oracle_port, chn, freq):
    x = gate_input(chn, freq)
    want = oracle_streams(oracle_port, ("gate", chn, freq), x, chn, freq)
    assert want[0].any()
    got = run_gpu(cuda, chn, freq, x, packets_per_launch=5)  # the gated frame is the last packet of a launch that began with zero frames
    diff = int((got != want).sum())
    print("gate %dx%d: %d differing samples of %d" % (chn, freq, diff, want.size))
    assert diff == 0
