"""GPU: the gate of the float AEC's near kernel that settles the two decisions of SmoothedPSD without the ordered sums
(wmix_amd/csrc/aec_gate.h):
(a) the gate on its own, with the kernel's own reduction and, where it is undecided, the kernel's own ordered sums
    (wmx_debug_aec_decide_device), against the reference's ordered sums in numpy;
(b) the canceller against oracle/orc_aec.c on two inputs that lean on exactly these decisions -- a far end that falls silent (e == d,
    seSum == sdSum: every block of the stretch is undecided) and an echo that breaks off (the reference's divergeState becomes 1 and
    its filter reset fires; asserted with the coverage build of the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

N_PACKETS, N_STREAMS = 200, 8
DIVERGE_LINE = "if (a->divergeState) memcpy(efw, dfw, sizeof(efw));"
RESET_LINE = "if (seSum > (19.95f * sdSum)) memset(a->wf, 0, sizeof(a->wf));"


def silent_far_input(freq):
    """echo and near-end talk throughout; the far end is silent for packets 60 .. 139"""
    from wmix_amd import synth
    pkg = freq // 100
    far = synth.far_end(8101, N_PACKETS, pkg)
    far[60 * pkg:140 * pkg] = 0
    near = synth.near_end(8200, N_STREAMS, N_PACKETS, pkg, far=far)
    return far, near


def broken_echo_input(freq):
    """the filter adapts to a loud echo for 90 packets; then, for 60 packets, the near end is loud noise that has nothing to do with the
    far end (streams 0 .. 3) or the microphone goes dead (streams 4 .. 7: the filter's echo estimate is all that is left in the
    error): the error outgrows the near signal -- the reference's divergeState, and its filter reset -- until the echo comes back"""
    from wmix_amd import synth
    pkg = freq // 100
    n = N_PACKETS * pkg
    far = synth.far_end(8301, N_PACKETS, pkg, amp=12000)
    echo = np.zeros(n)
    echo[40:] = 0.8 * far[:-40]
    noise = synth.lcg_noise(8400 + np.arange(N_STREAMS, dtype=np.uint64), n, 100).astype(np.float64)
    loud = synth.lcg_noise(8500 + np.arange(N_STREAMS, dtype=np.uint64), n, 30000).astype(np.float64)
    near = noise + echo[None, :]
    a, b = 90 * pkg, 150 * pkg
    near[:4, a:b] = loud[:4, a:b]
    near[4:, a:b] = 0
    return far, np.clip(np.round(near), -32768, 32767).astype(np.int16)


def child(out_path):
    """Runs under WMIX_ORACLE_COV=1, without a GPU: which outcomes of the two decisions does the reference take on broken_echo_input?"""
    sys.path[:0] = [ROOT, HERE, os.path.join(ROOT, "tools_dev")]
    import oracle_branches as T
    from oracle import loader as L
    lib = L.port()
    res = {}
    for freq in (8000, 16000):
        far, near = broken_echo_input(freq)
        L.cov_reset()
        for s in range(N_STREAMS):
            L.run_aec(lib, 1, freq, 10, far, near[s], freq // 100, 0, prefix="orc")
        L.cov_dump()
        counts = T.outcomes(files=("orc_aec.c",))
        res[str(freq)] = {k: n for k, n in counts.items() if DIVERGE_LINE in k or RESET_LINE in k}
    with open(out_path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child(sys.argv[2])
    sys.exit(0)

pytestmark = pytest.mark.gpu

from aec_gate_rows import crafted_rows, random_rows, reference  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------- (a)
def decide_device(wmx, cuda, sd, se, prev):
    import torch
    d_sd = torch.from_numpy(np.ascontiguousarray(sd, np.float32)).to(cuda)
    d_se = torch.from_numpy(np.ascontiguousarray(se, np.float32)).to(cuda)
    d_prev = torch.from_numpy(np.ascontiguousarray(prev, np.int32)).to(cuda)
    out = torch.zeros((sd.shape[0], 4), dtype=torch.int32, device=cuda)
    assert wmx.wmx_debug_aec_decide_device(d_sd.data_ptr(), d_se.data_ptr(), d_prev.data_ptr(), out.data_ptr(), sd.shape[0], None) == 0
    return out.cpu().numpy()


def test_gate_on_the_device_takes_the_references_decisions(wmx, cuda):
    sd, se, prev = random_rows(4096, 23)
    want = reference(sd, se, prev)
    out = decide_device(wmx, cuda, sd, se, prev)
    assert np.array_equal(out[:, 1], want[0]) and np.array_equal(out[:, 2], want[1])
    fast = float((out[:, 0] == 1).mean())
    print("random rows settled by the gate: %.4f" % fast)
    assert fast >= 0.99
    # the host form of the entry adds the same pairs: the same rows are left to the ordered sums
    host = np.zeros((4096, 4), np.int32)
    assert wmx.wmx_debug_aec_decide(sd.ctypes.data, se.ctypes.data, prev.ctypes.data, host.ctypes.data, 4096) == 0
    assert np.array_equal(host[:, 0], out[:, 0])
    for kind, (sd, se, prev) in crafted_rows().items():
        want = reference(sd, se, prev)
        out = decide_device(wmx, cuda, sd, se, prev)
        assert np.array_equal(out[:, 1], want[0]) and np.array_equal(out[:, 2], want[1]), kind
        assert (out[:, 0] == 0).any(), "%s: no row took the ordered sums" % kind
        if kind == "se == sd":
            assert (out[prev == 0, 0] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("freq", [8000, 16000])
def test_far_end_falls_silent_vs_oracle(cuda, oracle_port, freq):
    from oracle import loader as L
    from test_aec_gpu import check_float_path, gpu_aec
    far, near = silent_far_input(freq)
    pkg = freq // 100
    want = np.stack([L.run_aec(oracle_port, 1, freq, 10, far, near[s], pkg, 0, prefix="orc") for s in range(N_STREAMS)])
    got = gpu_aec(cuda, 1, freq, 10, 0, far, near, pkts_per_launch=50, packet_major=True)
    check_float_path(got, want)


@pytest.fixture(scope="module")
def broken_echo_outcomes(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gate_cov") / "cov.json")
    env = dict(os.environ, WMIX_ORACLE_COV="1")
    for k in ("WMIX_ORACLE_SAN", "GCOV_PREFIX", "GCOV_PREFIX_STRIP"):
        env.pop(k, None)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], check=True, env=env, cwd=ROOT)
    with open(out) as f:
        return json.load(f)


@pytest.mark.parametrize("freq", [8000, 16000])
def test_echo_path_breaks_vs_oracle(cuda, oracle_port, broken_echo_outcomes, freq):
    from oracle import loader as L
    from test_aec_gpu import check_float_path, gpu_aec
    # the reference takes both outcomes of both decisions on this input: divergeState 0 and 1, the filter kept and reset
    counts = broken_echo_outcomes[str(freq)]
    for line in (DIVERGE_LINE, RESET_LINE):
        hits = [n for k, n in counts.items() if line in k]
        assert len(hits) == 2 and min(hits) > 0, (line, counts)
    far, near = broken_echo_input(freq)
    pkg = freq // 100
    want = np.stack([L.run_aec(oracle_port, 1, freq, 10, far, near[s], pkg, 0, prefix="orc") for s in range(N_STREAMS)])
    got = gpu_aec(cuda, 1, freq, 10, 0, far, near, pkts_per_launch=50, packet_major=True)
    check_float_path(got, want)
