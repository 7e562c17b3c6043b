"""GPU: lane predicates taken from scalar mask constants (wmix_amd/csrc/wmx_internal.h lanes<>, lane_sites.h).
(a) every mask the kernels use, evaluated per lane beside the arithmetic predicate of the lane id it replaces
    (wmx_debug_lane_masks: one row per entry of WMX_LANE_SITES, the list the call sites take their masks from), in a workgroup of
    64 and of 256 threads and once more inside a divergent branch that switches half the lanes off;
(b) the echo canceller at 8 and 16 kHz against oracle/orc_aec.c, 5 streams -- a workgroup carries four, so the second one holds one
    stream and three waves without -- one packet per launch (launches of 2 and of 3 blocks at 16 kHz), 70 packets: the pass-through
    phase is packets 0 .. 5, and the 64 packets behind it are 160 (16 kHz) and 80 (8 kHz) blocks per stream with 8 delay-estimate
    blocks each, the start of the noise floor (block 50) and the order statistics of the echo state in every block (counted with
    the coverage build of the oracle: echoState = 1 and its qsort in 800 of 800 and 400 of 400 blocks);
(c) the noise suppressor at 8, 16 and 32 kHz against oracle/orc_ns.c, 5 streams, 60 packets (block 50 is crossed), one of them
    all zero.
Bit for bit, (b) with the fallback of tests/test_aec_gpu.py::check_float_path on a host whose powf is not the product's."""
import numpy as np
import pytest

from oracle import loader as L

pytestmark = pytest.mark.gpu

HALF = 0x0F0F33335555FF00  # 32 lanes on, in runs of 8, 4, 2 and 1


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("threads,diverge", [(64, None), (256, None), (256, HALF)])
def test_every_mask_is_its_arithmetic_predicate(wmx, cuda, threads, diverge):
    import torch
    n = wmx.wmx_debug_lane_sites()
    names = [wmx.wmx_debug_lane_site_name(i).decode() for i in range(n)]
    assert n >= 30 and len(set(names)) == n and wmx.wmx_debug_lane_site_name(n) is None
    out = torch.full((n, threads), -1, dtype=torch.int32, device=cuda)
    assert wmx.wmx_debug_lane_masks(threads, (1 << 64) - 1 if diverge is None else diverge, out.data_ptr(), None) == 0
    out = out.cpu().numpy()
    lane = np.arange(threads) & 63
    on = np.array([diverge is None or (diverge >> int(l)) & 1 == 1 for l in lane])
    assert on.sum() == (threads if diverge is None else threads // 2)
    assert (out[:, ~on] == -1).all(), "a lane outside the branch stored"
    got = out[:, on]
    assert ((got == 0) | (got == 3)).all(), "mask and arithmetic predicate disagree: %s" % sorted(
        {"%s lane %d: mask %d, arithmetic %d" % (names[s], lane[on][t], got[s, t] & 1, got[s, t] >> 1) for s, t in zip(*np.nonzero((got != 0) & (got != 3)))})[:8]
    # and the rows are the sets the names say (the list is not checked against itself alone)
    row = {nm: got[i] == 3 for i, nm in enumerate(names)}
    ln = lane[on]
    assert np.array_equal(row["aec_lane0"], ln == 0) and np.array_equal(row["aec_upper"], ln >= 32)
    assert np.array_equal(row["aec_upd8"], ln < 8) and np.array_equal(row["aec_ef"], (ln & 3) == 2)
    assert np.array_equal(row["fft_p1_b1"], (ln >> 2) == 1) and np.array_equal(row["fft_p2_b1"], (ln >> 4) == 1)


def test_the_entry_refuses_a_block_that_is_no_multiple_of_a_wave(wmx):
    assert wmx.wmx_debug_lane_masks(96, (1 << 64) - 1, 8, None) == -10001
    assert wmx.wmx_debug_lane_masks(64, (1 << 64) - 1, None, None) == -10001


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("freq", [8000, 16000])
def test_aec_five_streams_vs_oracle(cuda, oracle_port, freq):
    from wmix_amd import synth
    from test_aec_gpu import check_float_path, gpu_aec
    S, n, pkg = 5, 70, freq // 100
    far = synth.far_end(9101, n, pkg)
    near = synth.near_end(9200, S, n, pkg, far=far)
    want = np.stack([L.run_aec(oracle_port, 1, freq, 10, far, near[s], pkg, 0, prefix="orc") for s in range(S)])
    got = gpu_aec(cuda, 1, freq, 10, 0, far, near, pkts_per_launch=1)
    assert (want[:, 8 * pkg:] != near[:, 8 * pkg:]).any(), "the run never left the pass-through phase"
    check_float_path(got, want)


# ---------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("chn,freq", [(1, 8000), (1, 16000), (2, 16000), (1, 32000)])
def test_ns_five_streams_vs_oracle(cuda, oracle_port, chn, freq):
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    from make_ns_golden import ns_case_input
    from test_ns_gpu import run_gpu
    S, nf = 5, 60
    x = np.stack([ns_case_input(chn, freq, nf, seed=9300 + 17 * s) for s in range(S)])
    x.reshape(S, nf, -1)[:, 31] = 0  # one all-zero packet
    want = np.stack([L.run_ns(oracle_port, chn, freq, x[s], freq // 100, prefix="orc") for s in range(S)])
    got = run_gpu(cuda, chn, freq, x, packets_per_launch=7)
    assert np.array_equal(got, want)
