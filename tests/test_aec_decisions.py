"""CPU: the decision function of the float AEC's sdSum / seSum gate (wmix_amd/csrc/aec_gate.h) through its host entry
wmx_debug_aec_decide -- the source the near kernel compiles -- against the reference's ordered float32 sums and comparisons
(oracle/orc_aec.c:241-256) in numpy.  Where the gate says `decided`, its two decisions are the reference's, without exception; what it
cannot prove it leaves undecided, and the kernel then adds in index order as before."""
import numpy as np

from aec_gate_rows import crafted_rows, random_rows, reference


def decide(wmx, sd, se, prev):
    sd, se, prev = np.ascontiguousarray(sd, np.float32), np.ascontiguousarray(se, np.float32), np.ascontiguousarray(prev, np.int32)
    out = np.zeros((sd.shape[0], 4), np.int32)
    assert wmx.wmx_debug_aec_decide(sd.ctypes.data, se.ctypes.data, prev.ctypes.data, out.ctypes.data, sd.shape[0]) == 0
    return out


def test_random_rows_decided_means_the_references_decisions(wmx):
    sd, se, prev = random_rows(1_000_000, 17)
    want_div, want_rst = reference(sd, se, prev)
    assert want_div.min() == 0 and want_div.max() == 1 and want_rst.min() == 0 and want_rst.max() == 1  # the rows take all four outcomes
    out = decide(wmx, sd, se, prev)
    ok = out[:, 0] == 1
    wrong = ok & ((out[:, 1] != want_div) | (out[:, 2] != want_rst))
    assert not wrong.any(), "%d decided rows differ from the reference, first %d" % (wrong.sum(), np.flatnonzero(wrong)[0])
    undecided = 1.0 - ok.mean()
    print("undecided: %.3g of %d rows" % (undecided, ok.size))
    assert undecided <= 0.01


def test_crafted_rows_are_undecided_or_right(wmx):
    for kind, (sd, se, prev) in crafted_rows().items():
        want_div, want_rst = reference(sd, se, prev)
        out = decide(wmx, sd, se, prev)
        ok = out[:, 0] == 1
        assert not (ok & ((out[:, 1] != want_div) | (out[:, 2] != want_rst))).any(), kind
        assert not ok.all(), "%s: no row of this kind is left to the ordered sums" % kind


def test_rows_near_the_thresholds_lie_on_both_sides():
    """the crafted rows do what they are for: around each threshold the reference decides both ways"""
    kinds = crafted_rows()
    for kind, col in (("f = 1.0 within 4 ulp", 0), ("f = 1.05 within 4 ulp", 0), ("19.95 within 4 ulp", 1)):
        sd, se, prev = kinds[kind]
        got = reference(sd, se, prev)[col]
        assert got.min() == 0 and got.max() == 1, kind
