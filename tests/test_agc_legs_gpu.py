"""wmx_agc_process_legs (wmix_amd/csrc/agc.hip): the AGC over the ragged rows of a bridge's legs, the kernel alone.  70 legs (one full
workgroup and a part-full one) over 40 ticks of seeded rows at levels from 3 to 30 000: 0 .. max_packets rows per leg and tick, lens
other than 0 and 320 among them, one leg that never gets a row, without call lists and with random ones, every leg on the batch's
compression gain and with legs 1, 9 and 66 on gains of their own (the per-lane gain tables).  Every row taken equals
tests/leg_level_model.py (the oracle over the leg's ordered rows), every other byte of the plane is unchanged, and outputs and exported
state equal wmx_agc_process over a dense plane of the same rows in the same order.  Integers, np.array_equal."""
import numpy as np
import pytest

from leg_level_model import level
from leg_stage_inputs import IDLE_LEG, ROW, TICKS, script
from legs_kernel_harness import Stage, check_against_dense, check_against_model, refusals, run_legs, switched_off, two_byte_boundary

pytestmark = pytest.mark.gpu

N, VALUE = 70, 20
OWN = {1: 6, 9: 30, 66: 12}  # leg -> a compression gain of its own


def make(n=N, own=None, chn=1, freq=8000):
    from wmix_amd.agc import AgcBatch
    ab = AgcBatch(n, chn, freq, VALUE)
    for g, v in (own or {}).items():
        ab.set_gain_streams([g], v)
    return ab


def stage(own=None):
    """the batch with the legs of `own` on gains of their own, and its model: a handle made with the batch's value, agc_addition in
    front of the leg's first call"""
    return Stage(lambda n=N: make(n, own), (2, 80),
                 lambda lib, rows, g: level(lib, rows, VALUE, {0: own[g]} if own and g in own else None), "wmx_agc_process_legs", b"1 x 8000", ())


@pytest.mark.parametrize("own", [None, OWN], ids=["one_gain", "own_gains"])
@pytest.mark.parametrize("k_slots,with_lists", [(1, False), (3, False), (4, False), (1, True), (3, True), (4, True)])
def test_ragged_rows_equal_the_model_and_the_dense_call(cuda, oracle_port, k_slots, with_lists, own):
    ticks = script(100 * k_slots + int(with_lists), k_slots, with_lists, n=N)
    st, ab = stage(own), make(N, own)
    idle_before = ab.export_stream(IDLE_LEG)
    got, seen = run_legs(cuda, ticks, ab, watch=[IDLE_LEG])
    fed = check_against_model(st, oracle_port, ticks, got)
    counts = [len(f) for f in fed]
    assert counts[IDLE_LEG] == 0 and min(c for g, c in enumerate(counts) if g != IDLE_LEG) > 0 and max(counts) >= TICKS // 4
    # the levels reach what they are for: full-scale samples come out of the loud legs, on both sides
    taken = np.concatenate([got[t][g, k, :ROW] for g in range(N) for t, k in fed[g]])
    assert (taken == 32767).any() and (taken == -32768).any()
    if with_lists:
        lists = [c for _, _, ls in ticks for c in ls]
        assert any(len(c) == 4 for c in lists) and any(("S", None) in c for c in lists)
    check_against_dense(st, cuda, ticks, got, fed, ab)
    # assertion 6: the leg given nothing never changes its state -- that of a fresh stream
    assert all(np.array_equal(s[IDLE_LEG], idle_before) for s in seen)
    other = make(1)
    assert np.array_equal(idle_before, other.export_stream(0))
    if own:
        assert [ab.stream_gain(g) for g in (0, 1, 9, 66)] == [VALUE, OWN[1], OWN[9], OWN[66]]
    other.close()
    ab.close()


def test_rows_on_a_two_byte_boundary_are_taken_and_an_odd_address_is_refused(cuda, wmx, oracle_port):
    two_byte_boundary(stage(OWN), cuda, wmx, oracle_port, script(9, 3, True, n=N, ticks=6, pad=1))


def test_a_leg_switched_off_keeps_its_rows_and_its_state(cuda):
    """wmx_agc_set_active's mask holds here as in wmx_nsx_process_legs: a leg that is switched off is a leg without a row"""
    plane, _, again = switched_off(stage(OWN), cuda, N, [2, 64, N - 1])
    assert all(not np.array_equal(again[g], plane[g]) for g in range(N))


def test_refusals_launch_nothing(cuda, wmx):
    refusals(stage(), cuda, wmx, [make(6, None, 2, 8000), make(6, None, 1, 16000), make(6, None, 1, 32000)])  # a handle that is not 1 x 8000
