"""wmx_nsx_process_legs (wmix_amd/csrc/nsx.hip): the fixed-point noise suppressor over the ragged rows of a bridge's legs, the kernel
alone.  37 legs (the last workgroup is part full) over 40 ticks of seeded random rows: 0 .. max_packets rows per leg and tick, lens
other than 0 and 320 among them, without call lists and with random ones.  Every row taken equals tests/leg_denoise_model.py (the
oracle over the leg's ordered rows), every other byte of the plane is unchanged, and outputs and exported state equal wmx_nsx_process
over a dense plane of the same rows in the same order.  Integers, np.array_equal."""
import numpy as np
import pytest

from leg_denoise_model import suppress
from leg_stage_inputs import IDLE_LEG, N, ROW, TICKS, script, signal
from legs_kernel_harness import Stage, check_against_dense, check_against_model, refusals, run_legs, two_byte_boundary

pytestmark = pytest.mark.gpu


def make(n=N, chn=1, freq=8000):
    from wmix_amd.nsx import NsxBatch
    return NsxBatch(n, chn, freq)


STAGE = Stage(make, (2, 80), lambda lib, rows, g: suppress(lib, rows), "wmx_nsx_process_legs", b"1 x 8000", ())


@pytest.mark.parametrize("k_slots,with_lists", [(1, False), (3, False), (4, False), (1, True), (3, True), (4, True)])
def test_ragged_rows_equal_the_model_and_the_dense_call(cuda, oracle_port, k_slots, with_lists):
    ticks = script(100 * k_slots + int(with_lists), k_slots, with_lists)
    nb = make()
    idle_before = nb.export_stream(IDLE_LEG)
    got, _ = run_legs(cuda, ticks, nb)
    fed = check_against_model(STAGE, oracle_port, ticks, got)
    counts = [len(f) for f in fed]
    assert counts[IDLE_LEG] == 0 and min(c for g, c in enumerate(counts) if g != IDLE_LEG) > 0 and max(counts) >= TICKS // 4
    if with_lists:  # the lists reach what they are for
        lists = [c for _, _, ls in ticks for c in ls]
        assert any(len(c) == 4 for c in lists) and any(("S", None) in c for c in lists)
        assert any(kind == "D" and k >= k_slots for c in lists for kind, k in c) or k_slots == 4
        assert any([k for _, k in c if k is not None] != sorted(k for _, k in c if k is not None) for c in lists) or k_slots == 1
    check_against_dense(STAGE, cuda, ticks, got, fed, nb)
    # assertion 4: a leg given nothing has the state of a fresh stream
    other = make(1)
    assert np.array_equal(nb.export_stream(IDLE_LEG), idle_before) and np.array_equal(idle_before, other.export_stream(0))
    other.close()
    nb.close()


def test_the_long_run_reaches_the_histogram_update(cuda, oracle_port):
    """3 legs, 2 rows a tick, 140 ticks: 560 blocks, past the suppressor's first feature update from its histograms"""
    rng = np.random.default_rng(7)
    n, ticks_n = 3, 140
    src = [signal(rng, 2 + g, ticks_n * 2 * ROW).reshape(ticks_n, 2, ROW) for g in range(n)]
    ticks = [(np.stack([src[g][t] for g in range(n)]), np.full((n, 2), 320, np.uint32), None) for t in range(ticks_n)]
    nb = make(n)
    got, _ = run_legs(cuda, ticks, nb)
    fed = check_against_model(STAGE, oracle_port, ticks, got)
    assert all(len(f) == 2 * ticks_n for f in fed)
    check_against_dense(STAGE, cuda, ticks, got, fed, nb)
    nb.close()


def test_rows_on_a_two_byte_boundary_are_taken_and_an_odd_address_is_refused(cuda, wmx, oracle_port):
    two_byte_boundary(STAGE, cuda, wmx, oracle_port, script(9, 3, True, n=6, ticks=6, pad=1))


def test_refusals_launch_nothing(cuda, wmx):
    refusals(STAGE, cuda, wmx, [make(6, 2, 8000), make(6, 1, 16000), make(6, 1, 32000)])  # a handle that is not 1 x 8000
