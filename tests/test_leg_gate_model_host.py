"""tests/leg_gate_model.py on the host alone: the model over contiguous rows is the oracle's batch runner, and the inputs of the GPU tests
(tests/leg_gate_inputs.py, tests/conf_inputs.py) do on the oracle what those tests need them to do: some leg of the direct test's
script reaches every `reduce` 0 .. 4 both rising and falling, the quiet leg stays shut, the sigma = 400 noise leg is shut from its
10th row on, random codes open the gate within five rows.  No GPU, nothing of wmix_amd."""
import numpy as np
import pytest

from conf_inputs import G, SEED, T, alaw_decode, arrivals, ulaw_decode, ulaw_encode
from leg_gate_inputs import CASES, CODES_LEG, LAST_GROUP, N, NOISE_LEG, QUIET_LEG, ROW, TICKS, case_seed, leg_signal, script, spurts
from leg_gate_model import LegsGateModel, gate, was_voice
from leg_rows_model import rows_taken
from oracle import loader as L


def steps(trace):
    """the (from, to) pairs of a leg's `reduce`, the fresh 4 in front"""
    return set(zip([4] + trace[:-1], trace))


RISING, FALLING = {(r, r + 1) for r in range(4)}, {(r + 1, r) for r in range(4)}


def test_the_model_over_contiguous_rows_is_the_oracles_runner(oracle_port):
    for x in (spurts(120, phase=30), leg_signal(NOISE_LEG, 60, 1), leg_signal(CODES_LEG, 30, 1), leg_signal(QUIET_LEG, 30, 1)):
        got, trace = gate(oracle_port, x.reshape(-1, ROW))
        want = L.run_vad(oracle_port, 1, 8000, 20, x, ROW, prefix="orc").reshape(-1, ROW)
        assert np.array_equal(got, want)
        # and a row is the input shifted right by the `reduce` behind it
        assert all(np.array_equal(got[i], x.reshape(-1, ROW)[i] >> trace[i]) for i in range(len(trace)))


def test_the_step_of_reduce_tells_the_decision():
    assert [was_voice(b, a) for b, a in ((4, 3), (1, 0), (0, 0))] == [True] * 3
    assert [was_voice(b, a) for b, a in ((3, 4), (0, 1), (4, 4))] == [False] * 3


def test_the_spurts_walk_reduce_through_every_value_both_ways(oracle_port):
    _, trace = gate(oracle_port, spurts(150).reshape(-1, ROW))
    assert RISING | FALLING <= steps(trace)
    for period in range(1, 3):  # in every period: shut at the end of the noise, open at the end of the voice
        assert trace[50 * period + 24] == 4 and trace[50 * period + 49] == 0, trace


@pytest.mark.parametrize("k_slots,with_lists", CASES)
def test_the_direct_tests_script_reaches_what_it_is_for(oracle_port, k_slots, with_lists):
    ticks = script(case_seed(k_slots, with_lists), k_slots, with_lists)
    m = LegsGateModel(oracle_port, N)
    fed_counts = np.zeros((TICKS, N), int)
    for t, (plane, lens, lists) in enumerate(ticks):
        fed = m.tick(plane.copy(), lens, lists)
        fed_counts[t] = [len(f) for f in fed]
    both = [g for g in range(N) if RISING | FALLING <= steps(m.trace[g])]
    assert both, "no leg walks reduce through 0 .. 4 both ways"
    assert any(g in LAST_GROUP for g in both) or any(FALLING <= steps(m.trace[g]) for g in LAST_GROUP)
    assert m.trace[QUIET_LEG] and set(m.trace[QUIET_LEG]) == {4}
    assert len(m.trace[NOISE_LEG]) > 20 and set(m.trace[NOISE_LEG][9:]) == {4}
    assert m.trace[CODES_LEG][0] >= 3 and set(m.trace[CODES_LEG][5:]) == {0}  # open after four rows judged voice, and stays open
    assert m.voiced.sum() > 0 and m.unvoiced.sum() > 0 and np.array_equal(m.voiced + m.unvoiced, fed_counts.sum(0))
    # the schedule: every count 0 .. k_slots occurs, ticks in which the second workgroup brings nothing while the first does, and ticks
    # in which it brings something
    assert set(fed_counts.reshape(-1)) == set(range(k_slots + 1))
    empty = [t for t in range(TICKS) if not fed_counts[t, 64:].any()]
    assert len(empty) >= TICKS // 5 and all(fed_counts[t, :64].any() for t in empty) and len(empty) < TICKS // 2
    if with_lists:
        lists = [c for _, _, ls in ticks for c in ls]
        assert any(("S", None) in c for c in lists)
        assert any(kind == "D" and (k >= k_slots or lens[g][k] != 320) for _, lens, ls in ticks for g, c in enumerate(ls) for kind, k in c)
        assert any([k for _, k in c if k is not None] != sorted(k for _, k in c if k is not None) for c in lists)
    m.close()


def test_stationary_noise_shuts_the_gate_and_random_codes_open_it(oracle_port):
    for sigma, want in ((400.0, [3, 2, 1, 0, 1, 2, 3, 4]), (50.0, [3, 2, 1, 0, 1, 2, 3, 4])):
        x = np.clip(np.round(np.random.default_rng(11).normal(0, sigma, 300 * ROW)), -32768, 32767).astype(np.int16)
        _, trace = gate(oracle_port, ulaw_decode(ulaw_encode(x)).reshape(-1, ROW))
        assert trace[:8] == want and set(trace[9:]) == {4}, (sigma, trace[:12])
    pk, recv = arrivals(SEED, T, G)
    for g in range(G):
        rows = [alaw_decode(pk[t, g, k, 12:]) for t in range(T) for k in rows_taken(np.where(recv[t, g] == 172, 320, 0))
                if (pk[t, g, k, 1] & 0x7F) in (8, 0)]
        _, trace = gate(oracle_port, np.array(rows))
        assert trace[:5] == [4, 3, 2, 1, 0] and set(trace[5:]) == {0}, (g, trace)  # a call's first four rows come out attenuated
