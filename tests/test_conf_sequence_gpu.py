"""wmx_conf_sequence (wmix_amd/csrc/conf.hip) through the Python mirror: the conference bridge with its legs reordered, de-duplicated and
gap-filled by RTP sequence number.  The layout, T, K and the script generator are those of tests/conf_inputs.py -- every packet of
clean_script() is audio (PCMA or PCMU), so that a clean script has no gap.  The reference for an impaired script is replay_seq() of
tests/conf_single_replays.py: the tick-by-tick replay (one reference ring per leg, a cursor per source leg) fed the REPAIRED rows, the
call lists of tests/leg_seq_model.py laid out as four slots, a silence call being a row of zeros.  Bytes and integers, np.array_equal."""
import numpy as np
import pytest

from conf_harness import bridge, counters_equal, run
from conf_inputs import EINVAL, G, IN_CONF, T, clean_script, impair, rows_of
from conf_single_replays import replay_seq
from leg_seq_model import COUNTERS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clean(cuda):
    pk, recv = rows_of(clean_script(1))
    cb = bridge()
    off = run(cb, pk, recv, "ahead")
    cb.close()
    return pk, recv, off


@pytest.mark.parametrize("slots,mode", [(1, "wait"), (3, "ahead"), (3, "resident")])
def test_a_clean_script_is_sent_as_with_sequencing_off(cuda, clean, slots, mode):
    pk, recv, off = clean
    cb = bridge(slots=slots)
    cb.sequence(True)
    got = run(cb, pk, recv, mode)
    assert np.array_equal(got, off), np.argwhere((got != off).any(2))[:6]
    st = cb.export_sequence()
    assert not any(st[name].any() for name in COUNTERS) and st["synced"].all()
    assert (off[:, IN_CONF, 12:] != 0xD5).any()
    cb.close()


def test_an_impaired_script_is_sent_as_the_replay_of_the_repaired_rows(cuda, oracle_port):
    script, kinds = impair(clean_script(2), 3)
    assert all(n >= 3 for n in kinds.values()), kinds  # on legs that are in a conference
    pk, recv = rows_of(script)
    want, model, _ = replay_seq(oracle_port, pk, recv)
    plain, clean_model, _ = replay_seq(oracle_port, *rows_of(clean_script(2)))
    assert not any(clean_model.export()[name].any() for name in COUNTERS) and not np.array_equal(want, plain)
    seen = model.export()
    assert all(seen[name][IN_CONF].sum() >= 3 for name in ("lost", "late", "dup", "resync")), {n: seen[n] for n in COUNTERS}
    for slots, mode in ((3, "ahead"), (3, "resident")):
        cb = bridge(slots=slots)
        cb.sequence(True, 3)
        got = run(cb, pk, recv, mode)
        assert np.array_equal(got, want), (mode, np.argwhere((got != want).any(2))[:6])
        counters_equal(cb, model)
        assert not cb.export_legs()["dropped"].any()
        cb.close()
    # sequencing off, the same script is sent otherwise
    cb = bridge()
    got = run(cb, pk, recv, "ahead")
    assert not np.array_equal(got, want)
    cb.close()


def test_lost_packets_do_not_shift_a_legs_cursor(cuda):
    """What the feature is for.  Losses only, on a steady script: with sequencing on every leg's cursor ends where the lossless run's
    ends; with it off, 320 bytes earlier per lost packet."""
    steady = clean_script(4, steady=True)
    rng = np.random.default_rng(5)
    lossy, lost = [[list(now) for now in tick] for tick in steady], np.zeros(G, np.uint32)
    for g in IN_CONF:
        for t in sorted(rng.choice(np.arange(4, T - 4), size=int(rng.integers(1, 5)), replace=False)):
            lossy[t][g] = []
            lost[g] += 1
    assert lost[IN_CONF].all() and lost.sum() >= 15

    def ticks_after(script, on):
        cb = bridge()
        cb.sequence(on, 3)
        run(cb, *rows_of(script), "ahead")
        st, sq = cb.export_legs(), cb.export_sequence()
        cb.close()
        return st["tick"].astype(np.int64), sq

    lossless, _ = ticks_after(steady, False)
    assert (lossless[IN_CONF] == lossless[0]).all() and lossless[9] == 0
    on, sq = ticks_after(lossy, True)
    assert np.array_equal(on, lossless) and np.array_equal(sq["lost"], lost)
    off, _ = ticks_after(lossy, False)
    assert np.array_equal(off, lossless - 320 * lost.astype(np.int64))


def test_talker_selection_does_not_hear_a_late_packet(cuda, oracle_port):
    """Leg 6's packet of tick 10 is the loudest thing its conference ever hears, and it arrives at tick 12, behind the packets of ticks
    11 and 12: late.  The selection runs on the rewritten d_len, so leg 6 is not the talker because of it."""
    script = clean_script(6, steady=True, quiet=True)
    s, pt, _ = script[10][6][0]
    script[12][6].append((s, 8, np.tile(np.array([0x2A, 0xAA], np.uint8), 80)))
    script[10][6] = []
    pk, recv = rows_of(script)
    select = (1, 0, 3)
    want, model, sel = replay_seq(oracle_port, pk, recv, select=select)
    _, _, deaf = replay_seq(oracle_port, pk, recv, select=select, rewrite=False)
    assert model.export()["late"][6] == 1 and model.export()["lost"][6] == 1
    assert not np.array_equal(sel[12][1], deaf[12][1]) and deaf[12][0][6] == 1  # fed the lens as ingest left them, leg 6 would speak
    seen = []
    cb = bridge()
    cb.sequence(True, 3)
    cb.speakers(*select)
    got = run(cb, pk, recv, "ahead", after=lambda t, c: seen.append(c.export_legs()))
    for t in range(T):
        assert np.array_equal(seen[t]["speaking"], sel[t][0]) and np.array_equal(seen[t]["env"], sel[t][1]), ("speaking / env, tick", t)
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    counters_equal(cb, model)
    cb.close()


def test_a_new_call_may_start_at_any_sequence_number(cuda, oracle_port):
    """reset_legs on leg 3 at tick 15; from then on its sender counts from an unrelated number.  No resync and nothing late is counted,
    and every datagram is the replay's in which leg 3's ring, cursor, sender and sequence state were made fresh at tick 15."""
    script = clean_script(7, steady=True)
    for t in range(15, T):
        script[t][3] = [((s + 30000) % 65536, pt, codes) for s, pt, codes in script[t][3]]
    pk, recv = rows_of(script)
    want, model, _ = replay_seq(oracle_port, pk, recv, fresh_at={15: [3]})
    stale, stale_model, _ = replay_seq(oracle_port, pk, recv)
    assert stale_model.export()["resync"][3] == 1 and not any(model.export()[name].any() for name in COUNTERS)
    cb = bridge()
    cb.sequence(True, 3)
    got = run(cb, pk, recv, "ahead", before={15: lambda c: c.reset_legs([3])})
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    counters_equal(cb, model)
    assert got[15, 3, 2:4].tolist() == [0, 0] and not np.array_equal(got[15:, 3], stale[15:, 3])
    cb.close()


def test_sequence_refusals(cuda, wmx):
    cb = bridge()
    assert wmx.wmx_conf_sequence(cb._h, 1, 4) == EINVAL and wmx.wmx_conf_sequence(cb._h, 1, -1) == EINVAL
    assert wmx.wmx_conf_sequence(None, 1, 3) == EINVAL
    assert wmx.wmx_conf_export_sequence(None, None, None, None, None, None, None, None, None) == EINVAL
    st = cb.export_sequence()
    assert not any(st[name].any() for name in st)
    cb.close()
