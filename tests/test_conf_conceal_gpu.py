"""wmx_conf_conceal (wmix_amd/csrc/conf.hip) through the Python mirror: the conference bridge with its legs sequenced and the gaps
concealed from each leg's own history.  Layout, T, K and the scripts are those of tests/conf_inputs.py, the runner that of
tests/conf_harness.py.  The reference is replay_conceal() of tests/conf_single_replays.py: the tick-by-tick replay fed the rows
tests/leg_plc_model.py makes of the call lists of tests/leg_seq_model.py, four slots per leg, every one a data call.  Bytes and
integers, np.array_equal."""
import numpy as np
import pytest

from conf_harness import bridge, counters_equal, run
from conf_inputs import EINVAL, G, IN_CONF, T, clean_script, impair, rows_of, tone_script
from conf_single_replays import replay_conceal, replay_seq
from leg_seq_model import COUNTERS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def impaired():
    script, _ = impair(clean_script(2), 3)
    return rows_of(script)


def test_an_impaired_script_is_sent_as_the_replay_of_the_concealed_rows(cuda, oracle_port, impaired):
    pk, recv = impaired
    want, seq, plc, _ = replay_conceal(oracle_port, pk, recv)
    silent, _, _ = replay_seq(oracle_port, pk, recv)
    concealed = plc.export()["concealed"]
    assert concealed[IN_CONF].sum() >= 3 and np.array_equal(concealed, seq.export()["lost"]) and not np.array_equal(want, silent)
    for mode in ("ahead", "resident"):
        cb = bridge(slots=3)
        cb.sequence(True, 3)
        cb.conceal(True)
        got = run(cb, pk, recv, mode)
        assert np.array_equal(got, want), (mode, np.argwhere((got != want).any(2))[:6])
        counters_equal(cb, seq)
        assert np.array_equal(cb.export_conceal(), concealed), (mode, cb.export_conceal(), concealed)
        assert not cb.export_legs()["dropped"].any()
        cb.close()
    # concealment off, the same script is sent with the gaps as zeros
    cb = bridge()
    cb.sequence(True, 3)
    got = run(cb, pk, recv, "ahead")
    assert np.array_equal(got, silent) and not np.array_equal(got, want) and not cb.export_conceal().any()
    cb.close()


def test_concealment_switched_off_again_is_concealment_never_touched(cuda, impaired):
    pk, recv = impaired
    sent = []
    for touch in (False, True):
        cb = bridge()
        cb.sequence(True, 3)
        if touch:
            cb.conceal(True)
            cb.conceal(False)
        sent.append(run(cb, pk, recv, "ahead"))
        assert not cb.export_conceal().any()
        cb.close()
    assert np.array_equal(sent[0], sent[1])
    # and without sequencing the stage is not run: the bytes of a handle with both off, the state where it was
    both = []
    for on in (False, True):
        cb = bridge()
        cb.conceal(on)
        both.append(run(cb, pk[:12], recv[:12], "ahead"))
        assert not cb.export_conceal().any()
        cb.close()
    assert np.array_equal(both[0], both[1])


def test_a_clean_script_is_sent_as_with_concealment_off(cuda):
    pk, recv = rows_of(clean_script(1))
    sent = []
    for on in (False, True):
        cb = bridge()
        cb.sequence(True)
        cb.conceal(on)
        sent.append(run(cb, pk, recv, "resident" if on else "ahead"))
        assert not cb.export_conceal().any() and not any(cb.export_sequence()[name].any() for name in COUNTERS)
        cb.close()
    assert np.array_equal(sent[0], sent[1]) and (sent[0][:, IN_CONF, 12:] != 0xD5).any()


def test_the_other_legs_hear_the_tone_go_on_through_a_lost_packet(cuda, oracle_port):
    """What the feature is for.  Leg 6 loses the packet of tick 12; when the next one arrives (tick 13) the gap is loaded ten ticks
    ahead of the play head, so the rings of the legs that hear leg 6 hold it: with concealment on, the tone continued -- exactly the
    samples the lost packet held, under the gain -- on top of the other talkers; with it off, the other talkers alone."""
    lost_at, ticks = 12, 14
    script, period = tone_script(lost_at)
    pk, recv = rows_of(script)
    pk, recv = pk[:ticks], recv[:ticks]
    _, _, plc, rp_on = replay_conceal(oracle_port, pk, recv)
    assert plc.legs[6].lags == [50] and plc.export()["concealed"].tolist() == [0] * 6 + [1] + [0] * 3
    k = np.arange(160, dtype=np.int64)
    row = (period.astype(np.int64)[(lost_at * 160 + k) % 50] * (32768 - 68 * k)) >> 15  # the lost packet under the gain
    assert np.abs(row).max() > 1000

    def rings_after(on):
        cb = bridge()
        cb.sequence(True, 3)
        cb.conceal(on)
        run(cb, pk, recv, "wait")
        rings, tick6 = {g: cb.export_ring(g)[0] for g in (5, 7, 8)}, int(cb.export_legs()["tick"][6])
        assert cb.export_conceal()[6] == (1 if on else 0)
        cb.close()
        return rings, tick6

    on, tick_on = rings_after(True)
    off, tick_off = rings_after(False)
    assert tick_on == tick_off  # the cursor is the sequencer's business, with or without
    gap = (((tick_on - 640) % 16000) // 2 + np.arange(160)) % 8000  # leg 6's cursor stands behind S D
    for g in (5, 7, 8):
        ref = rp_on.orc.rings.store[g][:16000].view(np.int16)
        assert np.array_equal(on[g], ref), ("ring of leg", g, np.flatnonzero(on[g] != ref)[:6])
        assert np.abs(off[g][gap].astype(np.int64)).max() < 200  # two or three quiet talkers
        assert np.array_equal(on[g][gap].astype(np.int64) - off[g][gap], row), ("ring of leg", g)
        assert on[g][gap].any()


def test_a_reset_leg_conceals_from_a_fresh_history(cuda, wmx, oracle_port):
    """reset_legs([3]) at tick 15 zeroes leg 3's history and count with the rest of its state; the new call loses its second packet
    (tick 16), and the gap is concealed from a history whose older half is still zero -- the replay with leg 3 made fresh at tick
    15, not the one whose concealment state lived on.  (A gap cannot meet a history that is zero throughout: the sequencer makes a
    silence call only once the leg is synced, that is behind a data call made since the reset, and that call is in the history.  What is zero is read back right
    after the reset, and the older half of what the gap is concealed from.)"""
    script = clean_script(7, steady=True)
    for t in range(15, T):
        script[t][3] = [((s + 30000) % 65536, pt, codes) for s, pt, codes in script[t][3]]
    script[9][3], script[16][3] = [], []
    pk, recv = rows_of(script)
    want, seq, plc, _ = replay_conceal(oracle_port, pk, recv, fresh_at={15: [3]})
    stale, _, stale_plc, _ = replay_conceal(oracle_port, pk, recv, fresh_at={15: [3]}, plc_fresh=False)
    assert plc.export()["concealed"][3] == 1 and stale_plc.export()["concealed"][3] == 2 and not np.array_equal(want, stale)
    seen = {}

    def reset(c):
        c.reset_legs([3])
        hist = np.zeros((G, 320), np.int16)
        assert wmx.wmx_rtp_export_conceal(wmx.wmx_conf_senders(c._h), hist.ctypes.data, None, None) == 0
        seen["hist"], seen["concealed"] = hist, c.export_conceal()

    cb = bridge()
    cb.sequence(True, 3)
    cb.conceal(True)
    got = run(cb, pk, recv, "ahead", before={15: reset})
    assert not seen["hist"][3].any() and seen["hist"][[2, 4]].any(1).all() and seen["concealed"][3] == 0
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    counters_equal(cb, seq)
    assert np.array_equal(cb.export_conceal(), plc.export()["concealed"])
    cb.close()


def test_conceal_refusals(cuda, wmx):
    assert wmx.wmx_conf_conceal(None, 1) == EINVAL and wmx.wmx_conf_export_conceal(None, None, None) == EINVAL
    cb = bridge()
    assert not cb.export_conceal().any()
    bad = np.array([3, G], np.int32)
    cb.conceal(True)
    assert wmx.wmx_conf_reset_legs(cb._h, bad.ctypes.data, 2, None) == EINVAL
    cb.close()
