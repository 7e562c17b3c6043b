"""wmx_conf_level (wmix_amd/csrc/conf.hip) through the Python mirror: the conference bridge with every leg's rows going through the
leg's own AGC.  The replay is ConfReplay of tests/conf_replay_model.py, which has tests/leg_dtmf_model.py, tests/leg_denoise_model.py
and tests/leg_level_model.py where include/wmix_amd.h places the stages: behind the sequencer, DTMF detection first (on the row as it
arrived), then the suppressor, then the AGC, then the selection, the concealment and the load on the levelled rows.  Layout, K = 3 and
the scripts are those of tests/conf_inputs.py, the stories those of tests/conf_stories.py, the runner and the handle / replay
comparison those of tests/conf_harness.py: every datagram of every tick and speaking / env after every tick are compared, and at the
end head, tick and dropped and what the sequencer, the concealment and the codecs export.  Bytes and integers, np.array_equal."""
import numpy as np
import pytest

from conf_harness import MODES, bridge, expected, handle_equals_replay, run
from conf_inputs import EINVAL, G, K, KEY_LEG, LAYOUT, SEED, T, arrivals, one_talker, ulaw_decode
from conf_replay_model import replay_story
from conf_stories import VALUE, alone, everything, regained, switched
from leg_codec_model import LAW_U, PCMU

pytestmark = pytest.mark.gpu

REFUSED = (187, 200)  # compression gains the AGC's gain table cannot be made for: 0 .. 186 dB are the ones it can


def level_alone(lib):
    return expected(("level", "alone"), lib, G, K, lambda: alone("level"))


def gains_of(cb):
    from wmix_amd._lib import lib
    agc = lib().wmx_conf_leveller(cb._h)
    return [lib().wmx_agc_stream_gain(agc, g) for g in range(cb.n_legs)]


# ---- a. level alone
@pytest.mark.parametrize("slots,mode", MODES)
def test_level_alone(cuda, oracle_port, slots, mode):
    e = handle_equals_replay(level_alone(oracle_port), slots, mode)
    pk, recv, want, m = e["pk"], e["recv"], e["want"], e["model"]
    plain, _, _ = replay_story(oracle_port, G, K, pk, recv, lambda c: c.set_conferences(LAYOUT))
    assert not np.array_equal(want[:, :9], plain[:, :9]) and np.array_equal(want[:, 9], plain[:, 9])  # leg 9 hears nobody
    assert all(len(h) > 0 for h in m.lv.history)  # a leg in no conference is levelled all the same: the load is where it is left out


# ---- b. every stage on, on an impaired schedule
@pytest.mark.parametrize("slots,mode", [(3, "ahead"), (3, "resident")])
def test_every_stage_on(cuda, oracle_port, slots, mode):
    e = handle_equals_replay(expected(("level", "everything"), oracle_port, G, K, lambda: everything(oracle_port, True, True)), slots, mode)
    m, st = e["model"], e["model"].export_sequence()
    assert m.keys.export()["count"][KEY_LEG] >= 1 and m.export_conceal().sum() >= 1 and not m.export_legs()["dropped"].any()
    assert st["lost"].any() and st["late"].any() and st["dup"].any()
    # the same story, with the same floor, with level off sends other bytes
    off = expected(("level", "everything off"), oracle_port, G, K, lambda: everything(oracle_port, True, False, floor_from=True))
    assert np.array_equal(off["pk"], e["pk"]) and not np.array_equal(off["want"], e["want"])


# ---- c. level switched on a running handle, a leg reset, off and on again
@pytest.mark.parametrize("slots,mode", MODES[1:])
def test_level_switched_on_a_running_handle_and_a_reset_leg(cuda, oracle_port, slots, mode):
    """on at tick 8; legs 1 and 6 get a gain of their own at 12; leg 1 is a new call at tick 16 (its AGC starts again, on the gain it
    has); off at 22 -- the state stays as it stood, but for leg 6, reset at tick 26 while the stage is off -- and on again at 30 with
    the value of before: no leg's gain changes"""
    e = handle_equals_replay(expected(("level", "switched"), oracle_port, G, K, lambda: switched("level")), slots, mode)
    pk, recv, setup, before, want, m = e["pk"], e["recv"], e["setup"], e["before"], e["want"], e["model"]
    plain, _, _ = replay_story(oracle_port, G, K, pk, recv, setup, {t: f for t, f in before.items() if t in (16, 26)})
    assert np.array_equal(want[:8], plain[:8]) and not np.array_equal(want[8:22], plain[8:22]) and not np.array_equal(want[30:], plain[30:])
    assert m.lv.gain == [VALUE, 9] + [VALUE] * 4 + [9] + [VALUE] * 3
    # the reset matters: without it leg 0 hears leg 1 through an AGC that has adapted; and so does the gain it kept
    kept, _, _ = replay_story(oracle_port, G, K, pk, recv, setup, {t: f for t, f in before.items() if t != 16})
    assert not np.array_equal(kept[16:, 0], want[16:, 0])
    same_gain, _, _ = replay_story(oracle_port, G, K, pk, recv, setup, {t: f for t, f in before.items() if t != 12})
    assert not np.array_equal(same_gain[12:, 0], want[12:, 0])


def test_the_gains_and_the_state_are_kept_through_off_and_on(cuda):
    pk, recv = arrivals(SEED, T, G)
    cb = bridge()
    cb.level(True, VALUE)
    cb.set_leg_gain([1, 6], 9)
    fresh = cb.leveller_state(3)
    run(cb, pk[:6], recv[:6], "ahead")
    moved = [cb.leveller_state(g) for g in range(G)]
    assert not np.array_equal(moved[3], fresh)
    cb.level(False)
    run(cb, pk[6:9], recv[6:9], "ahead")
    assert all(np.array_equal(cb.leveller_state(g), moved[g]) for g in range(G))  # off: the state does not move
    cb.reset_legs([1, 3])
    cb.level(True, VALUE)
    assert np.array_equal(cb.leveller_state(3), fresh) and gains_of(cb) == [VALUE, 9] + [VALUE] * 4 + [9] + [VALUE] * 3
    assert not np.array_equal(cb.leveller_state(1), fresh) and np.array_equal(cb.leveller_state(1)[:-4], fresh[:-4])  # all but its gain
    assert all(np.array_equal(cb.leveller_state(g), moved[g]) for g in range(G) if g not in (1, 3))
    cb.reset_legs()  # every leg
    assert all(np.array_equal(cb.leveller_state(g)[:-4], fresh[:-4]) for g in range(G)) and gains_of(cb)[6] == 9
    cb.level(True, 12)  # another value: every leg
    assert gains_of(cb) == [12] * G
    cb.close()


# ---- d. another value on a made handle, and one leg's volume
@pytest.mark.parametrize("slots,mode", MODES[1:])
def test_another_value_and_one_legs_gain_are_agc_addition_at_that_tick(cuda, oracle_port, slots, mode):
    e = handle_equals_replay(expected(("level", "regained"), oracle_port, G, K, regained), slots, mode)
    pk, recv, setup, before, want, m = e["pk"], e["recv"], e["setup"], e["before"], e["want"], e["model"]
    assert m.lv.gain == [9, 9, 30] + [9] * 7 and all(a for a in m.lv.additions)
    base = level_alone(oracle_port)["want"]  # the same script and setup
    only14, _, _ = replay_story(oracle_port, G, K, pk, recv, setup, {14: before[14]})
    assert np.array_equal(want[:14], base[:14]) and not np.array_equal(want[14:24], base[14:24])
    assert np.array_equal(want[:24], only14[:24]) and not np.array_equal(want[24:, 3:5], only14[24:, 3:5])  # legs 3 and 4 hear leg 2


# ---- e. before the first switch-on, NULL, and a value that is refused
def test_level_off_on_a_handle_that_was_never_on_changes_nothing(cuda, wmx):
    pk, recv = arrivals(SEED, T, G)
    sent = []
    for touch in (False, True):
        cb = bridge()
        if touch:
            cb.level(False)
            for v in REFUSED:  # the first switch-on refused: nothing is made
                assert wmx.wmx_conf_level(cb._h, 1, v) == EINVAL and b"compression gain" in wmx.wmx_last_error()
        sent.append(run(cb, pk, recv, "ahead"))
        assert cb.leveller_state(0) is None and not wmx.wmx_conf_leveller(cb._h)
        cb.close()
    assert np.array_equal(sent[0], sent[1])
    assert wmx.wmx_conf_level(None, 1, VALUE) == EINVAL and wmx.wmx_conf_level(None, 0, VALUE) == EINVAL and not wmx.wmx_conf_leveller(None)


def test_a_refused_value_changes_nothing_on_a_running_handle(cuda, wmx, oracle_port):
    e = level_alone(oracle_port)
    pk, recv, setup, want = e["pk"], e["recv"], e["setup"], e["want"]

    def refused(c):
        for v in REFUSED:
            assert wmx.wmx_conf_level(c._h, 1, v) == EINVAL and b"compression gain" in wmx.wmx_last_error()
            with pytest.raises(Exception, match="compression gain"):
                c.set_leg_gain([2], v)
        assert gains_of(c) == [VALUE] * G

    cb = bridge()
    setup(cb)
    got = run(cb, pk, recv, "ahead", before={10: refused, 20: refused})
    cb.close()
    assert np.array_equal(got, want)


# ---- f. what it is for
def test_a_quiet_leg_is_heard_nearer_to_a_loud_one(cuda):
    """A conference of three, level(True, 20).  Leg 0 sends voiced bursts at amplitude 10 000, leg 1 the same signal at amplitude 1 000,
    each alone in a run of 6 s; what leg 2 is sent, decoded, over the last 2 s has an rms r0 while leg 0 talks and r1 while leg 1 talks.
    r0 / r1 with level on is at most 0.7 of r0 / r1 with level off.  The oracle alone (one agc of value 20 over the mu-law round trip
    of each signal, the last 2 s) gives 15 406 / 5 613 = 2.745 against 10 596 / 1 061 = 9.987 going in: 0.275 of it; the handle
    measured 15 378 / 5 568 = 2.762 against 10 596 / 1 061 = 9.987: 0.277 (what leg 2 is sent has been through the mu-law encoder once
    more).  The cap is a condition on the wiring, not a measure of quality."""
    ticks, tail = 300, 100
    rms = {}
    for on in (False, True):
        for talker, amp in ((0, 10000), (1, 1000)):
            pk, recv = one_talker(talker, amp, ticks)
            cb = bridge(3, 3, [[0, 1, 2]])
            cb.set_codecs(None, PCMU, LAW_U)
            cb.level(on, VALUE)
            out = run(cb, pk, recv, "ahead")
            cb.close()
            heard = ulaw_decode(out[-tail:, 2, 12:].reshape(-1)).astype(np.float64)
            rms[on, talker] = float(np.sqrt((heard ** 2).mean()))
    off, on = rms[False, 0] / rms[False, 1], rms[True, 0] / rms[True, 1]
    print("rms of the last 2 s: off %.1f / %.1f = %.3f, on %.1f / %.1f = %.3f, on / off %.3f"
          % (rms[False, 0], rms[False, 1], off, rms[True, 0], rms[True, 1], on, on / off))
    assert 9.0 < off < 11.0 and on <= 0.7 * off, rms
