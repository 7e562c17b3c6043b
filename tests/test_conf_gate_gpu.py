"""wmx_conf_gate (wmix_amd/csrc/conf.hip) through the Python mirror: the conference bridge with every leg's rows going through the leg's
own voice-activity gate.  The replay is ConfReplay of tests/conf_replay_model.py, which ticks tests/leg_gate_model.py where
include/wmix_amd.h places the stage: directly behind the AGC and in front of the selection, the concealment and the load, which see the
gated rows; the stories are those of tests/conf_stories.py.  Layout, K = 3 and the scripts are those of tests/conf_inputs.py, the runner and the handle / replay comparison those of
tests/conf_harness.py: every datagram of every tick and speaking / env after every tick are compared, and at the end head, tick and
dropped and what the sequencer, the concealment and the codecs export; export_gate is compared after every tick.  Bytes and integers,
np.array_equal."""
import numpy as np
import pytest

from conf_harness import MODES, bridge, expected, handle, handle_equals_replay, run
from conf_inputs import EINVAL, G, K, KEY_LEG, SEED, T, arrivals, noise_script, ulaw_decode
from conf_replay_model import ConfReplay, replay_story
from conf_stories import (OFF_AT, ON_AGAIN_AT, ON_AT, RESET_OFF_AT, RESET_OFF_LEG, RESET_ON_AT, RESET_ON_LEG, alone, everything, plain_setup,
                          switched)
from leg_codec_model import LAW_U, PCMU

pytestmark = pytest.mark.gpu

GATE_FIELDS = ("reduce", "voiced", "unvoiced")


def gate_equals(got, want, where):
    for name in GATE_FIELDS:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (where, name, got[name], want[name])


# ---- a. the gate alone
@pytest.mark.parametrize("slots,mode", MODES)
def test_gate_alone(cuda, oracle_port, slots, mode):
    e = handle_equals_replay(expected("gate alone", oracle_port, G, K, lambda: alone("gate")), slots, mode)
    pk, recv, want, m = e["pk"], e["recv"], e["want"], e["model"]
    plain, _, _ = replay_story(oracle_port, G, K, pk, recv, plain_setup)
    # the oracle on random codes: a call's first four rows are attenuated (reduce 4, 3, 2, 1), from the fifth on the gate is open
    assert all(tr[:5] == [4, 3, 2, 1, 0] and set(tr[5:]) == {0} for tr in m.gt.trace)
    fed = np.array([s["voiced"].astype(int) + s["unvoiced"] for s in m.gate_seen])  # [tick, leg] rows fed so far
    fourth = max(int(np.argmax(fed[:, g] >= 4)) for g in range(G))  # the tick in which the last leg was fed its fourth row
    differs = np.flatnonzero((want != plain).any((1, 2)))
    # so the datagrams differ from the plain handle's where those rows are heard and nowhere else: from the tick the first row leaves
    # the rings to that many ticks behind the last attenuated row
    assert len(differs) and differs[-1] <= fourth + differs[0] < T - 1, (differs, fourth)
    assert all((want[:, g] != plain[:, g]).any() for g in range(9)) and np.array_equal(want[:, 9], plain[:, 9])  # leg 9 hears nobody
    assert all(len(tr) > 0 for tr in m.gt.trace)  # a leg in no conference is gated all the same: the load is where it is left out


# ---- b. every stage on, on the impaired schedule
@pytest.mark.parametrize("slots,mode", MODES)
def test_every_stage_on(cuda, oracle_port, slots, mode):
    e = handle_equals_replay(expected("gate everything", oracle_port, G, K, lambda: everything(oracle_port, True, True, gate=True)), slots, mode)
    m, st = e["model"], e["model"].export_sequence()
    assert m.keys.export()["count"][KEY_LEG] >= 1 and m.export_conceal().sum() >= 1 and not m.export_legs()["dropped"].any()
    assert st["lost"].any() and st["late"].any() and st["dup"].any()
    assert m.level_on and m.denoise_on and m.gate_on and m.gt.voiced.all()
    # the same story with the gate off sends other bytes
    off = expected(("level", "everything"), oracle_port, G, K, lambda: everything(oracle_port, True, True))  # the level tests' replay
    assert np.array_equal(off["pk"], e["pk"]) and off["model"].gt is None and not np.array_equal(off["want"], e["want"])


# ---- c. the gate switched on a running handle, a leg reset while it is on and one while it is off
@pytest.mark.parametrize("slots,mode", MODES)
def test_gate_switched_on_a_running_handle_and_reset_legs(cuda, oracle_port, slots, mode):
    e = handle_equals_replay(expected("gate switched", oracle_port, G, K, lambda: switched("gate")), slots, mode)
    pk, recv, before, want, m = e["pk"], e["recv"], e["before"], e["want"], e["model"]
    resets = {t: f for t, f in before.items() if t in (RESET_ON_AT, RESET_OFF_AT)}
    plain, _, _ = replay_story(oracle_port, G, K, pk, recv, plain_setup, resets)
    assert np.array_equal(want[:ON_AT], plain[:ON_AT]) and not np.array_equal(want[ON_AT:OFF_AT], plain[ON_AT:OFF_AT])
    seen = m.gate_seen
    assert all((s["reduce"] == 4).all() and not s["voiced"].any() and not s["unvoiced"].any() for s in seen[:ON_AT])
    # a leg reset while the gate is on: shut again, its counts from zero
    assert seen[RESET_ON_AT - 1]["reduce"][RESET_ON_LEG] == 0 and seen[RESET_ON_AT - 1]["voiced"][RESET_ON_LEG] > 4
    assert seen[RESET_ON_AT]["reduce"][RESET_ON_LEG] >= 3 and seen[RESET_ON_AT]["voiced"][RESET_ON_LEG] + seen[RESET_ON_AT]["unvoiced"][RESET_ON_LEG] <= 3
    # off: state and counts stay, but for the leg that is reset while it is off
    for t in range(OFF_AT, ON_AGAIN_AT):
        for name in GATE_FIELDS:
            keep = np.arange(G) != RESET_OFF_LEG if t >= RESET_OFF_AT else np.ones(G, bool)
            assert np.array_equal(seen[t][name][keep], seen[OFF_AT - 1][name][keep]), (t, name)
    at = seen[ON_AGAIN_AT - 1]
    assert at["reduce"][RESET_OFF_LEG] == 4 and at["voiced"][RESET_OFF_LEG] == 0 and at["unvoiced"][RESET_OFF_LEG] == 0
    assert seen[-1]["reduce"][RESET_OFF_LEG] == 0 and (seen[-1]["voiced"] > seen[ON_AGAIN_AT - 1]["voiced"]).all()  # on again: it goes on
    # the resets matter: without the one at 16 leg 0 hears leg 1 through a gate that stayed open
    kept, _, _ = replay_story(oracle_port, G, K, pk, recv, plain_setup, {t: f for t, f in before.items() if t != RESET_ON_AT})
    assert not np.array_equal(kept[RESET_ON_AT:, 0], want[RESET_ON_AT:, 0])


# ---- d. export_gate after every tick
@pytest.mark.parametrize("slots,mode", MODES)
def test_export_gate_equals_the_model_after_every_tick(cuda, oracle_port, slots, mode):
    e = expected("gate switched", oracle_port, G, K, lambda: switched("gate"))
    cb, seen = bridge(G, slots, None), []
    e["setup"](cb)
    gate_equals(cb.export_gate(), ConfReplay(oracle_port, G, K).export_gate(), "before the first switch-on")
    got = run(cb, e["pk"], e["recv"], mode, before=e["before"], after=lambda t, c: seen.append(c.export_gate()))
    cb.close()
    assert np.array_equal(got, e["want"])
    # ahead of the wait the tick's launches are queued all the same: the export drains the stream it is given
    for t in range(T):
        gate_equals(seen[t], e["model"].gate_seen[t], ("tick", t))


def test_the_gaters_state_is_kept_through_off_and_on_and_reset_by_reset_legs(cuda):
    pk, recv = arrivals(SEED, T, G)
    cb = bridge()
    assert cb.gater_state(0) is None
    cb.gate(True)
    fresh = cb.gater_state(3)
    assert all(np.array_equal(cb.gater_state(g), fresh) for g in range(G))
    run(cb, pk[:8], recv[:8], "ahead")
    moved = [cb.gater_state(g) for g in range(G)]
    assert all(not np.array_equal(b, fresh) for b in moved) and (cb.export_gate()["reduce"] < 4).all()
    cb.gate(False)
    run(cb, pk[8:11], recv[8:11], "ahead")
    assert all(np.array_equal(cb.gater_state(g), moved[g]) for g in range(G))  # off: the state does not move
    cb.reset_legs([1, 3])
    cb.gate(True)
    assert np.array_equal(cb.gater_state(3), fresh) and np.array_equal(cb.gater_state(1), fresh)
    assert all(np.array_equal(cb.gater_state(g), moved[g]) for g in range(G) if g not in (1, 3))
    st = cb.export_gate()
    assert st["reduce"][[1, 3]].tolist() == [4, 4] and not st["voiced"][[1, 3]].any() and not st["unvoiced"][[1, 3]].any()
    assert (st["voiced"][[0, 2]] > 0).all()
    cb.reset_legs()  # every leg
    st = cb.export_gate()
    assert all(np.array_equal(cb.gater_state(g), fresh) for g in range(G)) and (st["reduce"] == 4).all() and not st["voiced"].any() and not st["unvoiced"].any()
    cb.close()


# ---- e. before the first switch-on, and NULL
def test_gate_off_on_a_handle_that_was_never_on_changes_nothing(cuda, wmx):
    pk, recv = arrivals(SEED, T, G)
    sent = []
    for touch in (False, True):
        cb = bridge()
        if touch:
            cb.gate(False)
        sent.append(run(cb, pk, recv, "ahead"))
        assert cb.gater_state(0) is None and not wmx.wmx_conf_gater(cb._h)
        st = cb.export_gate()
        assert (st["reduce"] == 4).all() and not st["voiced"].any() and not st["unvoiced"].any()
        assert wmx.wmx_conf_export_gate(cb._h, None, None, None, None) == 0  # any pointer may be NULL
        cb.close()
    assert np.array_equal(sent[0], sent[1])
    assert wmx.wmx_conf_gate(None, 1) == EINVAL and wmx.wmx_conf_gate(None, 0) == EINVAL and not wmx.wmx_conf_gater(None)
    assert wmx.wmx_conf_export_gate(None, None, None, None, None) == EINVAL


# ---- f. what it is for
def test_a_leg_that_sends_only_room_noise_is_gated_out_and_holds_no_talker_slot(cuda, oracle_port):
    """A conference of three in mu-law; leg 0 sends stationary noise of sigma 400 for 6 s, the others nothing.  The rms of what leg 2 is
    sent over the last 2 s with the gate on is at most 1 / 8 of that with the gate off: the oracle leaves `reduce` at 4 from the noise's
    10th row on, a shift by 4, about 1 / 16 -- the replay gives 25.5 against 401.7, 0.064, and so did the handle when it was measured.
    The cap is a condition on the wiring, not a measure of quality.  With speakers(1, floor), the floor half way between the levels of the rows the selection is shown with the
    gate on (2 734 .. 3 659 in the replay's tail) and with it off (43 592 .. 58 676), leg 0 is speaking throughout the tail with the
    gate off and never with it on -- tick by tick as the replay says."""
    ticks, tail = 300, 100
    pk, recv = noise_script(3, ticks)

    def story(on, floor=None):
        def setup(c):
            c.set_conferences([[0, 1, 2]])
            c.set_codecs(None, PCMU, LAW_U)
            if floor is not None:
                c.speakers(1, floor, 3)
            c.gate(on)
        return setup

    def held_against_the_replay(on, floor):
        want, legs, m = replay_story(oracle_port, 3, K, pk, recv, story(on, floor))
        got, seen, st = handle(3, 3, pk, recv, story(on, floor), None, "ahead", lambda cb: cb.export_gate())
        assert np.array_equal(got, want)
        for t in range(ticks):
            assert np.array_equal(seen[t]["speaking"], legs[t]["speaking"]) and np.array_equal(seen[t]["env"], legs[t]["env"]), ("tick", t)
        gate_equals(st, m.export_gate(), ("at the end, gate", on))
        if on:
            assert st["reduce"][0] == 4 and st["unvoiced"][0] >= ticks - 10 and st["voiced"][0] + st["unvoiced"][0] == ticks
        return got, seen, m

    # everybody is mixed: what the gate alone does to what leg 2 hears
    rms, shown = {}, {}
    for on in (False, True):
        got, _, m = held_against_the_replay(on, None)
        heard = ulaw_decode(got[-tail:, 2, 12:].reshape(-1)).astype(np.float64)
        rms[on] = float(np.sqrt((heard ** 2).mean()))
        shown[on] = np.array(m.levels[-tail:], np.int64)  # the rows as the selection would be shown them
    print("rms of what leg 2 is sent over the last 2 s: gate off %.1f, gate on %.1f, on / off %.4f" % (rms[False], rms[True], rms[True] / rms[False]))
    assert 300 < rms[False] < 500 and 0 < rms[True] <= rms[False] / 8, rms
    # one talker slot, the floor between the gated and the ungated rows
    assert shown[True].max() < shown[False].min(), (shown[True].max(), shown[False].min())
    floor = int(shown[True].max() + shown[False].min()) // 2
    print("floor %d between the rows' levels with the gate on, at most %d, and off, at least %d" % (floor, shown[True].max(), shown[False].min()))
    for on in (False, True):
        _, seen, _ = held_against_the_replay(on, floor)
        assert all(bool(s["speaking"][0]) == (not on) for s in seen[-tail:]), [int(s["speaking"][0]) for s in seen[-tail:]]
