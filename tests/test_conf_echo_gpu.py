"""wmx_conf_echo (wmix_amd/csrc/conf.hip) through the Python mirror: the conference bridge with every leg's rows going through the leg's
own echo canceller, what the handle sent to the leg as its far end.  The replay is ConfEchoReplay of tests/conf_echo_replay.py, which
ticks tests/leg_echo_model.py where include/wmix_amd.h places the stage: the rows between the denoiser and the leveller, the far row
behind the egress.  Layout, K = 3 and the scripts are those of tests/conf_inputs.py, the runner that of tests/conf_harness.py: every
datagram of every tick, speaking / env and export_echo after every tick, and at the end head, tick and dropped and what the sequencer,
the concealment, the codecs and the gate export.  Bytes and integers, np.array_equal."""
import functools

import numpy as np
import pytest

from conf_echo_replay import ECHO_FIELDS, ConfEchoReplay, replay_echo_story
from conf_harness import MODES, bridge, run
from conf_inputs import EINVAL, G, K, LAYOUT, SEED, T, alaw_decode, arrivals, clean_script, impair, rows_of
from conf_replay_model import replay_story
from conf_stories import everything, plain_setup
from leg_echo_inputs import talk

pytestmark = pytest.mark.gpu

DELAY = 20
ON_AT, RESET_AT, RESET_LEGS, OFF_AT = 10, 20, [1, 6], 30
REPLAYED = {}


def with_echo(setup, delay=DELAY):
    def both(c):
        setup(c)
        c.echo(True, delay)
    return both


def stories(lib):
    """name -> () -> (pk, recv, setup, before)"""
    def full():
        pk, recv, setup, before = everything(lib, True, True, gate=True)
        return pk, recv, with_echo(setup), before

    switched = {ON_AT: lambda c: c.echo(True, DELAY), RESET_AT: lambda c: c.reset_legs(RESET_LEGS), OFF_AT: lambda c: c.echo(False)}
    return {"clean": lambda: rows_of(clean_script(41)) + (with_echo(plain_setup), None),
            "impaired": lambda: rows_of(impair(clean_script(42), 43)[0]) + (with_echo(plain_setup), None),
            "everything": full,
            "switched": lambda: arrivals(SEED, T, G) + (plain_setup, switched)}


def expected(lib, name):
    if name not in REPLAYED:
        pk, recv, setup, before = stories(lib)[name]()
        want, legs, m = replay_echo_story(lib, G, K, pk, recv, setup, before)
        REPLAYED[name] = {"pk": pk, "recv": recv, "setup": setup, "before": before, "want": want, "legs": legs, "model": m}
    return REPLAYED[name]


def echo_equals(got, want, where):
    for name in ECHO_FIELDS:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (where, name, got[name], want[name])


def handle_equals_replay(e, slots, mode, n=G, k=K):
    pk, recv, m = e["pk"], e["recv"], e["model"]
    cb, seen = bridge(n, slots, None, k), []
    e["setup"](cb)
    got = run(cb, pk, recv, mode, before=e["before"], after=lambda t, c: seen.append((c.export_legs(), c.export_echo())))
    end = (cb.export_legs(), cb.export_sequence(), cb.export_conceal(), cb.export_codecs(), cb.export_gate())
    cb.close()
    assert np.array_equal(got, e["want"]), np.argwhere((got != e["want"]).any(2))[:6]
    for t in range(recv.shape[0]):
        for name in ("speaking", "env"):
            assert np.array_equal(seen[t][0][name], e["legs"][t][name]), (name, "tick", t)
        echo_equals(seen[t][1], m.echo_seen[t], ("tick", t))
    for name in ("head", "tick", "dropped"):
        assert np.array_equal(end[0][name], e["legs"][-1][name]), name
    for have, want in ((end[1], m.export_sequence()), (end[3], m.export_codecs()), (end[4], m.export_gate())):
        for name in want:
            assert np.array_equal(have[name], want[name]), (name, have[name], want[name])
    assert np.array_equal(end[2], m.export_conceal())
    return e


@pytest.mark.parametrize("slots,mode", MODES)
@pytest.mark.parametrize("name", ["clean", "impaired"])
def test_echo_alone(cuda, oracle_port, name, slots, mode):
    e = handle_equals_replay(expected(oracle_port, name), slots, mode)
    plain, _, _ = replay_story(oracle_port, G, K, e["pk"], e["recv"], plain_setup)
    last = e["model"].echo_seen[-1]
    # the cancellers leave their start-up and rewrite rows: other datagrams than the plain handle's
    assert (last["startup"][:9] == 0).all() and not np.array_equal(plain, e["want"])


@pytest.mark.parametrize("slots,mode", MODES)
def test_every_stage_on(cuda, oracle_port, slots, mode):
    e = handle_equals_replay(expected(oracle_port, "everything"), slots, mode)
    m = e["model"]
    assert m.echo_on and m.level_on and m.denoise_on and m.gate_on and m.seq_on and m.conceal_on and m.max_speakers > 0
    without = replay_story(oracle_port, G, K, e["pk"], e["recv"], *everything(oracle_port, True, True, gate=True)[2:])[0]
    assert not np.array_equal(without, e["want"])


@pytest.mark.parametrize("slots,mode", MODES)
def test_echo_switched_on_a_running_handle_reset_legs_and_off(cuda, oracle_port, slots, mode):
    e = handle_equals_replay(expected(oracle_port, "switched"), slots, mode)
    seen, want = e["model"].echo_seen, e["want"]
    plain, _, _ = replay_story(oracle_port, G, K, e["pk"], e["recv"], plain_setup, {RESET_AT: e["before"][RESET_AT]})
    assert np.array_equal(want[:ON_AT], plain[:ON_AT]) and not np.array_equal(want[ON_AT:OFF_AT], plain[ON_AT:OFF_AT])
    assert all((s["startup"] == 1).all() and (s["delay_blocks"] == -2).all() for s in seen[:ON_AT])
    # a leg reset while the stage is on starts over; off: nothing moves
    assert seen[RESET_AT - 1]["startup"][RESET_LEGS].tolist() == [0, 0] and seen[RESET_AT]["startup"][RESET_LEGS].tolist() == [1, 1]
    for t in range(OFF_AT, T):
        echo_equals(seen[t], seen[OFF_AT - 1], ("off, tick", t))


def test_a_handle_that_never_hears_of_echo_is_the_parent_model(cuda, oracle_port, wmx):
    pk, recv = arrivals(SEED, T, G)
    want, _, _ = replay_story(oracle_port, G, K, pk, recv, plain_setup)
    for touch in (False, True):
        cb = bridge()
        if touch:
            cb.echo(False, 9999)  # off does not look at the delay
            assert wmx.wmx_conf_echo(cb._h, 1, 501) == EINVAL and wmx.wmx_conf_echo(cb._h, 1, -1) == EINVAL  # refused: nothing made
        got = run(cb, pk, recv, "ahead")
        assert cb.canceller_state(0) is None and not wmx.wmx_conf_canceller(cb._h)
        echo_equals(cb.export_echo(), ConfEchoReplay(oracle_port, G, K).export_echo(), "never on")
        assert wmx.wmx_conf_export_echo(cb._h, None, None, None, None, None) == 0  # any pointer may be NULL
        cb.close()
        assert np.array_equal(got, want)
    assert wmx.wmx_conf_echo(None, 1, 20) == EINVAL and not wmx.wmx_conf_canceller(None)


def test_the_cancellers_state_is_kept_through_off_and_on_and_a_legs_delay_is_its_own(cuda, oracle_port):
    pk, recv = arrivals(SEED, T, G)
    cb = bridge()
    cb.echo(True, DELAY)
    fresh = cb.canceller_state(3)
    run(cb, pk[:8], recv[:8], "ahead")
    moved = [cb.canceller_state(g) for g in range(G)]
    assert all(not np.array_equal(b, fresh) for b in moved)
    cb.echo(False)
    run(cb, pk[8:11], recv[8:11], "ahead")
    assert all(np.array_equal(cb.canceller_state(g), moved[g]) for g in range(G))
    cb.set_leg_echo_delay([2], 200)
    cb.reset_legs([2, 3])
    assert np.array_equal(cb.canceller_state(3), fresh) and not np.array_equal(cb.canceller_state(2), fresh)  # the delay stays
    assert np.array_equal(cb.canceller_state(2)[:-4], fresh[:-4]) and cb.canceller_state(2)[-4:].view(np.int32)[0] == 200
    cb.close()


# ---- what it is for
GAIN, ECHO_DELAY, REPORTED, TICKS, MEASURED = 0.8, 517, 0, 250, 0.17


@functools.lru_cache(maxsize=None)
def speakerphone(lib):
    """A conference of two: leg 0 sends talk(seed 1) as A-law, one packet a tick; leg 1 is a speakerphone -- each of its packets is
    GAIN x what the model sent to leg 1 ECHO_DELAY samples earlier, re-encoded, made by running the model closed-loop
    -> (pk, recv, the model's datagrams with echo control on)"""
    from oracle import loader
    enc = lambda x: loader._g711(lib, "orc_PCM2G711a", np.ascontiguousarray(x, np.int16), np.uint8, 320)[0]  # noqa: E731
    speech, sent = talk(TICKS * 160, 1), np.zeros(TICKS * 160, np.int16)
    m = ConfEchoReplay(lib, 2, 1)
    m.set_conferences([[0, 1]])
    m.echo(True, REPORTED)
    pk, recv = np.full((TICKS, 2, 1, 172), 0xEE, np.uint8), np.full((TICKS, 2, 1), 172, np.int32)
    out = np.zeros((TICKS, 2, 172), np.uint8)
    for t in range(TICKS):
        at = np.arange(t * 160, (t + 1) * 160) - ECHO_DELAY
        echo = np.rint(np.where(at >= 0, sent[np.maximum(at, 0)], 0) * GAIN).astype(np.int16)
        for g, row in enumerate((speech[t * 160:(t + 1) * 160], echo)):
            pk[t, g, 0, :12] = 0
            pk[t, g, 0, :4] = 0x80, 0x80 | 8, (t >> 8) & 255, t & 255
            pk[t, g, 0, 12:] = enc(row)
        out[t] = m.tick(pk[t], recv[t])
        sent[t * 160:(t + 1) * 160] = m.far_rows[-1][1]
    return pk, recv, out


def test_a_speakerphone_on_one_leg_is_cancelled_for_the_other(cuda, oracle_port):
    """What leg 0 hears of its own voice coming back from leg 1, rms over the second half of 5 s, echo control on against off, on the
    model; the handle sends the model's bytes both times.  Measured on the model (the oracle, not the code under test) with the echo at
    0.8 x, 517 samples late and a reported delay of 0 ms: 85.5 against 505.3, 0.17; the test asserts twice that, capped at 0.3.  The
    residual is the canceller's comfort noise (rms about 80 whatever the echo's level).  The input is not the one first proposed
    (0.3 x, reported delay 20 ms): there the model gives 131 against 239, 0.55, for talk(seed 1) and 0.28 / 0.32 for seeds 2 / 3 -- with
    20 ms reported this talker's echo has not converged within 5 s at any gain tried (0.42 .. 0.50), with 0 ms it has at every echo
    delay from 197 to 1157 samples (0.17 .. 0.20 at 0.8 x; 0.24 .. 0.27 at 0.5 x)."""
    pk, recv, on = speakerphone(oracle_port)
    setup = lambda c: c.set_conferences([[0, 1]])  # noqa: E731
    off, _, _ = replay_echo_story(oracle_port, 2, 1, pk, recv, setup)
    for want, story in ((off, setup), (on, with_echo(setup, REPORTED))):
        cb = bridge(2, 3, None, 1)
        story(cb)
        got = run(cb, pk, recv, "ahead")
        cb.close()
        assert np.array_equal(got, want)
    rms = [float(np.sqrt((alaw_decode(o[TICKS // 2:, 0, 12:].reshape(-1)).astype(np.float64) ** 2).mean())) for o in (off, on)]
    print("rms of what leg 0 hears over the second half: echo control off %.1f, on %.1f, on / off %.4f" % (rms[0], rms[1], rms[1] / rms[0]))
    assert rms[0] > 400 and rms[1] <= min(2 * MEASURED, 0.3) * rms[0], rms
