"""wmx_conf_prompts / _add_clip / _play / _stop / _export_prompts (wmix_amd/csrc/conf.hip, the kernel in mix.hip) through the Python
mirror: announcements and hold music per leg.  The replay is tests/conf_prompt_replay.py -- the reference's orc_load_data on one ring
per leg, the legs' calls and then the prompts' -- installed as the `rp` of the composed replay, or of the one with echo control; the
stories are those of tests/conf_prompt_stories.py (tests/test_conf_prompt_replay.py holds them against what they are for, on the CPU).
G = 10 legs, the family's layout, leg 9 in no conference, 60 ticks.  Every datagram of every tick and export_prompts after every tick,
in the three modes of tests/conf_harness.py.  Bytes and integers, np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from conf_echo_replay import ECHO_FIELDS, ConfEchoReplay
from conf_harness import MODES, bridge, run
from conf_inputs import EINVAL, G, K, SEED, T as T_PLAIN, arrivals
from conf_prompt_replay import replay_prompt_story
from conf_prompt_stories import LONG, MUSIC, T, clips, echo_story, main_story, order_story, stages_script, stages_story, store
from conf_replay_model import replay_story
from conf_stories import floor_of, plain_setup

pytestmark = pytest.mark.gpu

ESTATE = -10003
REPLAYED = {}
PROMPT_FIELDS = ("clip", "pos", "left", "done")


def expected(lib, name, story, **how):
    """story() -> (pk, recv, setup, before); the story and its replay, made once in a session"""
    if name not in REPLAYED:
        pk, recv, setup, before = story()
        want, legs, m = replay_prompt_story(lib, G, K, pk, recv, setup, before, **how)
        REPLAYED[name] = {"pk": pk, "recv": recv, "setup": setup, "before": before, "want": want, "legs": legs, "model": m}
    return REPLAYED[name]


def prompts_equal(got, want, where):
    for name in PROMPT_FIELDS:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (where, name, got[name], want[name])


def handle_equals_replay(e, slots, mode, also=None):
    """the handle over the story of e: every datagram, export_prompts, speaking and env after every tick; head, tick and dropped at the
    end.  also(cb) -> anything, collected after every tick as well -> (that per tick, at_end)"""
    pk, recv, m = e["pk"], e["recv"], e["model"]
    cb, seen = bridge(G, slots, None, K), []
    e["setup"](cb)
    got = run(cb, pk, recv, mode, before=e["before"], after=lambda t, c: seen.append((c.export_legs(), c.export_prompts(), also(c) if also else None)))
    end = (cb.export_legs(), cb.export_sequence(), cb.export_conceal(), cb.export_gate())
    cb.close()
    for t in range(recv.shape[0]):
        prompts_equal(seen[t][1], m.rp.prompt_seen[t], ("tick", t))
        for name in ("speaking", "env"):
            assert np.array_equal(seen[t][0][name], e["legs"][t][name]), (name, "tick", t)
    assert np.array_equal(got, e["want"]), np.argwhere((got != e["want"]).any(2))[:6]
    for name in ("head", "tick", "dropped"):
        assert np.array_equal(end[0][name], e["legs"][-1][name]), name
    return [s[2] for s in seen], end


@pytest.mark.parametrize("slots,mode", MODES)
def test_the_story_that_runs_at_once(cuda, oracle_port, slots, mode):
    e = expected(oracle_port, "main", main_story)
    handle_equals_replay(e, slots, mode)
    assert e["model"].rp.prompt_calls > 150 and e["model"].export_prompts()["done"].tolist() == [0, 0, 1, 1, 0, 2, 1, 1, 0, 0]


@pytest.mark.parametrize("slots,mode", MODES)
def test_a_ring_receives_the_legs_first_and_its_prompt_last(cuda, oracle_port, slots, mode):
    e = expected(oracle_port, "order", order_story)
    pk, recv, setup, before = order_story()
    other = replay_prompt_story(oracle_port, G, K, pk, recv, setup, before, prompt_first=True)[0]
    # the guard, in front of anything the handle does: the inputs saturate, so the other order sends leg 4 other datagrams
    assert not np.array_equal(other[:, 4], e["want"][:, 4])
    handle_equals_replay(e, slots, mode)


@pytest.mark.parametrize("slots,mode", MODES)
def test_prompts_pass_no_stage_and_no_stage_sees_them(cuda, oracle_port, slots, mode):
    """sequencing (with what it drops), concealment, the gate and speakers(2) on: what those stages export is what they export in the
    same story without prompts -- on the replay, and therefore on the handle"""
    pk, recv = stages_script()
    floor = floor_of(oracle_port, pk, recv)
    e = expected(oracle_port, "stages", lambda: (pk, recv) + stages_story(floor))
    if "stages_plain" not in REPLAYED:
        REPLAYED["stages_plain"] = replay_story(oracle_port, G, K, pk, recv, *stages_story(floor, prompts=False))
    plain_out, plain_legs, plain = REPLAYED["stages_plain"]
    gates, (legs, sq, concealed, gate) = handle_equals_replay(e, slots, mode, also=lambda c: c.export_gate())
    assert not np.array_equal(plain_out, e["want"])
    for t in range(T):
        for name in ("speaking", "env"):
            assert np.array_equal(e["legs"][t][name], plain_legs[t][name]), (name, t)
        for name in ("reduce", "voiced", "unvoiced"):
            assert np.array_equal(gates[t][name], plain.gate_seen[t][name]), (name, t)
    want = plain.export_sequence()
    for name in want:
        assert np.array_equal(sq[name], want[name]), (name, sq[name], want[name])
    assert sum(int(want[name].sum()) for name in ("late", "dup", "lost")) > 20
    assert np.array_equal(concealed, plain.export_conceal()) and concealed.sum() > 0
    for name in ("reduce", "voiced", "unvoiced"):
        assert np.array_equal(gate[name], plain.export_gate()[name]), name


@pytest.mark.parametrize("slots,mode", MODES)
def test_with_echo_control_the_prompt_is_in_the_far_row(cuda, oracle_port, slots, mode):
    e = expected(oracle_port, "echo", echo_story, base=ConfEchoReplay)
    m = e["model"]
    echoes, _ = handle_equals_replay(e, slots, mode, also=lambda c: c.export_echo())
    for t in range(T):
        for name in ECHO_FIELDS:
            assert echoes[t][name].dtype == m.echo_seen[t][name].dtype and np.array_equal(echoes[t][name], m.echo_seen[t][name]), (name, t)
    # leg 9 is in no conference: its far rows are its prompt and nothing else, and they are not silence
    assert any(far[9].any() for far in m.far_rows[10:])


def test_no_store_and_a_store_nobody_plays_from_are_the_plain_handle(cuda, oracle_port, wmx):
    pk, recv = arrivals(SEED, T_PLAIN, G)
    want, _, _ = replay_story(oracle_port, G, K, pk, recv, plain_setup)
    idle = {"clip": np.full(G, -1, np.int32), "pos": np.zeros(G, np.uint32), "left": np.zeros(G, np.uint32), "done": np.zeros(G, np.uint32)}
    for made in (False, True):
        cb = bridge()
        if made:
            store(cb)
        else:  # no store: nothing to add to, nothing to play from, nothing to stop; the export says idle
            one = np.ones(4, np.int16)
            assert wmx.wmx_conf_add_clip(cb._h, one.ctypes.data, 4, None) == ESTATE
            assert wmx.wmx_conf_play(cb._h, None, 0, 0, 1, 0, None) == ESTATE and wmx.wmx_conf_stop(cb._h, None, 0, None) == ESTATE
        got = run(cb, pk, recv, "ahead")
        prompts_equal(cb.export_prompts(), idle, "made" if made else "no store")
        cb.reset_legs([3])  # with and without a store
        assert wmx.wmx_conf_export_prompts(cb._h, None, None, None, None, None) == 0  # any pointer may be NULL
        cb.close()
        assert np.array_equal(got, want)
    assert wmx.wmx_conf_prompts(None, 1, 1) == EINVAL and wmx.wmx_conf_play(None, None, 0, 0, 1, 0, None) == EINVAL


@pytest.mark.parametrize("slots,mode", MODES)
def test_prompts_that_start_after_every_other_has_ended(cuda, oracle_port, slots, mode):
    """between the prompts lie ticks in which no leg plays -- the handle launches nothing for them -- and the next play finds the ring's
    play head where those ticks left it; leg 9 waits through a gap while nobody else plays"""
    from conf_prompt_stories import ODD, ONE, TAIL

    def setup(c):
        plain_setup(c)
        store(c)
        c.play([3], ODD, 1, 0)

    before = {12: lambda c: c.play([3, 9], TAIL, 2, 5), 13: lambda c: c.stop([3]), 30: lambda c: c.play([0], ONE, 1, 0),
              31: lambda c: c.play(None, MUSIC, 1, 0), 36: lambda c: c.reset_legs(None)}
    e = expected(oracle_port, "again", lambda: arrivals(SEED, T_PLAIN, G) + (setup, before))
    handle_equals_replay(e, slots, mode)
    seen = e["model"].rp.prompt_seen
    playing = [int((s["clip"] >= 0).sum()) for s in seen]
    assert playing[1] == 1 and playing[2:12] == [0] * 10 and playing[13:20] == [1] * 7 and playing[20:31] == [0] * 11 and playing[31] == G and playing[33] == 0
    assert seen[35]["done"].tolist() == [2, 1, 1, 2, 1, 1, 1, 1, 1, 2] and not seen[36]["done"].any()


def test_what_is_refused_changes_nothing(cuda, oracle_port, wmx):
    """a second store, a clip of no samples, a full table, an arena too small, a bad leg, a bad clip, a negative repeat, a gap of 65 536:
    each leaves export_prompts as it was, and the ticks behind them send the replay's datagrams"""
    def setup(c):
        plain_setup(c)
        c.prompts(3, 1200)
        assert c.add_clip(clips()[LONG]) == 0 and c.add_clip(clips()[MUSIC][:100]) == 1
        c.play([2, 9], 0, 0, 1)
        c.play([5], 1, 2, 3)

    pk, recv = arrivals(SEED, T_PLAIN, G)
    e = expected(oracle_port, "refusals", lambda: (pk, recv, setup, None))
    cb, h = bridge(G, 3, None, K), None
    setup(cb)
    h, x = cb._h, np.ones(200, np.int16)
    idx = lambda *legs: np.array(legs, np.int32).ctypes.data  # noqa: E731
    clip = C.c_int(77)
    refusals = [("a second store", lambda: wmx.wmx_conf_prompts(h, 3, 1200), ESTATE),
                ("no samples", lambda: wmx.wmx_conf_add_clip(h, x.ctypes.data, 0, C.byref(clip)), EINVAL),
                ("the arena too small", lambda: wmx.wmx_conf_add_clip(h, x.ctypes.data, 101, C.byref(clip)), EINVAL),
                ("a bad leg", lambda: wmx.wmx_conf_play(h, idx(1, G), 2, 0, 1, 0, None), EINVAL),
                ("a negative leg", lambda: wmx.wmx_conf_stop(h, idx(2, -1), 2, None), EINVAL),
                ("a bad clip", lambda: wmx.wmx_conf_play(h, idx(2), 1, 2, 1, 0, None), EINVAL),
                ("a negative clip", lambda: wmx.wmx_conf_play(h, None, 0, -1, 1, 0, None), EINVAL),
                ("a negative repeat", lambda: wmx.wmx_conf_play(h, idx(2), 1, 1, -1, 0, None), EINVAL),
                ("a gap too long", lambda: wmx.wmx_conf_play(h, idx(2), 1, 1, 1, 65536, None), EINVAL)]
    got = run(cb, pk[:7], recv[:7], "ahead")
    was = cb.export_prompts()
    prompts_equal(was, e["model"].rp.prompt_seen[6], "tick 6")
    for what, call, rc in refusals:
        assert call() == rc, what
        prompts_equal(cb.export_prompts(), was, what)
    assert clip.value == 77
    # the table takes its third clip of exactly what the arena has left, and then is full
    assert wmx.wmx_conf_add_clip(h, x.ctypes.data, 100, C.byref(clip)) == 0 and clip.value == 2
    assert wmx.wmx_conf_add_clip(h, x.ctypes.data, 1, C.byref(clip)) == EINVAL and clip.value == 2
    prompts_equal(cb.export_prompts(), was, "a full table")
    rest = run(cb, pk[7:], recv[7:], "ahead")
    prompts_equal(cb.export_prompts(), e["model"].rp.prompt_seen[-1], "the end")
    cb.close()
    assert np.array_equal(np.concatenate([got, rest]), e["want"])


def test_a_clip_in_another_format_goes_through_the_converter(cuda):
    """add_clip(pcm, freq, channels) stores what the package's pcm_zoom makes of the clip: 2 x 16 000 -> 1 x 8000"""
    import torch
    from wmix_amd.mix import pcm_zoom
    rng = np.random.default_rng(5)
    stereo = rng.integers(-8000, 8000, size=2 * 640).astype(np.int16)
    mono = pcm_zoom(2, 16000, torch.from_numpy(stereo).cuda().reshape(1, -1), 1, 8000)[0].cpu().numpy()
    assert 300 <= mono.size <= 340
    pk, recv = np.full((12, 2, 1, 172), 0xEE, np.uint8), np.zeros((12, 2, 1), np.int32)
    outs = []
    for given in ((stereo, 16000, 2), (mono, 8000, 1)):
        cb = bridge(2, 3, [[0, 1]], 1)
        cb.prompts(1, 400)
        cb.play([1], cb.add_clip(*given), 1, 0)
        outs.append(run(cb, pk, recv, "wait"))
        assert cb.export_prompts()["done"].tolist() == [0, 1]
        cb.close()
    assert np.array_equal(outs[0], outs[1]) and len(np.unique(outs[0][10, 1, 12:])) > 20
