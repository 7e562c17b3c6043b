"""wmx_conf_play_duck / wmx_conf_export_duck (wmix_amd/csrc/conf.hip; duck_fold_kernel and the ducking form of the legs' load in
mix.hip) through the Python mirror: the conference ducked under a leg's prompt, datagram for datagram against
tests/conf_duck_replay.py -- the reference's orc_load_data on one ring per leg whose reduce_mode the replay holds as the reference's
play task holds wmix->reduceMode.  The stories are those of tests/conf_duck_replay.py (tests/test_conf_duck_replay.py holds them
against what they are for, on the CPU): once on the plain handle, once beside sequencing, concealment, denoise, echo control, level and
the gate.  Every datagram of every tick, export_prompts and export_duck after every tick, in the three modes of tests/conf_harness.py.
Bytes and integers, np.array_equal."""
import numpy as np
import pytest

from conf_duck_replay import plain_duck_story, replay_duck_story, stages_duck_story
from conf_echo_replay import ECHO_FIELDS, ConfEchoReplay
from conf_harness import MODES, bridge, run
from conf_inputs import EINVAL, G, K, T
from conf_replay_model import ConfReplay

pytestmark = pytest.mark.gpu

REPLAYED = {}
PROMPT_FIELDS = ("clip", "pos", "left", "done")
STORIES = {"plain": (plain_duck_story, ConfReplay), "stages": (stages_duck_story, ConfEchoReplay)}


def expected(lib, name, **wrong):
    """the story and its replay, made once in a session; wrong: one of the two controls of tests/conf_duck_replay.py"""
    key = (name,) + tuple(sorted(wrong))
    if key not in REPLAYED:
        story, base = STORIES[name]
        pk, recv, setup, before = story()
        want, legs, m = replay_duck_story(lib, G, K, pk, recv, setup, before, base=base, **wrong)
        REPLAYED[key] = {"pk": pk, "recv": recv, "setup": setup, "before": before, "want": want, "legs": legs, "model": m}
    return REPLAYED[key]


def handle_over(e, slots, mode, also=None):
    """the handle over the story of e -> (datagrams, (export_prompts, export_duck, also(cb)) after every tick, export_legs at the end)"""
    cb, seen = bridge(G, slots, None, K), []
    e["setup"](cb)
    got = run(cb, e["pk"], e["recv"], mode, before=e["before"],
              after=lambda t, c: seen.append((c.export_prompts(), c.export_duck(), also(c) if also else None)))
    end = cb.export_legs()
    cb.close()
    return got, seen, end


@pytest.mark.parametrize("slots,mode", MODES)
@pytest.mark.parametrize("name", sorted(STORIES))
def test_the_handle_equals_the_replay_datagram_for_datagram(cuda, oracle_port, name, slots, mode):
    e = expected(oracle_port, name)
    m = e["model"]
    got, seen, end = handle_over(e, slots, mode, also=(lambda c: c.export_echo()) if name == "stages" else None)
    for t in range(T):
        for field in PROMPT_FIELDS:
            assert np.array_equal(seen[t][0][field], m.rp.prompt_seen[t][field]), (field, "tick", t)
        assert seen[t][1].dtype == np.uint8 and np.array_equal(seen[t][1], m.rp.duck_seen[t]), ("export_duck, tick", t, seen[t][1], m.rp.duck_seen[t])
        if name == "stages":  # what a ducked leg was sent is its far row: the canceller's state says so
            for field in ECHO_FIELDS:
                assert np.array_equal(seen[t][2][field], m.echo_seen[t][field]), (field, "tick", t)
    assert np.array_equal(got, e["want"]), np.argwhere((got != e["want"]).any(2))[:6]
    for field in ("head", "tick", "dropped"):
        assert np.array_equal(end[field], e["legs"][-1][field]), field
    assert m.rp.ducked_calls > 80
    # the controls: a handle that kept ducking through the gap, or divided the prompt too, would have sent other datagrams
    for wrong in ({"keep_in_gap": True}, {"divide_prompt": True}):
        other = expected(oracle_port, name, **wrong)["want"]
        assert not np.array_equal(other, e["want"]) and not np.array_equal(other, got), wrong


def test_what_play_duck_refuses_changes_nothing(cuda, oracle_port, wmx):
    """reduce 16 and reduce -1, on the handle; what wmx_conf_play refuses is refused here as well; the ticks behind the refusals send
    the replay's datagrams"""
    e = expected(oracle_port, "plain")
    cb = bridge(G, 3, None, K)
    e["setup"](cb)
    got = run(cb, e["pk"][:5], e["recv"][:5], "ahead")
    was, duck = cb.export_prompts(), cb.export_duck()
    idx = np.array([1, 5], np.int32)
    for what, rc in (("reduce 16", wmx.wmx_conf_play_duck(cb._h, idx.ctypes.data, 2, 0, 1, 0, 16, None)),
                     ("reduce -1", wmx.wmx_conf_play_duck(cb._h, idx.ctypes.data, 2, 0, 1, 0, -1, None)),
                     ("a bad clip", wmx.wmx_conf_play_duck(cb._h, idx.ctypes.data, 2, 99, 1, 0, 3, None)),
                     ("a bad leg", wmx.wmx_conf_play_duck(cb._h, np.array([1, G], np.int32).ctypes.data, 2, 0, 1, 0, 3, None)),
                     ("no handle", wmx.wmx_conf_play_duck(None, None, 0, 0, 1, 0, 3, None)),
                     ("no array", wmx.wmx_conf_export_duck(cb._h, None, None))):
        assert rc == EINVAL, what
        now = cb.export_prompts()
        assert all(np.array_equal(now[f], was[f]) for f in PROMPT_FIELDS) and np.array_equal(cb.export_duck(), duck), what
    rest = run(cb, e["pk"][5:], e["recv"][5:], "ahead", before={t - 5: f for t, f in e["before"].items()})
    cb.close()
    assert np.array_equal(np.concatenate([got, rest]), e["want"])


def test_a_handle_without_a_store_ducks_nothing(cuda, wmx):
    cb = bridge()
    assert cb.export_duck().tolist() == [1] * G
    assert wmx.wmx_conf_play_duck(cb._h, None, 0, 0, 1, 0, 3, None) == -10003  # WMX_ESTATE: no store
    cb.close()
