"""examples/host_conf.c --prompt LEN,EVERY,REPEAT,GAP,REDUCE: the C example with an announcement that ducks the conference
(wmx_conf_play_duck, wmx_conf_export_duck), in the manner of tests/test_host_conf_prompts_gpu.py.  The datagrams it sends are those of
the replay of tests/conf_duck_replay.py over the same script with the same clip, and those of the Python handle; with four fields it
sends what it sent before there was a fifth.  Bytes, np.array_equal."""
import numpy as np
import pytest

from conf_duck_replay import replay_duck_story
from conf_harness import host_conf, run
from conf_inputs import G, K, LAYOUT, SEED, T, Lcg, arrivals, fnv1a
from conf_prompt_replay import replay_prompt_story

pytestmark = pytest.mark.gpu

LEN, EVERY, REPEAT, GAP, REDUCE = 477, 3, 0, 2, 3
LEGS = [g for g in range(G) if g % EVERY == EVERY - 1]


def the_clip():
    """the example's clip: a second LCG seeded with the seed + 1, (next & 16383) - 8192 per sample"""
    rnd = Lcg(SEED + 1)
    return np.array([(rnd.next() & 16383) - 8192 for _ in range(LEN)], np.int16)


def story(reduce):
    def setup(c):
        c.set_conferences(LAYOUT)
        c.prompts(1, LEN)
        clip = c.add_clip(the_clip())
        if reduce is None:
            c.play(LEGS, clip, REPEAT, GAP)
        else:
            c.play(LEGS, clip, REPEAT, GAP, reduce=reduce)
    return setup


def test_host_conf_with_a_reduce_sends_what_the_replay_and_the_python_handle_send(tmp_path, cuda, oracle_port):
    from wmix_amd.conf import ConfBridge
    info, got = host_conf(tmp_path, "--prompt", "%d,%d,%d,%d,%d" % (LEN, EVERY, REPEAT, GAP, REDUCE))
    four, plain = host_conf(tmp_path, "--prompt", "%d,%d,%d,%d" % (LEN, EVERY, REPEAT, GAP))
    assert info["rc"] == 0 and info["prompt"] == LEN and info["prompt_legs"] == len(LEGS) == 3 and info["prompt_reduce"] == REDUCE
    assert not {"prompt_reduce", "prompt_ducking"} & set(four)
    pk, recv = arrivals(SEED, T, G)
    # four fields: what the example sent before there was a fifth -- the prompt replay -- and a fifth of 0 sends the same
    want_plain, _, _ = replay_prompt_story(oracle_port, G, K, pk, recv, story(None))
    zero, same = host_conf(tmp_path, "--prompt", "%d,%d,%d,%d,0" % (LEN, EVERY, REPEAT, GAP))
    assert np.array_equal(plain, want_plain) and four["datagrams_fnv1a"] == fnv1a(want_plain)
    assert np.array_equal(same, plain) and zero["prompt_reduce"] == 0 and zero["prompt_ducking"] == 0
    # the fifth: the legs that play are sent the rest of their conference divided by REDUCE + 1; nobody else notices
    want, _, m = replay_duck_story(oracle_port, G, K, pk, recv, story(REDUCE))
    assert [g for g in range(G) if not np.array_equal(want[:, g], want_plain[:, g])] == [2, 5, 8]
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    cb = ConfBridge(G, 3, K)
    story(REDUCE)(cb)
    sent = run(cb, pk, recv, "ahead")
    duck = cb.export_duck()
    cb.close()
    assert np.array_equal(sent, want) and info["datagrams_fnv1a"] == fnv1a(want)
    assert np.array_equal(duck, m.export_duck()) and info["prompt_ducking"] == int((duck > 1).sum())
    assert m.rp.ducked_calls > 60


def test_host_conf_refuses_the_reduce_the_library_refuses(tmp_path, cuda):
    import os
    import subprocess

    import conftest
    exe = os.path.join(conftest.ROOT, "examples", "host_conf")
    base = [exe, str(tmp_path / "o.rtp"), str(G), "4", "--sizes", "2,3,4", "--seed", str(SEED)]
    r = subprocess.run(base + ["--prompt", "100,3,1,0,16"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 4 and "reduce" in r.stderr
