"""examples/host_conf.c --prompt LEN,EVERY[,REPEAT[,GAP]]: the C example with an announcement played to every third leg from tick 0
(wmx_conf_prompts, wmx_conf_add_clip, wmx_conf_play), at the sizes tests/test_host_conf_gpu.py runs it.  The datagrams it sends are
those of the replay of tests/conf_prompt_replay.py over the same script with the same clip, and those of the Python handle.  Bytes,
np.array_equal."""
import numpy as np
import pytest

from conf_harness import host_conf, run
from conf_inputs import G, K, LAYOUT, SEED, T, Lcg, arrivals, fnv1a
from conf_prompt_replay import replay_prompt_story

pytestmark = pytest.mark.gpu

LEN, EVERY, REPEAT, GAP = 477, 3, 2, 1
LEGS = [g for g in range(G) if g % EVERY == EVERY - 1]


def the_clip():
    """the example's clip: a second LCG seeded with the seed + 1, (next & 16383) - 8192 per sample"""
    rnd = Lcg(SEED + 1)
    return np.array([(rnd.next() & 16383) - 8192 for _ in range(LEN)], np.int16)


def test_host_conf_prompt_sends_what_the_replay_and_the_python_handle_send(tmp_path, cuda, oracle_port):
    from wmix_amd.conf import ConfBridge
    info, got = host_conf(tmp_path, "--prompt", "%d,%d,%d,%d" % (LEN, EVERY, REPEAT, GAP))
    plain, other = host_conf(tmp_path)
    assert info["rc"] == 0 and info["prompt"] == LEN and info["prompt_legs"] == len(LEGS) == 3 and not np.array_equal(got, other)
    assert not {"prompt", "prompt_legs", "prompt_done"} & set(plain)
    # the legs that play nothing are sent what they are sent without the flag: the network's script is the same
    quiet = [g for g in range(G) if g not in LEGS]
    assert np.array_equal(got[:, quiet], other[:, quiet])
    pk, recv = arrivals(SEED, T, G)

    def setup(c):
        c.set_conferences(LAYOUT)
        c.prompts(1, LEN)
        c.play(LEGS, c.add_clip(the_clip()), REPEAT, GAP)

    want, _, m = replay_prompt_story(oracle_port, G, K, pk, recv, setup)
    cb = ConfBridge(G, 3, K)
    setup(cb)
    sent = run(cb, pk, recv, "ahead")
    done = cb.export_prompts()["done"]
    cb.close()
    assert info["datagrams_in"] == int((recv > 0).sum())
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    assert np.array_equal(sent, want) and info["datagrams_fnv1a"] == fnv1a(want)
    assert info["prompt_done"] == int(done.sum()) == int(m.export_prompts()["done"].sum()) == len(LEGS)
    assert m.rp.prompt_calls == len(LEGS) * REPEAT * 3  # 477 samples: two whole ticks and a tail of 157


def test_host_conf_refuses_what_the_library_refuses(tmp_path, cuda):
    import os
    import subprocess

    import conftest
    exe = os.path.join(conftest.ROOT, "examples", "host_conf")
    base = [exe, str(tmp_path / "o.rtp"), str(G), "4", "--sizes", "2,3,4", "--seed", str(SEED)]
    r = subprocess.run(base + ["--prompt", "100,3,1,65536"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 4 and "gap_ticks" in r.stderr
    assert subprocess.run(base + ["--prompt", "0,3"], capture_output=True, text=True, timeout=60).returncode == 2
