"""examples/host_conf.c --ulaw-every N: the conference bridge from plain C with every N-th leg on PCMU, both ways, run once at a small
size.  The datagrams it sends are those of the replay with a codec per leg (CodecReplay, tests/leg_oracle_model.py) for the same
scripted arrivals (ulaw_every_script, tests/conf_inputs.py), and its refused count is the replay's.  Bytes, np.array_equal."""
import os
import subprocess

import numpy as np
import pytest

import conftest
from conf_harness import host_conf
from conf_inputs import EVERY, G, K, LAYOUT, SEED, T, ULAW, arrivals, fnv1a, ulaw_every_script
from conf_single_replays import replay
from leg_codec_model import LAW_U, PCMU
from leg_oracle_model import CodecReplay

pytestmark = pytest.mark.gpu


def test_host_conf_with_ulaw_legs_sends_what_the_replay_sends(tmp_path, oracle_port):
    info, got = host_conf(tmp_path, "--slots", "3", "--ulaw-every", str(EVERY))
    pk, recv = ulaw_every_script()
    rp, want = CodecReplay(oracle_port, G), np.zeros((T, G, 172), np.uint8)
    rp.set_codecs(ULAW, PCMU, LAW_U)
    for t in range(T):
        want[t] = rp.tick(*rp.decode(pk[t], recv[t]), LAYOUT)
    assert ULAW == [2, 5, 8] and K == 3
    assert info["rc"] == 0 and info["ulaw_every"] == EVERY and info["ulaw_legs"] == len(ULAW) and info["dropped"] == 0
    assert info["datagrams_in"] == int((recv > 0).sum())
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    assert info["datagrams_fnv1a"] == fnv1a(want)
    assert info["refused"] == int(rp.refused.sum()) > 0
    assert (got[:, ULAW, 1] == 0x80).all() and (got[:, [g for g in range(G) if g not in ULAW], 1] == 0x88).all()
    # without the flag the same legs are decoded as A-law and answered in A-law: other bytes for everybody who hears them
    plain, _ = replay(oracle_port, *arrivals(SEED, T, G), LAYOUT, "alsa")
    assert not np.array_equal(want[:, 3, 12:], plain[:, 3, 12:])


def test_host_conf_ulaw_every_0_exits_2(tmp_path):
    exe = os.path.join(conftest.ROOT, "examples", "host_conf")
    bad = subprocess.run([exe, str(tmp_path / "out.rtp"), str(G), str(T), "--sizes", "2,3,4", "--seed", "1", "--ulaw-every", "0"], capture_output=True,
                         text=True, timeout=60)
    assert bad.returncode == 2 and "--ulaw-every" in bad.stderr
