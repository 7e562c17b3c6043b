"""examples/host_conf.c: a conference bridge of RTP/G.711 legs from plain C over wmx_conf_* alone, run once at a small size.  The datagrams
it sends are those of the whole-script replay (tests/conf_single_replays.py) for the same scripted arrivals (tests/conf_inputs.py); with
talker selection they are what the Python handle sends for the same script (run() of tests/conf_harness.py).  Bytes, np.array_equal."""
import os
import subprocess

import numpy as np
import pytest

import conftest
from conf_harness import host_conf, run
from conf_inputs import G, K, LAYOUT, SEED, T, arrivals, fnv1a
from conf_single_replays import replay

pytestmark = pytest.mark.gpu


def test_host_conf_sends_what_the_replay_sends(tmp_path, oracle_port):
    info, got = host_conf(tmp_path, "--slots", "3")
    pk, recv = arrivals(SEED, T, G)
    want, _ = replay(oracle_port, pk, recv, LAYOUT, "alsa")
    assert info["rc"] == 0 and info["bridge_sizes"] == [2, 3, 4] and info["slots"] == 3 and info["dropped"] == 0
    assert info["datagrams_in"] == int((recv > 0).sum()) and info["groups"] == G and info["ticks"] == T
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    assert info["datagrams_fnv1a"] == fnv1a(want)


def test_host_conf_with_talker_selection_sends_what_the_python_handle_sends(tmp_path, cuda):
    from wmix_amd.conf import ConfBridge
    floor = 950000  # between the levels of this script's packets (600 000 .. 1 270 000)
    info, got = host_conf(tmp_path, "--speakers", "2,%d,3" % floor)
    pk, recv = arrivals(SEED, T, G)
    cb = ConfBridge(G, 3, K)
    cb.set_conferences(LAYOUT)
    cb.speakers(2, floor, 3)
    want = run(cb, pk, recv, "ahead")
    cb.close()
    cb = ConfBridge(G, 3, K)
    cb.set_conferences(LAYOUT)
    plain = run(cb, pk, recv, "ahead")
    cb.close()
    assert info["rc"] == 0 and info["speakers"] == 2
    assert np.array_equal(got, want) and not np.array_equal(want, plain)


def test_host_conf_without_sizes_exits_2(tmp_path):
    exe = os.path.join(conftest.ROOT, "examples", "host_conf")
    bad = subprocess.run([exe, str(tmp_path / "out.rtp"), str(G), str(T), "--seed", "1"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--sizes" in bad.stderr
