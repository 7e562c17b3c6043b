"""examples/host_tick.c --bridge-rtp: a conference bridge of RTP/G.711 legs from plain C -- wmx_rtp_ingest_legs, wmx_mix_load_minus_legs
on the tick's mixer, wmx_tick_play, wmx_rtp_egress per 20 ms -- run once at a small size.  The datagrams it sends are compared with the
whole-script replay of tests/conf_single_replays.py -- the oracle's ingest, one reference ring per leg with a cursor per source leg, the
drain and the oracle's egress -- fed by the same scripted arrivals (arrivals() of tests/conf_inputs.py).  Bytes, np.array_equal."""
import json
import os
import subprocess

import numpy as np
import pytest

import conftest
from conf_inputs import arrivals, fnv1a
from conf_single_replays import replay

pytestmark = pytest.mark.gpu


def test_host_tick_bridge_rtp_sends_what_the_replay_sends(tmp_path, oracle_port):
    exe = os.path.join(conftest.ROOT, "examples", "host_tick")
    assert os.path.exists(exe), "examples/host_tick missing: run __graft_entry__.build()"
    T, G, seed = 40, 10, 20260
    layout = [[0, 1], [2, 3, 4], [5, 6, 7, 8]]  # leg 9 is in no conference
    cmd = [exe, "-", "-", str(tmp_path / "out.rtp"), str(G), "1", "1", str(T), "8000", "1", "--bridge-sizes", "2,3,4", "--bridge-rtp", str(seed)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    pk, recv = arrivals(seed, T, G)
    want, calls = replay(oracle_port, pk, recv, layout, "alsa")
    got = np.fromfile(tmp_path / "out.rtp", dtype=np.uint8).reshape(T, G, 172)
    assert info["rc"] == 0 and info["bridge_sizes"] == [2, 3, 4] and info["dropped"] == 0 and info["datagrams_in"] == int((recv > 0).sum())
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    assert info["datagrams_fnv1a"] == fnv1a(want)
    # the script reached what it is for: empty ticks, bursts, a hole in a burst, a foreign payload type; every leg in a conference is
    # played something and the idle one silence (A-law of 0 is 0xD5)
    assert (recv[:, :, 0] <= 0).any() and (recv[:, :, 1] > 0).any() and (recv[:, :, 1] < 0).any() and calls < int((recv > 0).sum())
    assert all((got[:, g, 12:] != 0xD5).any() for g in range(9)) and (got[:, 9, 12:] == 0xD5).all()
    # refused: without --bridge-sizes
    bad = subprocess.run(cmd[:10] + ["--bridge-rtp", "1"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--bridge-sizes" in bad.stderr
