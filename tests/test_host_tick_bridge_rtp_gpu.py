"""examples/host_tick.c --bridge-rtp: a conference bridge of RTP/G.711 legs from plain C -- wmx_rtp_ingest_legs, wmx_mix_load_minus_legs
on the tick's mixer, wmx_tick_play, wmx_rtp_egress per 20 ms -- run once at a small size.  The datagrams it sends are compared with a
Python replay built from the oracle's ingest, one reference ring per leg with a cursor per source leg, the drain and the oracle's
egress, fed by the same scripted arrivals.  Bytes, np.array_equal."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import conftest
from oracle import loader as L
from test_bridge_legs_gpu import LegsOracle

pytestmark = pytest.mark.gpu

MASK = (1 << 64) - 1


class Lcg:
    def __init__(self, seed):
        self.s = seed

    def next(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & MASK
        return self.s >> 33


def arrivals(seed, T, G):
    """the example's script (examples/host_tick.c, bridge_rtp): datagram rows [T, G, 3, 172] and what recvfrom returned [T, G, 3]"""
    rnd = Lcg(seed)
    pk = np.full((T, G, 3, 172), 0xEE, np.uint8)
    recv = np.zeros((T, G, 3), np.int32)
    seq = [0] * G
    for t in range(T):
        for g in range(G):
            u = rnd.next() % 8
            recv[t, g] = [172 if u >= 2 else 0, 172 if u == 2 else (-1 if u == 3 else 0), 172 if u == 3 else 0]
            for k in range(3):
                if recv[t, g, k] <= 0:
                    continue
                v = rnd.next() % 16
                pk[t, g, k, :12] = 0
                pk[t, g, k, 0] = 0x80
                pk[t, g, k, 1] = 0x80 | (96 if v == 0 else (0 if v == 1 else 8))
                pk[t, g, k, 2], pk[t, g, k, 3] = (seq[g] >> 8) & 255, seq[g] & 255
                seq[g] = (seq[g] + 1) & 0xFFFF
                pk[t, g, k, 12:] = [rnd.next() & 255 for _ in range(160)]
    return pk, recv


def replay(lib, pk, recv, layout, platform):
    T, G = recv.shape[:2]
    ing = L._fn(lib, "orc_rtp_ingest", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    eg = L._fn(lib, "orc_rtp_egress", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p])
    senders = [(C.c_uint8 * 16)() for _ in range(G)]
    for s in senders:
        L._fn(lib, "orc_rtp_sender_init", None, [C.c_void_p, C.c_int])(s, 0)
    orc = LegsOracle(lib, G, (1, 8000), 1, L.PLATFORMS[platform][1])
    out = np.zeros((T, G, 172), np.uint8)
    calls = 0
    for t in range(T):
        pcm, lens = np.zeros((G, 3, 161), np.int16), np.zeros((G, 3), np.uint32)
        for g in range(G):
            for k in range(3):
                if recv[t, g, k] > 0:
                    row, dec = np.ascontiguousarray(pk[t, g, k]), np.zeros(160, np.int16)
                    lens[g, k] = ing(row.ctypes.data, dec.ctypes.data, None)
                    pcm[g, k, :160] = dec
        calls += int((lens == 320).sum())
        orc.load(layout, pcm, lens, 320, 8000, 1, 160, None)
        play = orc.drain()
        for g in range(G):
            row = np.ascontiguousarray(play[g])
            assert eg(senders[g], 1, 8000, row.ctypes.data, 320, 1, 8000, out[t, g].ctypes.data) == 172
    return out, calls


def fnv1a(data):
    h = 1469598103934665603
    for b in data.tobytes():
        h = ((h ^ b) * 1099511628211) & MASK
    return "%016x" % h


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
