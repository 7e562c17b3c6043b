"""The conference handle (wmix_amd/conf.py) and the C example (examples/host_conf.c) as the tests run them, and the one comparison of
a handle with its composed replay.

The rule of the family -- tests/conf_replay_model.py, every leg_*_model.py (leg_rows_model.py holds the row walk they share),
leg_stage_inputs.py, leg_gate_inputs.py, legs_kernel_harness.py, conf_inputs.py, conf_stories.py, conf_single_replays.py, this module,
and the test modules of the conference handle and of the stages' kernels -- is that none of them imports a module named test_*.  A new stage is one
setter and one line in ConfReplay.tick, one story in conf_stories.py, and one test module that imports support modules only."""
import json
import os
import subprocess
import time

import numpy as np

import conftest
from conf_inputs import G, K, LAYOUT, SEED, T
from conf_replay_model import replay_story
from leg_seq_model import COUNTERS

MODES = [(1, "wait"), (3, "ahead"), (3, "resident")]


def bridge(n=G, slots=3, layout=LAYOUT, max_packets=K):
    from wmix_amd.conf import ConfBridge
    cb = ConfBridge(n, slots, max_packets)
    if layout is not None:
        cb.set_conferences(layout)
    return cb


def run(cb, pk, recv, mode, before=None, after=None):
    """the handle over the script.  mode "wait": submit and wait, tick by tick; "ahead": the rows of tick t + 1 are written and submitted
    before tick t is waited for; "poll": as "ahead", but a tick is collected by asking cb.poll(slot) until it says yes (5 s at the most),
    never by waiting; "resident": wmx_conf_step_resident on rows that are on the device.  before[t](cb) runs in front of tick t's submit,
    after(t, cb) behind it."""
    import torch
    n_t, n = recv.shape[:2]
    out, queued = np.zeros((n_t, n, 172), np.uint8), []

    def collect(depth):
        while len(queued) > depth:
            t0, k0 = queued.pop(0)
            if mode == "poll":
                deadline = time.monotonic() + 5.0
                while not cb.poll(k0):
                    assert time.monotonic() < deadline, "tick %d has not landed in 5 s" % t0
            else:
                cb.wait(k0)
            out[t0] = cb.rows_out[k0]

    for t in range(n_t):
        if before and t in before:
            before[t](cb)
        if mode == "resident":
            rows = np.zeros((n, recv.shape[2], cb.in_row), np.uint8)
            rows[:, :, :172] = pk[t]
            out[t] = cb.step_resident(torch.from_numpy(rows).cuda(), torch.from_numpy(recv[t]).cuda()).cpu().numpy()
        else:
            k = cb.next_slot()
            cb.rows_in[k][:, :, :172] = pk[t]
            cb.recv[k][:] = recv[t]
            assert cb.submit() == k
            queued.append((t, k))
            collect(1 if mode in ("ahead", "poll") else 0)
        if after:
            after(t, cb)
    collect(0)
    return out


def handle(n, slots, pk, recv, setup, before, mode, at_end=None):
    """a fresh handle over a story -> (datagrams, export_legs() after every tick, at_end(cb) in front of its close)"""
    cb, seen = bridge(n, slots, None, recv.shape[2]), []
    setup(cb)
    got = run(cb, pk, recv, mode, before=before, after=lambda t, c: seen.append(c.export_legs()))
    end = at_end(cb) if at_end else None
    cb.close()
    return got, seen, end


def counters_equal(cb, model):
    """every field the sequence model exports, against the handle's"""
    got, want = cb.export_sequence(), model.export()
    for name in want:
        assert np.array_equal(got[name], want[name]), (name, got[name], want[name])


def host_conf(tmp_path, *extra):
    """examples/host_conf at the family's shape -> (the JSON line it prints, the datagrams it sent [T, G, 172])"""
    exe = os.path.join(conftest.ROOT, "examples", "host_conf")
    assert os.path.exists(exe), "examples/host_conf missing: run __graft_entry__.build()"
    out = tmp_path / "out.rtp"
    r = subprocess.run([exe, str(out), str(G), str(T), "--sizes", "2,3,4", "--seed", str(SEED)] + list(extra), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1]), np.fromfile(out, dtype=np.uint8).reshape(T, G, 172)


REPLAYED = {}  # a story's replay, made once in a session and shared by the modes and the tests that run it


def expected(key, lib, n, max_packets, story):
    """story() -> (pk, recv, setup, before); -> the story and its composed replay: the datagrams `want`, export_legs() after every tick
    `legs`, and the model as the last tick left it"""
    if key not in REPLAYED:
        pk, recv, setup, before = story()
        want, legs, m = replay_story(lib, n, max_packets, pk, recv, setup, before)
        REPLAYED[key] = {"pk": pk, "recv": recv, "setup": setup, "before": before, "want": want, "legs": legs, "model": m}
    return REPLAYED[key]


def handle_equals_replay(e, slots, mode):
    """the handle over the story of e = expected(...) against the replay: every datagram of every tick; speaking and env after every
    tick; head, tick and dropped at the end, every field of export_sequence, export_conceal, the three fields of export_codecs and the
    three of export_gate (before the first gate(True) both sides say reduce 4, counts 0).
    -> e, for what the caller asserts of the model"""
    pk, recv, m = e["pk"], e["recv"], e["model"]
    exports = lambda cb: (cb.export_legs(), cb.export_sequence(), cb.export_conceal(), cb.export_codecs(), cb.export_gate())  # noqa: E731
    got, seen, (end, sq, concealed, codecs, gate) = handle(recv.shape[1], slots, pk, recv, e["setup"], e["before"], mode, exports)
    for t in range(recv.shape[0]):
        for name in ("speaking", "env"):
            assert np.array_equal(seen[t][name], e["legs"][t][name]), (name, "tick", t, seen[t][name], e["legs"][t][name])
    assert np.array_equal(got, e["want"]), np.argwhere((got != e["want"]).any(2))[:6]
    for name in ("head", "tick", "dropped"):
        assert np.array_equal(end[name], e["legs"][-1][name]), (name, end[name], e["legs"][-1][name])
    want = m.export_sequence()
    assert sorted(want) == sorted(COUNTERS + ("next", "synced"))
    for name in want:
        assert np.array_equal(sq[name], want[name]), (name, sq[name], want[name])
    assert np.array_equal(concealed, m.export_conceal()), (concealed, m.export_conceal())
    want = m.export_codecs()
    for name in ("in_codec", "out_law", "refused"):
        assert np.array_equal(codecs[name], want[name]), (name, codecs[name], want[name])
    want = m.export_gate()
    for name in ("reduce", "voiced", "unvoiced"):
        assert gate[name].dtype == want[name].dtype and np.array_equal(gate[name], want[name]), (name, gate[name], want[name])
    return e
