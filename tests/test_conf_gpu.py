"""wmx_conf (wmix_amd/csrc/conf.hip) through the Python mirror: a conference bridge of RTP/G.711 legs in one handle, datagram in, datagram
out.  Every datagram of every tick is compared with the replay of tests/test_host_tick_bridge_rtp_gpu.py -- the oracle's ingest, one
reference ring per leg with a cursor per source leg (LegsOracle), the drain and the oracle's egress, fed by the same scripted arrivals --
which is wrapped here so that the layout, the mute and the calls can change between ticks.  Bytes, np.array_equal."""
import ctypes as C
import time

import numpy as np
import pytest

from oracle import loader as L
from speakers_legs_model import SpeakersLegsModel
from test_bridge_gpu import EINVAL, NULL_HEAD
from test_bridge_legs_gpu import LegsOracle
from test_host_tick_bridge_rtp_gpu import arrivals, replay

pytestmark = pytest.mark.gpu

LAYOUT = [[0, 1], [2, 3, 4], [5, 6, 7, 8]]  # leg 9 is in no conference
T, G, K, SEED = 40, 10, 3, 20260


class Replay:
    """replay() of tests/test_host_tick_bridge_rtp_gpu.py one tick at a time"""

    def __init__(self, lib, n, platform="alsa"):
        self.ing = L._fn(lib, "orc_rtp_ingest", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
        self.eg = L._fn(lib, "orc_rtp_egress", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p])
        self.init = L._fn(lib, "orc_rtp_sender_init", None, [C.c_void_p, C.c_int])
        self.senders = [(C.c_uint8 * 16)() for _ in range(n)]
        for s in self.senders:
            self.init(s, 0)
        self.orc, self.n = LegsOracle(lib, n, (1, 8000), 1, L.PLATFORMS[platform][1]), n

    def decode(self, pk, recv, slots=K):
        pcm, lens = np.zeros((self.n, slots, 161), np.int16), np.zeros((self.n, slots), np.uint32)
        for g in range(self.n):
            for k in range(slots):
                if recv[g, k] > 0:
                    row, dec = np.ascontiguousarray(pk[g, k]), np.zeros(160, np.int16)
                    lens[g, k] = self.ing(row.ctypes.data, dec.ctypes.data, None)
                    pcm[g, k, :160] = dec
        return pcm, lens

    def tick(self, pcm, lens, layout, mute=None):
        self.orc.load(layout, pcm, lens, 320, 8000, 1, 160, mute)
        play, out = self.orc.drain(), np.zeros((self.n, 172), np.uint8)
        for g in range(self.n):
            row = np.ascontiguousarray(play[g])
            assert self.eg(self.senders[g], 1, 8000, row.ctypes.data, 320, 1, 8000, out[g].ctypes.data) == 172
        return out

    def fresh(self, legs):
        """a new call in these legs' slots: the reference ring, the receive thread's cursor and the sender as a new task makes them"""
        self.orc.reset(legs)
        for g in legs:
            self.orc.rings.store[g][:] = 0
            self.init(self.senders[g], 0)


def replay_with(lib, pk, recv, layout_at, mute_at=None, fresh_at=None, select=None):
    """-> (datagrams [T, n, 172], per tick (speaking, env) when `select` = (max_speakers, floor, shift) is given)"""
    n = recv.shape[1]
    rp, model, out, sel = Replay(lib, n), SpeakersLegsModel(n), np.zeros((recv.shape[0], n, 172), np.uint8), []
    for t in range(recv.shape[0]):
        if fresh_at and t in fresh_at:
            rp.fresh(fresh_at[t])
            model.reset(fresh_at[t])
        pcm, lens = rp.decode(pk[t], recv[t])
        mute = mute_at(t) if mute_at else None
        if select:
            sp, mute = model.step_legs(layout_at(t), pcm, lens, 320, select[0], select[1], select[2], mute)
            sel.append((sp.copy(), model.env.copy()))
        out[t] = rp.tick(pcm, lens, layout_at(t), mute)
    return out, sel


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


@pytest.fixture(scope="module")
def script(oracle_port):
    pk, recv = arrivals(SEED, T, G)
    want, calls = replay(oracle_port, pk, recv, LAYOUT, "alsa")
    return pk, recv, want


def bridge(n=G, slots=3, layout=LAYOUT, max_packets=K):
    from wmix_amd.conf import ConfBridge
    cb = ConfBridge(n, slots, max_packets)
    if layout is not None:
        cb.set_conferences(layout)
    return cb


@pytest.mark.parametrize("slots,mode", [(1, "wait"), (3, "ahead"), (3, "resident"), (2, "poll")])
def test_every_datagram_is_the_replays(cuda, script, slots, mode):
    pk, recv, want = script
    cb = bridge(slots=slots)
    got = run(cb, pk, recv, mode)
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    st = cb.export_legs()
    assert not st["dropped"].any() and st["head"][9] == NULL_HEAD and (st["head"][:9] != NULL_HEAD).all()
    assert cb.sender_state(0) == (T, 160 * T) and cb.export_ring(0)[1:] == ((T * 320) % 16000, T * 320)
    assert all((got[:, g, 12:] != 0xD5).any() for g in range(9)) and (got[:, 9, 12:] == 0xD5).all()
    cb.close()


def test_the_tick_by_tick_replay_is_the_replay(oracle_port, script):
    pk, recv, want = script
    assert np.array_equal(replay_with(oracle_port, pk, recv, lambda t: LAYOUT)[0], want)


def test_a_conference_of_32_beside_one_of_2(cuda, oracle_port):
    n, ticks = 35, 12
    layout = [list(range(33, 1, -1)), [0, 34]]  # leg 1 idle
    pk, recv = arrivals(7, ticks, n)
    want, _ = replay(oracle_port, pk, recv, layout, "alsa")
    cb = bridge(n, 3, layout)
    got = run(cb, pk, recv, "ahead")
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    assert not cb.export_legs()["dropped"].any() and (got[:, 1, 12:] == 0xD5).all() and (got[:, 34, 12:] != 0xD5).any()
    cb.close()


def test_talker_selection(cuda, oracle_port, script):
    pk, recv, plain = script
    ticks = 30
    pk, recv = pk[:ticks], recv[:ticks]
    levels = []
    for t in range(ticks):
        pcm, lens = Replay(oracle_port, G).decode(pk[t], recv[t])
        levels += [int(np.abs(pcm[g, k].astype(np.int64)).sum()) for g in range(G) for k in range(K) if lens[g, k] == 320]
    floor = int(np.percentile(levels, 40))  # four packets in ten are below it
    want, sel = replay_with(oracle_port, pk, recv, lambda t: LAYOUT, select=(2, floor, 3))
    assert any(sp[LAYOUT[2]].sum() == 2 for sp, _ in sel) and any(sp[LAYOUT[2]].sum() < 2 for sp, _ in sel)
    assert not np.array_equal(want, plain[:ticks])
    seen = []
    cb = bridge()
    cb.speakers(2, floor, 3)
    got = run(cb, pk, recv, "ahead", after=lambda t, c: seen.append(c.export_legs()))
    for t in range(ticks):
        assert np.array_equal(seen[t]["speaking"], sel[t][0]) and np.array_equal(seen[t]["env"], sel[t][1]), ("speaking / env, tick", t)
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    cb.close()
    # everybody selected: the bytes of the run without selection
    cb = bridge()
    cb.speakers(32, 0, 3)
    got = run(cb, pk, recv, "ahead")
    assert np.array_equal(got, plain[:ticks])
    cb.close()


def test_the_hosts_mute_changes_mid_run(cuda, oracle_port, script):
    pk, recv, plain = script
    masks = {10: np.eye(G, dtype=np.uint8)[6], 22: np.eye(G, dtype=np.uint8)[3], 31: None}

    def mute_at(t):
        since = [s for s in masks if s <= t]
        return masks[max(since)] if since else None

    want, _ = replay_with(oracle_port, pk, recv, lambda t: LAYOUT, mute_at=mute_at)
    assert np.array_equal(want[:10], plain[:10]) and not np.array_equal(want[10:, 5], plain[10:, 5])
    cb = bridge()
    got = run(cb, pk, recv, "ahead", before={t: (lambda c, m=m: c.mute(m)) for t, m in masks.items()})
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    cb.close()


def test_a_new_call_in_a_used_slot(cuda, oracle_port, script):
    """At tick 15 leg 3 leaves and its slot is reset; at tick 20 it joins legs 0 and 1 as a new call.  Every leg, leg 3 included, equals
    the replay in which leg 3's reference ring, cursor and sender were made fresh at tick 15 -- on every tick.  The replay WITHOUT the
    reset is what every other leg equals up to tick 20 and the legs that do not hear leg 3 throughout (from tick 20 on legs 0 and 1
    hear leg 3 from where its cursor starts, and a fresh cursor starts elsewhere than the old one resumes); leg 3 itself differs from
    it: the old call's audio, loaded ahead, and the old sequence numbers are gone."""
    pk, recv, _ = script
    without3, joined = [[0, 1], [2, 4], [5, 6, 7, 8]], [[0, 1, 3], [2, 4], [5, 6, 7, 8]]
    layout_at = lambda t: LAYOUT if t < 15 else (without3 if t < 20 else joined)  # noqa: E731
    want, _ = replay_with(oracle_port, pk, recv, layout_at, fresh_at={15: [3]})
    stale, _ = replay_with(oracle_port, pk, recv, layout_at)
    cb = bridge()

    def leave(c):
        c.set_conferences(without3)
        c.reset_legs([3])

    got = run(cb, pk, recv, "ahead", before={15: leave, 20: lambda c: c.set_conferences(joined)})
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    others = [g for g in range(G) if g != 3]
    assert np.array_equal(got[:20, others], stale[:20, others]) and np.array_equal(got[:, [2, 4, 5, 6, 7, 8, 9]], stale[:, [2, 4, 5, 6, 7, 8, 9]])
    assert (got[15:20, 3, 12:] == 0xD5).all() and got[15, 3, 2:4].tolist() == [0, 0] and not np.array_equal(got[20:, 3], stale[20:, 3])
    assert (stale[15:20, 3, 12:] != 0xD5).any()  # without the reset the new call would have heard the old one's tail
    cb.close()


def test_refusals_take_no_slot_and_change_nothing(cuda, wmx, script):
    import torch
    pk, recv, _ = script
    stream = torch.cuda.current_stream().cuda_stream
    h = C.c_void_p()
    for n, slots, k, law in ((G, 0, K, 0), (G, 17, K, 0), (G, 3, 0, 0), (G, 3, 5, 0), (G, 3, K, 2), (0, 3, K, 0)):
        assert wmx.wmx_conf_create(C.byref(h), n, slots, k, law) == EINVAL and not h.value, (n, slots, k, law)
    cb = bridge(layout=None)
    slot = C.c_int(-1)
    assert wmx.wmx_conf_submit(cb._h, C.byref(slot), stream) == EINVAL and b"layout" in wmx.wmx_last_error() and slot.value == -1
    assert cb.next_slot() == 0
    cb.set_conferences(LAYOUT)
    run(cb, pk[:4], recv[:4], "wait")
    assert cb.poll(2) and cb.poll(-1)  # a slot that is not in flight, and every slot behind the run: at once
    assert wmx.wmx_conf_poll(cb._h, cb.slots) == EINVAL and wmx.wmx_conf_wait(cb._h, cb.slots) == EINVAL

    def state():
        return cb.next_slot(), cb.export_legs(), [cb.export_ring(g) for g in range(G)], [cb.sender_state(g) for g in range(G)]

    before = state()
    assert before[0] == 1 and before[1]["tick"][:9].any()
    bad = np.array([3, G], np.int32)
    assert wmx.wmx_conf_reset_legs(cb._h, bad.ctypes.data, 2, stream) == EINVAL
    assert wmx.wmx_conf_speakers(cb._h, 33, 0, 3) == EINVAL and wmx.wmx_conf_speakers(cb._h, 2, 0, 32) == EINVAL
    assert wmx.wmx_conf_step_resident(cb._h, None, None, None, stream) == EINVAL
    cb.set_conferences([])
    assert wmx.wmx_conf_submit(cb._h, C.byref(slot), stream) == EINVAL and slot.value == -1
    cb.set_conferences(LAYOUT)
    after = state()
    assert after[0] == before[0] and after[3] == before[3]
    assert all(np.array_equal(before[1][k], after[1][k]) for k in before[1])
    assert all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(before[2], after[2]))
    cb.close()
    assert cb.rows_in is None and cb.recv is None and cb.rows_out is None  # views of pinned rows that are gone
