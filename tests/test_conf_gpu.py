"""wmx_conf (wmix_amd/csrc/conf.hip) through the Python mirror: a conference bridge of RTP/G.711 legs in one handle, datagram in, datagram
out.  Every datagram of every tick is compared with the whole-script replay of tests/conf_single_replays.py -- the oracle's ingest, one
reference ring per leg with a cursor per source leg (LegsOracle), the drain and the oracle's egress, fed by the same scripted arrivals --
and with replay_with() of the same module, which goes tick by tick so that the layout, the mute and the calls can change between
ticks.  The shape and the script are those of tests/conf_inputs.py, the runner that of tests/conf_harness.py.  Bytes, np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from conf_harness import bridge, run
from conf_inputs import EINVAL, G, K, LAYOUT, NULL_HEAD, SEED, T, arrivals
from conf_single_replays import replay, replay_with
from leg_oracle_model import Replay

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def script(oracle_port):
    pk, recv = arrivals(SEED, T, G)
    want, calls = replay(oracle_port, pk, recv, LAYOUT, "alsa")
    return pk, recv, want


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
