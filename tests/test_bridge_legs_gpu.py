"""GPU parity of the bridge with a cursor per leg: wmx_mix_load_minus_legs / wmx_mix_reset_leg_cursors / wmx_mix_export_leg_cursors
(wmix_amd/csrc/mix.hip, leg_cursor.h) through the Python mirror.  An RTP leg delivers 0, 1, 2 or 3 datagrams in a 20 ms tick; every
wmix_thread_rtp_recv_pcma keeps a cursor of its own and calls wmix_load_data once per datagram that arrived (src/wmixTask.c:1266-1316).
So the oracle is what tests/test_bridge_gpu.py uses -- one reference ring per leg, and for every ring the ordered orc_load_data calls
of the other members of its conference -- with one cursor per SOURCE leg and as many calls per tick as that leg has valid slots:
LegsOracle over OracleRings, both of tests/leg_oracle_model.py.  Integer results, np.array_equal."""
import numpy as np
import pytest

from conf_inputs import EINVAL, NULL_HEAD
from leg_oracle_model import LegsOracle

pytestmark = pytest.mark.gpu

K = 3  # max_packets


def main_layout():
    """sizes 2, 3, 5, 9 and 17, a one-member placeholder and three rings in no conference (one of them joins later) over 40 rings;
    no member list but the 2's is ascending, and the size classes come in no order"""
    idle = [7, 20, 33]
    pool = iter(r for r in range(40) if r not in idle)
    take = lambda k: [next(pool) for _ in range(k)]  # noqa: E731
    c2, mixed, c9, one, c17 = take(2), take(8), take(9)[::-1], take(1), take(17)
    c3, c5 = mixed[0:6:2][::-1], mixed[1:6:2] + mixed[6:]
    return [c17[1::2] + c17[0::2], c2, [], c3, one, c5, c9], idle


def big_layout():
    """sizes 32, 4 and 2 and two idle rings over 40; the 32 reversed"""
    return [[38, 36], list(range(35, 3, -1)), [0, 2, 1, 3]], [37, 39]


def script(T, n, roles, sbytes, seed):
    """lens [T, n, K]: every leg sends one valid packet per tick in slot 0 but the scripted ones.  A slot that is no call holds 0, a
    shorter length or a longer one."""
    rng = np.random.default_rng(seed)
    lens = np.zeros((T, n, K), np.uint32)
    lens[:, :, 0] = sbytes
    t = np.arange(T)
    if "lossy" in roles:  # drops every third packet; in the second half it sends two at once after each gap
        r = roles["lossy"]
        lens[t % 3 == 2, r, 0] = 0
        lens[(t % 3 == 0) & (t >= T // 2), r, 1] = sbytes
    if "silent" in roles:  # silent for 15 ticks: falls behind, jumps when it returns
        lens[20:35, roles["silent"], :] = 0
    if "burst" in roles:  # 3 per tick for 10 ticks: runs ahead, stays inside the ring
        lens[10:20, roles["burst"], :] = sbytes
    if "gap" in roles:  # an invalid slot between two valid ones every other tick, nothing in between
        r = roles["gap"]
        lens[t % 2 == 0, r, 2] = sbytes
        lens[t % 2 == 0, r, 1] = np.where(t[t % 2 == 0] % 4 == 0, sbytes - 2, sbytes + 2)
        lens[t % 2 == 1, r, :] = 0
    if "leaver" in roles:  # two per tick for the ten ticks before it leaves: its cursor is ahead when it comes back as a new call
        lens[40:50, roles["leaver"], 1] = sbytes
    junk = rng.integers(0, 4, size=lens.shape)  # what a slot that made no call holds does not matter
    lens = np.where(lens == sbytes, lens, np.array([0, 1, sbytes - 1, 2 * sbytes], np.uint32)[junk]).astype(np.uint32)
    return lens


def layout_at(schedule, t):
    return [lay for since, lay in schedule if since <= t][-1]


def run_both(cuda, lib, ring, source, rmode, sbytes, play_correct, schedule, resets, lens, mute, seed, T, check_at, drop_rule=False):
    """T ticks of 20 ms on the oracle and on the device: drain one package, then the load.  Returns the device's export at the end."""
    import torch
    from wmix_amd.mix import MixBatch
    freq, chn = source
    n, per = lens.shape[1], sbytes // 2
    rng = np.random.default_rng(seed)
    src = rng.integers(-20000, 20000, size=(T, n, K, per + chn), dtype=np.int16)  # every row carries the fill's look-ahead frame
    orc = LegsOracle(lib, n, ring, rmode, play_correct, drop_rule)
    mb = MixBatch(n, ring[0], ring[1])
    mb.set(0, 0, rmode)
    if play_correct is not None:
        mb.set_play_correct(play_correct)
    n_out = orc.samples_of_a_call(lib, ring, sbytes, freq, chn)
    dsrc, dlens = torch.from_numpy(src).to(cuda), torch.from_numpy(lens.view(np.int32)).to(cuda)
    dmute = torch.from_numpy(mute).to(cuda) if mute is not None else None
    changes = dict(schedule)
    for t in range(T):
        if t in changes:
            mb.set_conferences(changes[t])
        if t in resets:
            mb.reset_leg_cursors(resets[t])
            orc.reset(resets[t])
        want = orc.drain()
        got = mb.drain(orc.pkg).cpu().numpy()
        assert np.array_equal(got, want), ("drained rows, tick", t, np.argwhere((got != want).any(1))[:6].ravel())
        orc.load(layout_at(schedule, t), src[t], lens[t], sbytes, freq, chn, n_out, mute)
        mb.load_minus_legs(dsrc[t], sbytes, freq, chn, dlens[t], mute=dmute)
        if t + 1 in check_at:
            h, tk, dropped = mb.export_leg_cursors()
            wh, wt = orc.cursors()
            assert np.array_equal(h, wh) and np.array_equal(tk, wt), ("cursors after tick", t, np.argwhere((h != wh) | (tk != wt)).ravel())
            assert np.array_equal(dropped, orc.dropped), ("dropped after tick", t)
            for k in range(n):
                assert np.array_equal(mb.export(k)[0], orc.rings.ring(k)), ("ring", k, "after tick", t)
    res = mb.export_leg_cursors()
    mb.close()
    return res, orc


#         ring         source      rmode sbytes
FORMATS = [
    ((1, 8000), (8000, 1), 1, 320),
    ((1, 16000), (8000, 1), 1, 320),    # the repair fill
    ((1, 8000), (32000, 2), 1, 2560),   # decimation
    ((1, 8000), (8000, 1), 2, 320),     # reduce_mode 2 with reduce 1: the division
]


@pytest.mark.parametrize("play_correct", [0, None])
@pytest.mark.parametrize("ring,source,rmode,sbytes", FORMATS)
def test_legs_with_their_own_arrivals_against_one_reference_mixer_per_leg(cuda, oracle_port, ring, source, rmode, sbytes, play_correct):
    """80 ticks, so the 1 s ring wraps, over conferences of 2, 3, 5, 9 and 17 with a steady majority and: a leg that drops every third
    packet and later sends two at once; one silent for 15 ticks; one that sends 3 per tick for 10 ticks; a muted one that keeps
    sending; one with an invalid slot between two valid ones; one that joins at tick 30 as a new call; one that leaves at tick 50 with
    its cursor ahead and comes back at 55 as a new call.  Drained rows every tick; rings, cursors and drop counts at ticks 1, 40, 80."""
    T = 80
    layout, idle = main_layout()
    c17, c3, c5, c9 = layout[0], layout[3], layout[5], layout[6]
    joiner, leaver = idle[1], c9[4]
    roles = {"lossy": c3[1], "silent": c5[2], "burst": c9[1], "gap": c17[5], "leaver": leaver}
    muted = c17[9]
    lens = script(T, 40, roles, sbytes, 5)
    mute = np.zeros(40, np.uint8)
    mute[muted] = 1
    with_joiner = layout[:3] + [c3 + [joiner]] + layout[4:]
    without_leaver = with_joiner[:6] + [[r for r in c9 if r != leaver]]
    schedule = [(0, layout), (30, with_joiner), (50, without_leaver), (55, with_joiner)]
    (h, tk, dropped), orc = run_both(cuda, oracle_port, ring, source, rmode, sbytes, play_correct, schedule, {30: [joiner], 55: [leaver]}, lens, mute,
                                     100 + sbytes + ring[1], T, {1, 40, 80})
    assert not dropped.any()
    # on the oracle alone: the script did what it is for
    fresh = [r for r in range(40) if orc.cursor[r] == (NULL_HEAD, 0)]
    assert fresh == sorted([idle[0], idle[2]] + layout[4])  # never in a conference of two: no cursor
    assert orc.cursor[muted] != (NULL_HEAD, 0)              # the muted leg's cursor moved
    steady = orc.cursor[layout[1][0]]
    assert orc.cursor[layout[1][1]] == steady and orc.cursor[joiner] != (NULL_HEAD, 0)
    if orc.pkg == 2 * orc.samples_of_a_call(oracle_port, ring, sbytes, *source):  # a call loads what a tick plays (the fill's 319 do not)
        assert orc.cursor[joiner] == steady and orc.cursor[leaver] == steady      # a new call lands where a steady leg is


def test_legs_in_a_conference_of_32(cuda, oracle_port):
    T = 80
    layout, idle = big_layout()
    c32 = layout[1]
    roles = {"lossy": c32[3], "silent": c32[30], "burst": c32[17], "gap": c32[8]}
    lens = script(T, 40, roles, 320, 6)
    mute = np.zeros(40, np.uint8)
    mute[c32[12]] = 1
    (h, tk, dropped), orc = run_both(cuda, oracle_port, (1, 8000), (8000, 1), 1, 320, None, [(0, layout)], {}, lens, mute, 77, T, {1, 40, 80})
    assert not dropped.any() and all(orc.cursor[r] == (NULL_HEAD, 0) for r in idle)


def test_a_leg_that_overruns_the_ring_is_dropped_not_lapped(cuda, oracle_port):
    """One leg sends 3 per tick for good: once its end cursor would lie more than one ring ahead of the mixer's tick the call is not made,
    nor are the later slots of that tick.  The rings equal an oracle for which exactly those calls are not made."""
    T, n = 40, 7
    layout = [[4, 0, 2], [], [5, 1]]
    lens = script(T, n, {}, 320, 7)
    lens[:, 0, :] = 320
    (h, tk, dropped), orc = run_both(cuda, oracle_port, (1, 8000), (8000, 1), 1, 320, None, [(0, layout)], {}, lens, None, 9, T, {1, 25, 40},
                                     drop_rule=True)
    assert np.array_equal(dropped, orc.dropped)
    # the leg gains two packages a tick on a lead of 200 ms: it reaches the bound after 20 ticks, then two of its three calls are left out
    assert dropped[0] == orc.dropped[0] > 30 and not dropped[1:].any()
    assert tk[0] - orc.rings.r[0].tick <= 16000 < tk[0] - orc.rings.r[0].tick + 320


def test_steady_arrivals_from_fresh_cursors_are_the_common_cursor_bridge_load(cuda):
    """every leg sends one valid packet, nobody muted: the rings and every leg's cursor equal wmx_mix_load_minus_conf's on a twin mixer"""
    import torch
    from wmix_amd.mix import MixBatch
    layout, idle = main_layout()
    n, per, T = 40, 160, 4
    rng = np.random.default_rng(31)
    pre = torch.from_numpy(rng.integers(-20000, 20000, size=(n, 1, per + 1), dtype=np.int16)).to(cuda)
    src = torch.from_numpy(rng.integers(-20000, 20000, size=(T, n, 1, per + 1), dtype=np.int16)).to(cuda)
    lens = torch.full((n, 1), 320, dtype=torch.int32, device=cuda)
    twin, mb = MixBatch(n, 1, 8000), MixBatch(n, 1, 8000)
    for m in (twin, mb):
        m.set(16000 - 3200 - 480, 0, 2)  # the second span runs across the ring's end; reduce_mode 2 with reduce 1: the division
        m.load(pre, 320, 8000, 1)
        m.set_conferences(layout)
    cur = None, None
    for t in range(T):
        cur = twin.load_minus_conf(src[t, :, 0], 320, 8000, 1, head=cur[0], tick=cur[1])
        mb.load_minus_legs(src[t], 320, 8000, 1, lens)
        assert np.array_equal(twin.drain(320).cpu().numpy(), mb.drain(320).cpu().numpy()), t
    h, tk, dropped = mb.export_leg_cursors()
    for c, mem in enumerate(layout):
        for r in mem:
            assert (h[r], tk[r]) == ((cur[0][c], cur[1][c]) if len(mem) >= 2 else (NULL_HEAD, 0)), (c, r)
    assert all((h[r], tk[r]) == (NULL_HEAD, 0) for r in idle) and not dropped.any()
    for k in range(n):
        a, b = twin.export(k)[0], mb.export(k)[0]
        assert np.array_equal(a, b) and (a.any() or k in idle + layout[4]), k
    twin.close()
    mb.close()


def test_load_minus_legs_refusals_leave_rings_layout_and_cursors_alone(cuda, wmx):
    import torch
    from wmix_amd.mix import MixBatch
    n, per = 12, 160
    mb = MixBatch(n, 1, 8000)
    rng = np.random.default_rng(4)
    mb.load(torch.from_numpy(rng.integers(-20000, 20000, size=(n, 1, per + 1), dtype=np.int16)).to(cuda), 320, 8000, 1)
    src = torch.from_numpy(rng.integers(-20000, 20000, size=n * 4 * 9000, dtype=np.int16)).to(cuda)  # room for every call below, refused or not
    lens = torch.full((n, 4), 320, dtype=torch.int32, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream

    def load(src_ptr, sbytes, max_packets, len_ptr, freq=8000, stride=9000):
        return wmx.wmx_mix_load_minus_legs(mb._h, src_ptr, sbytes, freq, 1, 16, 4 * stride, stride, max_packets, len_ptr, None, 1, stream)

    def state():
        torch.cuda.synchronize()
        return [mb.export(k)[0] for k in range(n)], mb.export_leg_cursors(), mb.conferences()

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and a[2] == b[2]

    # without a layout; the cursors read fresh before any call
    first = state()
    assert (first[1][0] == NULL_HEAD).all() and not first[1][1].any() and not first[1][2].any()
    assert load(src.data_ptr(), 320, 3, lens.data_ptr()) == EINVAL and b"layout" in wmx.wmx_last_error()
    assert same(state(), first)
    mb.set_conferences([[3, 1], [7, 5, 9]])
    assert load(src.data_ptr(), 320, 3, lens.data_ptr()) == 0
    before = state()
    assert not same(before, first) and sorted(np.flatnonzero(before[1][0] != NULL_HEAD)) == [1, 3, 5, 7, 9]
    for max_packets in (0, 5, -1):
        assert load(src.data_ptr(), 320, max_packets, lens.data_ptr()) == EINVAL and b"max_packets" in wmx.wmx_last_error(), max_packets
    assert load(None, 320, 3, lens.data_ptr()) == EINVAL and load(src.data_ptr(), 320, 3, None) == EINVAL
    assert load(src.data_ptr(), 6000, 3, lens.data_ptr()) == EINVAL and b"do not fit" in wmx.wmx_last_error()  # 3 x 3000 samples > the ring
    assert load(src.data_ptr(), 17000, 1, lens.data_ptr()) == EINVAL                                           # what wmx_mix_load refuses: one ring
    assert load(src.data_ptr(), 320, 3, lens.data_ptr(), freq=100) == EINVAL  # ... and a ratio it cannot fill
    idx = np.array([1, 12], np.int32)
    assert wmx.wmx_mix_reset_leg_cursors(mb._h, idx.ctypes.data, 2, stream) == EINVAL
    assert same(state(), before)
    # still working, on the layout that was set: rings 1, 3, 5, 7, 9 and nothing else
    assert load(src.data_ptr(), 320, 3, lens.data_ptr()) == 0
    after = state()
    assert [k for k in range(n) if not np.array_equal(after[0][k], before[0][k])] == [1, 3, 5, 7, 9]
    mb.reset_leg_cursors([3, 9])
    h, tk, _ = mb.export_leg_cursors()
    assert sorted(np.flatnonzero(h != NULL_HEAD)) == [1, 5, 7] and not tk[[3, 9]].any()
    mb.reset_leg_cursors()
    assert (mb.export_leg_cursors()[0] == NULL_HEAD).all()
    mb.close()
