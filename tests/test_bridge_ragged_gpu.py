"""GPU parity of the bridge over a layout: conferences of different sizes whose legs join and leave (wmx_mix_set_conferences /
wmx_mix_load_minus_conf in wmix_amd/csrc/mix.hip, wmx_tick_bridge_conferences in tick.hip, bridge_layout.h).  The oracle is what
tests/test_bridge_gpu.py uses -- one reference ring (and, for the tick, one orc_pkgfifo and one orc_chain) per leg, and for every ring
the ordered orc_load_data calls of the other members of its conference -- with the one thing that is new: every conference has a cursor
of its own, and all of a conference's calls of one tick start from it.  Integer results, np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from conf_inputs import EINVAL, NULL_HEAD
import conftest
from leg_oracle_model import OracleRings
from oracle import loader as L
from test_bridge_gpu import N, room, talkers, volume_add

pytestmark = pytest.mark.gpu

NS_, AEC_, AGC_, VAD_ = 1, 2, 4, 8


# ---------------------------------------------------------------- the load against one reference mixer per leg
def ragged_layout():
    """sizes 32, 2, 0, 3, 17, 1, 5, 9 over 71 rings, two of them idle in between; the 3 and the 5 interleaved, the 9 reversed, the 17 odd
    positions first: no member list is both consecutive and ascending but the 2's and the 32's, and the size classes come in no order"""
    idle = [10, 40]
    pool = iter(r for r in range(71) if r not in idle)
    take = lambda k: [next(pool) for _ in range(k)]  # noqa: E731
    c2, mixed, c9, one, c17, c32 = take(2), take(8), take(9)[::-1], take(1), take(17), take(32)
    c3, c5 = mixed[0:6:2], mixed[1:6:2] + mixed[6:]
    return [c32, c2, [], c3, c17[1::2] + c17[0::2], one, c5, c9], idle


def oracle_minus_conf(rings, layout, src, sbytes, freq, chn, rarg, heads, ticks, mute):
    """for every conference of >= 2 members: the ring of member q <- the sources of the members s != q that are not muted, in list order,
    every call from the conference's cursor.  Returns the cursors afterwards (a conference's calls all end with the same one: asserted;
    one of fewer than 2 members has none)."""
    heads, ticks = list(heads), list(ticks)
    for c, mem in enumerate(layout):
        if len(mem) < 2:
            heads[c], ticks[c] = NULL_HEAD, 0
            continue
        ends = set()
        for q in mem:
            for s in mem:
                if s != q and not (mute is not None and mute[s]):
                    ends.add(rings.load(q, src[s], sbytes, freq, chn, heads[c], ticks[c], rarg))
        assert len(ends) == 1
        heads[c], ticks[c] = ends.pop()
    return heads, ticks


#        ring          source      rmode sbytes  wrap   mute
CASES = [
    ((1, 8000), (8000, 1), 1, 320, False, False),
    ((1, 16000), (8000, 1), 1, 320, False, False),    # the repair fill
    ((2, 16000), (11025, 2), 1, 884, False, False),   # the repair fill, a rate that does not divide, two channels
    ((1, 8000), (32000, 2), 1, 2560, False, False),   # decimation
    ((1, 8000), (8000, 1), 2, 320, False, False),     # reduce_mode 2 with reduce 1: the division
    ((1, 8000), (8000, 1), 1, 320, True, False),      # a head 128 bytes before the ring end: the span wraps
    ((1, 8000), (8000, 1), 1, 320, False, True),      # one member muted
]


@pytest.mark.parametrize("ring,source,rmode,sbytes,wrap,muted", CASES)
def test_load_minus_conf_against_one_reference_mixer_per_leg(cuda, oracle_port, ring, source, rmode, sbytes, wrap, muted):
    """Two calls.  The first starts every conference from a fresh cursor; before the second the play head has moved on to where a fresh
    cursor falls on the START of the ring (src/wmix.c:1666-1673) and one conference's cursor is forgotten, so that one re-forms there
    while the others continue where they were: conferences alive together with different cursors."""
    import torch
    from wmix_amd.mix import MixBatch
    ring_chn, ring_freq = ring
    freq, chn = source
    layout, idle = ragged_layout()
    n, per, rarg = 71, sbytes // 2, 1
    reform = 7  # the conference of 9
    rng = np.random.default_rng(2000 + sbytes + ring_freq)
    pre = rng.integers(-20000, 20000, size=(n, 1, per + chn), dtype=np.int16)
    src = rng.integers(-20000, 20000, size=(2, n, per + chn), dtype=np.int16)  # every row carries the fill's look-ahead frame
    mute = None
    if muted:
        mute = np.zeros(n, np.uint8)
        mute[layout[6][2]] = 1
    size = ring_chn * 2 * ring_freq
    orc = OracleRings(oracle_port, n, ring_chn, ring_freq, 0, rmode)
    correct = orc.play_correct
    # a source without a cursor starts play_correct in front of the head
    start1 = size - correct - (128 if wrap else 4096)
    start2 = size - correct  # head + play_correct is the ring's end: a fresh cursor is the ring's start
    # ---- the oracle: every ring pre-loaded with an ordinary source of its own, then the two bridge calls
    for r in orc.r:
        r.head_off = start1
    for k in range(n):
        orc.load(k, pre[k, 0], sbytes, freq, chn, NULL_HEAD, 0, rarg)
    before = [orc.ring(k) for k in range(n)]
    h1, t1 = oracle_minus_conf(orc, layout, src[0], sbytes, freq, chn, rarg, [NULL_HEAD] * 8, [0] * 8, mute)
    after1 = [orc.ring(k) for k in range(n)]
    for r in orc.r:
        r.head_off = start2
    forgotten = [NULL_HEAD if c == reform else h for c, h in enumerate(h1)]
    h2, t2 = oracle_minus_conf(orc, layout, src[1], sbytes, freq, chn, rarg, forgotten, t1, mute)
    # ---- on the oracle alone: the re-formed conference began at the ring's start, the others went on from where they were
    live = [c for c, mem in enumerate(layout) if len(mem) >= 2]
    span = h2[reform]  # bytes one call writes: its cursor began at 0
    assert 0 < span < 4096 and {h2[c] for c in live if c != reform} == {(size - (128 if wrap else 4096) + 2 * span) % size}
    assert len({(h2[c], t2[c]) for c in live}) == 2
    assert all((h2[c], t2[c]) == (NULL_HEAD, 0) for c in (2, 5))
    # ---- the device
    mb = MixBatch(n, ring_chn, ring_freq)
    mb.set(start1, 0, rmode)
    mb.load(torch.from_numpy(pre).to(cuda), sbytes, freq, chn, reduce=rarg)
    mb.set_conferences(layout)
    assert mb.conferences() == 8
    d = torch.from_numpy(src).to(cuda)
    dm = torch.from_numpy(mute).to(cuda) if mute is not None else None
    g1 = mb.load_minus_conf(d[0], sbytes, freq, chn, mute=dm, reduce=rarg)
    mid = [mb.export(k)[0] for k in range(n)]
    mb.set(start2, 0, rmode)
    g2 = mb.load_minus_conf(d[1], sbytes, freq, chn, mute=dm, head=forgotten, tick=t1, reduce=rarg)
    end = [mb.export(k)[0] for k in range(n)]
    mb.close()
    assert g1[0].tolist() == h1 and g1[1].tolist() == t1
    assert g2[0].tolist() == h2 and g2[1].tolist() == t2
    for k in range(n):
        assert np.array_equal(mid[k], after1[k]), ("first call, ring", k)
        assert np.array_equal(end[k], orc.ring(k)), ("second call, ring", k)
    for k in idle + layout[5]:  # idle legs and the member of the one-member placeholder: as the pre-load left them
        assert np.array_equal(end[k], before[k]) and before[k].any(), k
    assert all(not np.array_equal(after1[k], before[k]) for c in live for k in layout[c])


@pytest.mark.parametrize("P", [3, 8])
def test_equal_consecutive_conferences_are_the_uniform_bridge_load(cuda, P):
    """n / P consecutive ascending conferences of P members: the rings and cursors of wmx_mix_load_minus on a twin mixer, over two calls"""
    import torch
    from wmix_amd.mix import MixBatch
    n_conf, per = 5, 160
    n = n_conf * P
    rng = np.random.default_rng(300 + P)
    pre = torch.from_numpy(rng.integers(-20000, 20000, size=(n, 1, per + 1), dtype=np.int16)).to(cuda)
    src = torch.from_numpy(rng.integers(-20000, 20000, size=(2, n, per + 1), dtype=np.int16)).to(cuda)
    mute = np.zeros(n, np.uint8)
    mute[P + 1] = 1
    dm = torch.from_numpy(mute).to(cuda)
    twin, mb = MixBatch(n, 1, 8000), MixBatch(n, 1, 8000)
    for m in (twin, mb):
        m.set(16000 - 3200 - 128, 0, 2)  # the first span runs across the ring's end; reduce_mode 2 with reduce 1: the division
        m.load(pre, 320, 8000, 1)
    mb.set_conferences([list(range(c * P, c * P + P)) for c in range(n_conf)])
    want = twin.load_minus(src[0].view(n_conf, P, per + 1), P, 320, 8000, 1, mute=dm)
    got = mb.load_minus_conf(src[0], 320, 8000, 1, mute=dm)
    assert got[0].tolist() == [want[0]] * n_conf and got[1].tolist() == [want[1]] * n_conf
    want = twin.load_minus(src[1].view(n_conf, P, per + 1), P, 320, 8000, 1, mute=dm, head=want[0], tick=want[1])
    got = mb.load_minus_conf(src[1], 320, 8000, 1, mute=dm, head=got[0], tick=got[1])
    assert got[0].tolist() == [want[0]] * n_conf and got[1].tolist() == [want[1]] * n_conf
    for k in range(n):
        a, b = twin.export(k)[0], mb.export(k)[0]
        assert np.array_equal(a, b) and a.any(), k
    twin.close()
    mb.close()


def test_load_minus_conf_refusals_leave_rings_layout_and_cursors_alone(cuda, wmx):
    import torch
    from wmix_amd.mix import MixBatch
    n, per = 40, 160
    mb = MixBatch(n, 1, 8000)
    rng = np.random.default_rng(4)
    mb.load(torch.from_numpy(rng.integers(-20000, 20000, size=(n, 1, per + 1), dtype=np.int16)).to(cuda), 320, 8000, 1)
    src = torch.from_numpy(rng.integers(-20000, 20000, size=n * 9000, dtype=np.int16)).to(cuda)  # room for every call below, refused or not
    stream = torch.cuda.current_stream().cuda_stream

    def cursors(*pairs):
        return np.array([p[0] for p in pairs], np.uint32), np.array([p[1] for p in pairs], np.uint32)

    def load(src_ptr, sbytes, stride, h, t):
        hp, tp = (None if a is None else a.ctypes.data for a in (h, t))  # None: a NULL cursor array
        return wmx.wmx_mix_load_minus_conf(mb._h, src_ptr, sbytes, 8000, 1, 16, stride, None, 1, hp, tp, stream)

    # without a layout
    h, t = cursors((77, 5), (NULL_HEAD, 0))
    assert load(src.data_ptr(), 320, per, h, t) == EINVAL and b"layout" in wmx.wmx_last_error()
    assert wmx.wmx_mix_conferences(mb._h) == 0
    mb.set_conferences([[3, 1], [7, 5, 9]])
    first = mb.load_minus_conf(src[:n * (per + 1)].view(n, per + 1), 320, 8000, 1)
    before = [mb.export(k)[0] for k in range(n)]

    def set_layout(off, members, n_conf=None):
        off, members = np.array(off, np.int32), np.array(members, np.int32)
        return wmx.wmx_mix_set_conferences(mb._h, len(off) - 1 if n_conf is None else n_conf, off.ctypes.data, members.ctypes.data, stream)

    assert set_layout([0, 2, 35], list(range(35))) == EINVAL and b"WMX_MIX_MAX_PARTIES" in wmx.wmx_last_error()  # 33 members
    assert set_layout([0, 2], [0, 40]) == EINVAL and set_layout([0, 2], [-1, 0]) == EINVAL                          # outside [0, n_groups)
    assert set_layout([0, 3], [0, 1, 0]) == EINVAL and b"twice" in wmx.wmx_last_error()                             # twice in one conference
    assert set_layout([0, 2, 4], [0, 1, 2, 1]) == EINVAL                                                             # ... and in two
    assert set_layout([0, 3, 2, 4], [0, 1, 2, 3]) == EINVAL and set_layout([1, 2, 4], [0, 1, 2, 3]) == EINVAL      # non-monotone off
    assert set_layout([0, 2], [0, 1], n_conf=-1) == EINVAL
    assert wmx.wmx_mix_conferences(mb._h) == 2
    # what wmx_mix_load refuses: more than one ring of output; the cursors stay
    h, t = first[0].copy(), first[1].copy()
    assert load(src.data_ptr(), 17000, 9000, h, t) == EINVAL
    assert np.array_equal(h, first[0]) and np.array_equal(t, first[1])
    assert load(src.data_ptr(), 320, per, None, t) == EINVAL and load(src.data_ptr(), 320, per, h, None) == EINVAL
    # no source: 0, the cursors unchanged
    assert load(None, 320, per, h, t) == 0 and load(src.data_ptr(), 0, per, h, t) == 0
    assert np.array_equal(h, first[0]) and np.array_equal(t, first[1])
    torch.cuda.synchronize()
    for k in range(n):
        assert np.array_equal(mb.export(k)[0], before[k]), k
    # the layout in force is still the one that was set: the next call loads rings 1, 3, 5, 7, 9 and nothing else
    mb.load_minus_conf(src[:n * (per + 1)].view(n, per + 1), 320, 8000, 1, head=first[0], tick=first[1])
    changed = [k for k in range(n) if not np.array_equal(mb.export(k)[0], before[k])]
    assert changed == [1, 3, 5, 7, 9]
    mb.set_conferences([])  # n_conf == 0 clears it
    assert mb.conferences() == 0
    h, t = cursors((NULL_HEAD, 0))
    assert load(src.data_ptr(), 320, per, h, t) == EINVAL
    mb.close()


# ---------------------------------------------------------------- the tick against one daemon per leg
T_RUN, LEGS = 130, 10
SCHEDULE = [
    (0, [[0, 1], [2, 3, 4]]),
    (40, [[0, 1, 5], [2, 3, 4]]),             # leg 5 joins conference 0
    (45, [[0, 1, 5], [2, 3, 4], [6, 7, 8]]),  # legs 6, 7, 8 form conference 2
    (60, [[0, 1, 5], [2, 4], [6, 7, 8]]),     # leg 3 leaves
    (80, [[0, 1, 5], [2], [6, 7, 8]]),        # conference 1 is down to one leg
    (100, [[0, 1, 5], [2, 4], [6, 7, 8]]),    # legs 2 and 4 re-form it; leg 9 is never in one
]


def layout_at(schedule, t):
    return [lay for since, lay in schedule if since <= t][-1]


def conf_port(lib, local, stages, platform, schedule):
    """test_bridge_gpu.bridge_port with a layout per tick and a cursor per conference index: n daemons (1 x 8000 Hz ring, 20 ms
    packages) over T ticks; per leg one ring, one orc_pkgfifo, one orc_chain; per tick and leg the drain, FIFO add / get, the room and
    the chain step; then for every conference of >= 2 legs, for p in list order and q != p, orc_load_data(ring_q, out_p), every call of
    the conference from the conference's cursor (they all end with the same one: asserted).  A conference of fewer than 2 legs forgets
    its cursor, and so does one that is new in the layout.  Returns dict(play, far, out: [T, n, 160], cursors: {tick: [(head, tick)]})."""
    L.mix_bind(lib)
    T, n = local.shape[:2]
    aec_ms, correct = L.PLATFORMS[platform]
    rings = OracleRings(lib, n, 1, 8000, 0, 1)
    for r in rings.r:
        r.play_correct = correct
    n_slots = aec_ms // 20 + 2
    fstore = [np.zeros(n_slots * 2 * N, np.uint8) for _ in range(n)]
    fifos = [L._PkgFifo() for _ in range(n)]
    for k in range(n):
        lib.orc_pkgfifo_init(C.byref(fifos[k]), fstore[k].ctypes.data_as(C.c_void_p), n_slots, 2 * N, 20, 2)
    c_open = L._fn(lib, "orc_chain_open", C.c_void_p, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint])
    c_step = L._fn(lib, "orc_chain_step", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])
    chains = [c_open(1, 8000, 20, 5, stages) for _ in range(n)]
    play, far, out = (np.zeros((T, n, N), np.int16) for _ in range(3))
    zero = np.zeros(N, np.int16)
    cursor, seen = {}, {}
    pad = np.zeros(N + 8, np.int16)
    for t in range(T):
        for k in range(n):
            r = rings.r[k]
            ring = rings.store[k][:16000].view(np.int16)
            pos = (r.head_off // 2 + np.arange(N)) % 8000
            play[t, k] = ring[pos]
            ring[pos] = 0
            r.head_off = (r.head_off + 2 * N) % 16000
            r.tick += 2 * N
            lib.orc_pkgfifo_add(C.byref(fifos[k]), play[t, k].ctypes.data_as(C.c_void_p))
            assert lib.orc_pkgfifo_get(C.byref(fifos[k]), far[t, k].ctypes.data_as(C.c_void_p), aec_ms) == 0
            out[t, k] = L.tick_room(local[t, k], far[t, k], far[t - 1, k] if t else zero)
            assert c_step(chains[k], far[t, k].ctypes.data, out[t, k].ctypes.data, N) == 0
        layout = layout_at(schedule, t)
        for c in list(cursor):
            if c >= len(layout) or len(layout[c]) < 2:
                del cursor[c]
        for c, legs in enumerate(layout):
            if len(legs) < 2:
                continue
            ends = set()
            for p in legs:
                pad[:N] = out[t, p]
                for q in legs:
                    if q != p:
                        ends.add(rings.load(q, pad, 2 * N, 8000, 1, *cursor.get(c, (NULL_HEAD, 0)), 1))
            assert len(ends) == 1, "the cursors of conference %d drifted apart in tick %d" % (c, t)
            cursor[c] = ends.pop()
        seen[t] = [cursor.get(c) for c in range(len(layout))]
    for c in chains:
        L._fn(lib, "orc_chain_close", None, [C.c_void_p])(c)
    return {"play": play, "far": far, "out": out, "cursors": seen}


def gpu_conf(cuda, local, stages, platform, schedule):
    """the same run on the device: local [T, n, 160] -> dict(play, far, out: [T, n, 160])"""
    import torch
    from wmix_amd.tick import TickBatch
    T, n = local.shape[:2]
    tb = TickBatch.for_platform(platform, n, 1, stages=stages)
    assert tb.pkg == N
    dloc = torch.from_numpy(np.ascontiguousarray(local)).to(cuda)
    play, far, out, zoom = (torch.zeros((T, n, N), dtype=torch.int16, device=cuda) for _ in range(4))
    prev = torch.zeros((n, N), dtype=torch.int16, device=cuda)
    changes = dict(schedule)
    for t in range(T):
        if t in changes:
            tb.bridge_conferences(changes[t])
        f = tb.play(play[t])
        far[t].copy_(f)
        out[t].copy_(room(dloc[t], f, prev))
        prev = far[t]
        assert tb.record(out[t], zoom[t]) == 2 * N
    res = {"play": play.cpu().numpy(), "far": far.cpu().numpy(), "out": out.cpu().numpy()}
    assert np.array_equal(zoom.cpu().numpy(), res["out"])  # 1 x 8000 -> 1 x 8000: wmix_pcm_zoom copies
    tb.close()
    return res


def replay(out, schedule, correct):
    """What every loudspeaker plays, worked out from the legs' outputs alone (stages 0, numpy): the package a conference loads in tick t
    sits at its cursor, and the play head gets there a whole number of packages later -- a number fixed when the conference forms
    (src/wmix.c:1666-1673: VIEW_PLAY_CORRECT in front of the head, or the ring's start when that lies behind its end).  Nobody's own
    output is among what they are played."""
    T, n = out.shape[:2]
    exp = np.zeros((T + 64, n, N), np.int16)
    wait = {}
    for t in range(T):
        layout = layout_at(schedule, t)
        head = (t + 1) * 2 * N % 16000  # the drain of tick t is done when the heartbeat loads
        for c in list(wait):
            if c >= len(layout) or len(layout[c]) < 2:
                del wait[c]
        for c, legs in enumerate(layout):
            if len(legs) < 2:
                continue
            if c not in wait:
                fresh = head + correct if head + correct < 16000 else 0
                wait[c] = (fresh - head) % 16000 // (2 * N)
            at = t + 1 + wait[c]
            for q in legs:
                for s in legs:
                    if s != q:
                        exp[at, q] = volume_add(exp[at, q], out[t, s])
    return exp[:T], wait


@pytest.mark.parametrize("platform", ["alsa", "t31"])
@pytest.mark.parametrize("stages", [0, NS_ | AEC_ | AGC_ | VAD_])
def test_tick_with_joins_and_leaves_against_one_daemon_per_leg(cuda, oracle_port, platform, stages):
    """Ten legs over 130 ticks while the layout changes five times (SCHEDULE): every leg's played package, far-end package and chain
    output equal those of a daemon of its own.  Under platform/alsa conference 2 forms when the play head is past ring - 3 200, so its
    cursor is the ring's start and differs from conference 0's for the rest of the run: one cursor for all does not pass."""
    if stages & (NS_ | AEC_) and not conftest.host_powf_is_the_products():
        pytest.skip("the float path through a feedback loop is bit-exact only against an oracle that links the product's powf")
    correct = L.PLATFORMS[platform][1]
    # stages 0: for the first 38 ticks leg 1 is the only one in a room that is not dead silent
    local = talkers(52, T_RUN, LEGS, only=1, alone_for=38 if stages == 0 else 0)
    want = conf_port(oracle_port, local, stages, platform, SCHEDULE)
    # ---- on the oracle alone
    at45 = want["cursors"][45]
    if platform == "alsa":
        assert 46 * 2 * N + correct >= 16000 and at45[2] == (2 * N, 46 * 2 * N + correct + 2 * N)  # began at the ring's start
        assert all(want["cursors"][t][2][0] != want["cursors"][t][0][0] for t in range(45, T_RUN))
    else:
        assert at45[2] == at45[0]
    assert want["cursors"][79][1] is not None and want["cursors"][80][1] is None and want["cursors"][100][1] is not None
    # ---- the device
    got = gpu_conf(cuda, local, stages, platform, SCHEDULE)
    for k in ("play", "far", "out"):
        assert np.array_equal(got[k], want[k]), (k, np.argwhere((got[k] != want[k]).any(2))[:4])
    assert all(got["play"][:, k].any() for k in range(9))
    if stages != 0:
        return
    play, out = got["play"], got["out"]
    lead = 1 + correct // (2 * N)  # a package loaded in tick t from a cursor that began in front of the head is played `lead` ticks later
    # nobody plays their own output, idle legs and placeholder members are loaded nothing: every loudspeaker from the outputs alone
    exp, wait = replay(out, SCHEDULE, correct)
    assert np.array_equal(play, exp)
    assert wait[0] == lead - 1 and wait[2] == (4 if platform == "alsa" else 0)
    # ... and leg 1, alone in a live room at first, is not played its own voice: silent until leg 0's microphone has picked it up from
    # leg 0's loudspeaker and sent it back, while leg 0 hears it all along
    first_back = int(np.argmax(out[:, 0].any(1)))
    assert 0 < first_back < 38 and not play[:first_back + 1, 1].any() and play[:first_back + 1, 0].any()
    # legs 0 and 1 play what they would have played had leg 5 never joined, up to the first package that carries leg 5: no gap at tick 40
    never = [(since, [[k for k in legs if k != 5] for legs in lay]) for since, lay in SCHEDULE]
    without = gpu_conf(cuda, local, 0, platform, never)["play"]
    assert np.array_equal(play[:40 + lead, :2], without[:40 + lead, :2]) and play[39 + lead, 0].any()
    assert not np.array_equal(play[40 + lead, 0], without[40 + lead, 0]) and out[40, 5].any()
    assert not without[:, 5].any() and not play[:40 + lead, 5].any() and play[40 + lead, 5].any()
    # leg 3's loudspeaker plays out what it was loaded and goes silent one lead after tick 60, for good
    assert play[59 + lead, 3].any() and not play[60 + lead:, 3].any()
    # leg 9 talks and is never in a conference: it plays nothing, and nobody plays it (replay above)
    assert out[:, 9].any() and not play[:, 9].any()


def test_the_layout_excludes_the_uniform_bridge_and_rw_test(cuda, wmx):
    from wmix_amd.tick import TickBatch
    stream = None
    off, mem = np.array([0, 2, 5], np.int32), np.array([0, 1, 2, 3, 4], np.int32)

    def conferences(tb, n_conf=2):
        return wmx.wmx_tick_bridge_conferences(tb._h, n_conf, off.ctypes.data, mem.ctypes.data, stream)

    tb = TickBatch.for_platform("t31", 6, 1, stages=0)
    assert conferences(tb) == 0 and wmx.wmx_mix_conferences(wmx.wmx_tick_mix(tb._h)) == 2
    assert wmx.wmx_tick_rw_test(tb._h, 1) == EINVAL
    assert wmx.wmx_tick_bridge(tb._h, 3) == EINVAL and b"wmx_tick_bridge_conferences" in wmx.wmx_last_error()
    bad = np.array([0, 1, 2, 3, 6], np.int32)  # ring 6 of 6: refused, and the layout in force stays
    assert wmx.wmx_tick_bridge_conferences(tb._h, 2, off.ctypes.data, bad.ctypes.data, stream) == EINVAL
    assert wmx.wmx_mix_conferences(wmx.wmx_tick_mix(tb._h)) == 2
    assert conferences(tb, 0) == 0 and wmx.wmx_mix_conferences(wmx.wmx_tick_mix(tb._h)) == 0  # off
    tb.rw_test(True)
    assert conferences(tb) == EINVAL
    tb.rw_test(False)
    tb.bridge(3)
    assert conferences(tb) == EINVAL
    tb.bridge(0)
    assert conferences(tb) == 0
    tb.close()
    two = TickBatch.for_platform("t31", 6, 2, stages=0)  # two record streams per group: not a conference of call legs
    assert conferences(two) == EINVAL and b"rec_per_group" in wmx.wmx_last_error()
    two.close()


def test_host_tick_with_conferences_of_different_sizes(tmp_path, oracle_port):
    """examples/host_tick.c --bridge-sizes 2,3,4: consecutive conferences of those sizes over 10 legs, the last one idle, from plain C"""
    import json
    import os
    import subprocess
    if not conftest.host_powf_is_the_products():
        pytest.skip("the float path through a feedback loop is bit-exact only against an oracle that links the product's powf")
    exe = os.path.join(conftest.ROOT, "examples", "host_tick")
    assert os.path.exists(exe), "examples/host_tick missing: run __graft_entry__.build()"
    T, n = 60, 10
    local = talkers(124, T, n)
    np.zeros((T, n, 1, N), "<i2").tofile(tmp_path / "src.i16")  # no task thread plays anything: the legs hear each other only
    local.astype("<i2").tofile(tmp_path / "local.i16")
    cmd = [exe, str(tmp_path / "src.i16"), str(tmp_path / "local.i16"), str(tmp_path / "out.i16"), str(n), "1", "1", str(T), "8000", "1",
           "--platform", "t31", "--bridge-sizes", "2,3,4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["rc"] == 0 and info["bridge_sizes"] == [2, 3, 4]
    got = np.fromfile(tmp_path / "out.i16", dtype="<i2").reshape(T, 3 * n, N)
    want = conf_port(oracle_port, local, 15, "t31", [(0, [[0, 1], [2, 3, 4], [5, 6, 7, 8]])])
    assert want["play"][:, :9].any((0, 2)).all() and not want["play"][:, 9].any()
    assert np.array_equal(got[:, :n], want["play"]) and np.array_equal(got[:, n:2 * n], want["far"]) and np.array_equal(got[:, 2 * n:], want["out"])
    for sizes in ("2,3,6", "2,33", "2,x"):  # 11 legs of 10; more than 32; not a number
        bad = subprocess.run(cmd[:-1] + [sizes], capture_output=True, text=True, timeout=60)
        assert bad.returncode == 4 and "wmx_tick_bridge" in bad.stderr, sizes
