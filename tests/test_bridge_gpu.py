"""GPU parity of the conference bridge: wmx_mix_load_minus (wmix_amd/csrc/mix.hip) and wmx_tick_bridge (tick.hip) through the Python
mirrors of the C ABI.  A conference of P call legs is P reference daemons whose cleaned microphone p is fed with wmix_load_data into
the ring of every other daemon q != p, so the oracle here is exactly that: P rings per conference and P - 1 ordered orc_load_data calls
per ring (and, for the tick, one orc_pkgfifo and one orc_chain per participant, composed after oracle.loader.tick_port).  Integer
results, np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import conftest
from conf_inputs import EINVAL, NULL_HEAD
from leg_oracle_model import OracleRings
from oracle import loader as L

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the load against P reference mixers per conference
def oracle_minus(rings, P, src, sbytes, freq, chn, rarg, cursor, mute):
    """ring c*P+q <- the sources s != q of conference c that are not muted, in index order, every call from `cursor`.  Returns the
    cursor the calls end with (they all end with the same one: asserted)."""
    ends = set()
    for c in range(src.shape[0]):
        for q in range(P):
            for s in range(P):
                if s != q and not (mute is not None and mute[c * P + s]):
                    ends.add(rings.load(c * P + q, src[c, s], sbytes, freq, chn, cursor[0], cursor[1], rarg))
    assert len(ends) == 1
    return ends.pop()


#        P  ring          source        rmode rarg sbytes  wrap   mute
CASES = [
    (2, (1, 8000), (8000, 1), 1, 1, 320, False, False),
    (3, (1, 8000), (8000, 1), 1, 1, 320, False, False),
    (8, (1, 8000), (8000, 1), 1, 1, 320, False, False),
    (16, (1, 8000), (8000, 1), 1, 1, 320, False, False),
    (32, (1, 8000), (8000, 1), 1, 1, 320, False, False),
    (3, (1, 8000), (32000, 2), 1, 1, 2560, False, False),    # decimation
    (8, (1, 16000), (8000, 1), 1, 1, 320, False, False),     # the repair fill
    (3, (2, 16000), (11025, 2), 1, 1, 884, False, False),    # the repair fill, a rate that does not divide, two channels
    (8, (1, 8000), (8000, 1), 2, 1, 320, False, False),      # reduce_mode 2 with reduce 1: the division
    (8, (1, 8000), (8000, 1), 1, 1, 320, True, False),       # a head 128 bytes before the ring end: the span wraps
    (8, (1, 8000), (8000, 1), 1, 1, 320, False, True),       # one participant of one conference muted
    (16, (2, 16000), (11025, 2), 2, 1, 884, True, True),
]


@pytest.mark.parametrize("P,ring,source,rmode,rarg,sbytes,wrap,muted", CASES)
def test_load_minus_against_one_reference_mixer_per_participant(cuda, oracle_port, P, ring, source, rmode, rarg, sbytes, wrap, muted):
    import torch
    from wmix_amd.mix import MixBatch
    ring_chn, ring_freq = ring
    freq, chn = source
    n_conf, per = 3, sbytes // 2
    n = n_conf * P
    rng = np.random.default_rng(1000 + P + sbytes)
    # three conferences with different data; every row carries the up-sampling fill's look-ahead frame
    pre = rng.integers(-20000, 20000, size=(n, 1, per + chn), dtype=np.int16)
    src = rng.integers(-20000, 20000, size=(2, n_conf, P, per + chn), dtype=np.int16)
    mute = None
    if muted:
        mute = np.zeros(n, np.uint8)
        mute[1 * P + (P - 1) // 2] = 1
    size = ring_chn * 2 * ring_freq
    start = 0
    orc = OracleRings(oracle_port, n, ring_chn, ring_freq, 0, rmode)
    if wrap:
        start = size - 128 - orc.play_correct  # a source without a cursor starts play_correct in front of the head
        for r in orc.r:
            r.head_off = start
    # ---- the oracle: every ring pre-loaded with an ordinary source of its own, then the P - 1 foreign sources in order, twice
    for k in range(n):
        orc.load(k, pre[k, 0], sbytes, freq, chn, NULL_HEAD, 0, rarg)
    before = [orc.ring(k) for k in range(n)]
    cur1 = oracle_minus(orc, P, src[0], sbytes, freq, chn, rarg, (NULL_HEAD, 0), mute)
    after1 = [orc.ring(k) for k in range(n)]
    cur2 = oracle_minus(orc, P, src[1], sbytes, freq, chn, rarg, cur1, mute)
    # ---- what keeps the test honest, on the oracle's rings alone: the result is not clip(ring before + sum of all - own)
    if P in (8, 16) and (freq, chn) == (ring_freq, ring_chn) and rmode == 1 and not wrap and not muted:
        pos = (start + orc.play_correct) // 2 + np.arange(per)
        total = src[0][:, :, :per].astype(np.int64).sum(1)  # [n_conf, per]
        differ = 0
        for c in range(n_conf):
            for q in range(P):
                shortcut = np.clip(before[c * P + q][pos].astype(np.int64) + total[c] - src[0][c, q, :per], -32768, 32767)
                differ += int((shortcut != after1[c * P + q][pos]).sum())
        share = differ / (n * per)
        print("P = %d: clip(total - own) differs from the ordered saturating adds on %.1f %% of the written samples" % (P, 100 * share))
        assert share >= 0.10
    # ---- the device
    mb = MixBatch(n, ring_chn, ring_freq)
    mb.set(start, 0, rmode)
    mb.load(torch.from_numpy(pre).to(cuda), sbytes, freq, chn, reduce=rarg)
    d = torch.from_numpy(src).to(cuda)
    dm = torch.from_numpy(mute).to(cuda) if mute is not None else None
    got1 = mb.load_minus(d[0], P, sbytes, freq, chn, mute=dm, reduce=rarg)
    mid = [mb.export(k)[0] for k in range(n)]
    got2 = mb.load_minus(d[1], P, sbytes, freq, chn, mute=dm, head=got1[0], tick=got1[1], reduce=rarg)
    end = [mb.export(k)[0] for k in range(n)]
    mb.close()
    assert got1 == cur1 and got2 == cur2
    for k in range(n):
        assert np.array_equal(mid[k], after1[k]), ("first call, ring", k)
        assert np.array_equal(end[k], orc.ring(k)), ("second call, ring", k)
    assert any(not np.array_equal(after1[k], before[k]) for k in range(n))


def test_load_minus_refusals_leave_the_rings_alone(cuda, wmx):
    import torch
    from wmix_amd.mix import MixBatch
    n, per = 12, 160
    mb = MixBatch(n, 1, 8000)
    rng = np.random.default_rng(4)
    mb.load(torch.from_numpy(rng.integers(-20000, 20000, size=(n, 1, per + 1), dtype=np.int16)).to(cuda), 320, 8000, 1)
    before = [mb.export(k)[0] for k in range(n)]
    assert any(r.any() for r in before)
    src = torch.from_numpy(rng.integers(-20000, 20000, size=120000, dtype=np.int16)).to(cuda)  # room for every call below, refused or not
    stream = torch.cuda.current_stream().cuda_stream
    for parties in (1, 33, 5, 8, -2):  # 5 and 8 do not divide 12
        h, t = C.c_uint32(NULL_HEAD), C.c_uint32(0)
        rc = wmx.wmx_mix_load_minus(mb._h, parties, src.data_ptr(), 320, 8000, 1, 16, parties * per, per, None, 1, C.byref(h), C.byref(t), stream)
        assert rc == EINVAL and b"parties" in wmx.wmx_last_error(), parties
        assert (h.value, t.value) == (NULL_HEAD, 0)
    # what wmx_mix_load refuses: more than one ring of output
    h, t = C.c_uint32(NULL_HEAD), C.c_uint32(0)
    assert wmx.wmx_mix_load_minus(mb._h, 3, src.data_ptr(), 17000, 8000, 1, 16, 3 * 9000, 9000, None, 1, C.byref(h), C.byref(t), stream) == EINVAL
    # no source: 0, the cursor unchanged
    h, t = C.c_uint32(77), C.c_uint32(5)
    assert wmx.wmx_mix_load_minus(mb._h, 3, None, 320, 8000, 1, 16, 0, 0, None, 1, C.byref(h), C.byref(t), stream) == 0
    assert wmx.wmx_mix_load_minus(mb._h, 3, src.data_ptr(), 0, 8000, 1, 16, 0, 0, None, 1, C.byref(h), C.byref(t), stream) == 0
    assert (h.value, t.value) == (77, 5)
    torch.cuda.synchronize()
    for k in range(n):
        assert np.array_equal(mb.export(k)[0], before[k])
    mb.close()


def test_an_ordinary_load_after_a_bridge_load_is_unchanged(cuda, oracle_port):
    """wmx_mix_load on a mixer that has also seen wmx_mix_load_minus (same schedule cache, same cursor rule) still equals the oracle."""
    import torch
    from wmix_amd.mix import MixBatch
    P, n_conf, per = 4, 2, 160
    n = P * n_conf
    rng = np.random.default_rng(21)
    src = rng.integers(-20000, 20000, size=(n_conf, P, per + 1), dtype=np.int16)
    plain = rng.integers(-20000, 20000, size=(n, 3, 2 * 640 + 2), dtype=np.int16)  # 3 sources of 2 x 32 000 per ring
    orc = OracleRings(oracle_port, n, 1, 8000, 64, 1)
    cur = oracle_minus(orc, P, src, 320, 8000, 1, 1, (NULL_HEAD, 0), None)
    ends = {orc.load(k, plain[k, s], 2560, 32000, 2, cur[0], cur[1], 1) for k in range(n) for s in range(3)}
    assert len(ends) == 1
    mb = MixBatch(n, 1, 8000)
    mb.set(64, 0, 1)
    got = mb.load_minus(torch.from_numpy(src).to(cuda), P, 320, 8000, 1)
    got2 = mb.load(torch.from_numpy(plain).to(cuda), 2560, 32000, 2, head=got[0], tick=got[1])
    assert got == cur and got2 == ends.pop()
    for k in range(n):
        assert np.array_equal(mb.export(k)[0], orc.ring(k)), k
    mb.close()


# ---------------------------------------------------------------- the bridge tick against P daemons per conference
N = 160  # one package of the shipped format: 1 x 8000 Hz, 20 ms


def bridge_port(lib, local, P, stages, platform, on=None, mute=None):
    """n = local.shape[1] daemons (1 x 8000 Hz ring, 20 ms packages) over T ticks, composed after oracle.loader.tick_port: per
    participant one ring, one orc_pkgfifo, one orc_chain; per tick and participant the drain, FIFO add / get, the room
    (tick_room on the participant's OWN far-end) and the chain step; then, for the conferences of P consecutive participants,
    for p in index order and q != p, orc_load_data(ring_q, out_p) with a cursor per (p, q) pair -- where the rwTest load sits in
    the heartbeat (src/wmix.c:716-726).  on(t): is the bridge on in tick t (off forgets the cursors); mute(t, p): is p muted.
    Asserts that the cursors of all pairs that load in one tick are equal: that is what lets the device keep ONE.
    Returns dict(play, far, out: [T, n, 160])."""
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
    cursors = {}
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
        if on is not None and not on(t):
            cursors = {}
            continue
        ends = set()
        for c in range(n // P):
            for p in range(c * P, c * P + P):
                if mute is not None and mute(t, p):
                    continue
                pad[:N] = out[t, p]
                for q in range(c * P, c * P + P):
                    if q != p:
                        cursors[p, q] = rings.load(q, pad, 2 * N, 8000, 1, *cursors.get((p, q), (NULL_HEAD, 0)), 1)
                        ends.add(cursors[p, q])
        assert len(ends) <= 1, "the pairs' cursors drifted apart in tick %d" % t
    for c in chains:
        L._fn(lib, "orc_chain_close", None, [C.c_void_p])(c)
    return {"play": play, "far": far, "out": out}


def room(local, far, prev_far):
    """oracle.loader.tick_room on the device, one far-end per record stream"""
    import torch
    line = torch.cat([prev_far, far], 1).to(torch.int32)
    echo = line[:, N - L.TICK_ECHO_DELAY: 2 * N - L.TICK_ECHO_DELAY] >> 1
    return torch.clamp(local.to(torch.int32) + echo, -32768, 32767).to(torch.int16)


def gpu_bridge(cuda, local, P, stages, platform, on=None, mute=None):
    """the same run on the device: local [T, n, 160] -> dict(play, far, out: [T, n, 160])"""
    import torch
    from wmix_amd.tick import TickBatch
    T, n = local.shape[:2]
    tb = TickBatch.for_platform(platform, n, 1, stages=stages)
    assert tb.pkg == N
    dloc = torch.from_numpy(np.ascontiguousarray(local)).to(cuda)
    play, far, out, zoom = (torch.zeros((T, n, N), dtype=torch.int16, device=cuda) for _ in range(4))
    prev = torch.zeros((n, N), dtype=torch.int16, device=cuda)
    was_on, was_mute = False, None
    for t in range(T):
        now_on = on is None or on(t)
        if now_on != was_on:
            tb.bridge(P if now_on else 0)
            was_on = now_on
        if mute is not None:
            m = [1 if mute(t, p) else 0 for p in range(n)]
            if m != was_mute:
                tb.bridge_mute(m if any(m) else None)
                was_mute = m
        f = tb.play(play[t])
        far[t].copy_(f)
        out[t].copy_(room(dloc[t], f, prev))
        prev = far[t]
        assert tb.record(out[t], zoom[t]) == 2 * N
    res = {"play": play.cpu().numpy(), "far": far.cpu().numpy(), "out": out.cpu().numpy()}
    assert np.array_equal(zoom.cpu().numpy(), res["out"])  # 1 x 8000 -> 1 x 8000: wmix_pcm_zoom copies
    tb.close()
    return res


def talkers(seed, T, n, only=None, alone_for=0):
    """the microphones' local signal [T, n, 160]; for the first `alone_for` ticks participant `only` is the only one in a room
    that is not dead silent"""
    from wmix_amd import synth
    local = synth.conference_inputs(seed, T, 1, n, 8000, 1)[1]
    for k in range(n):  # everybody has something to say from the start (conference_inputs lets the even ones begin silent)
        local[:, k] = np.clip(local[:, k].astype(np.int32) + (2500 * np.sin(0.02 * (1 + 0.13 * k) * np.arange(T * N))).astype(np.int32).reshape(T, N),
                              -32768, 32767)
    if only is not None:
        others = [k for k in range(n) if k != only]
        local[:alone_for, others] = 0
    return local


NS_, AEC_, AGC_, VAD_ = 1, 2, 4, 8


@pytest.mark.parametrize("n_conf,P,platform,stages", [
    (2, 3, "alsa", 0),
    (2, 3, "alsa", AGC_ | VAD_),
    (2, 3, "alsa", NS_ | AEC_ | AGC_ | VAD_),
    (1, 8, "alsa", 0),
    (1, 8, "alsa", NS_ | AEC_ | AGC_ | VAD_),
    (2, 3, "t31", 0),
    (2, 3, "t31", NS_ | AEC_ | AGC_ | VAD_),
])
def test_bridge_tick_against_one_daemon_per_participant(cuda, oracle_port, n_conf, P, platform, stages):
    """Every participant's played package, far-end package and chain output equal those of a daemon of their own whose ring the
    other participants of the conference load their cleaned microphones into.  Through the float NS / AEC the loop is compared
    where the host's powf is the product's (the bar of test_tick_with_the_self_send_receive_test: a tolerance means nothing inside a
    feedback loop)."""
    if stages & (NS_ | AEC_) and not conftest.host_powf_is_the_products():
        pytest.skip("the float path through a feedback loop is bit-exact only against an oracle that links the product's powf")
    T, n, q = 130, n_conf * P, 1
    local = talkers(40 + P, T, n, only=q, alone_for=T if stages == 0 else 0)
    want = bridge_port(oracle_port, local, P, stages, platform)
    got = gpu_bridge(cuda, local, P, stages, platform)
    for k in ("play", "far", "out"):
        assert np.array_equal(got[k], want[k]), (k, np.argwhere((got[k] != want[k]).any(2))[:4])
    assert got["play"].any()
    if stages == 0:
        # nobody hears themself: only q talks (conference 0), so q's loudspeaker stays silent until another participant's
        # microphone has picked q up from ITS loudspeaker and sent it back -- while the others hear q all along
        others = [k for k in range(P) if k != q]
        first_back = int(np.argmax(got["out"][:, others].any((1, 2))))
        assert got["out"][:, others].any() and not got["play"][:first_back + 1, q].any()
        assert all(got["play"][:first_back + 1, k].any() for k in others)
        if n_conf > 1:  # and conferences do not hear each other: nobody talks in conference 1
            assert not got["play"][:, P:].any()


def volume_add(a, b):  # src/wmix.c:1617-1636
    a, b = a.astype(np.int32), b.astype(np.int32)
    return np.where(a == 0, b, np.where(b == 0, a, np.clip(a + b, -32768, 32767))).astype(np.int16)


@pytest.mark.parametrize("platform", ["alsa", "t31"])
def test_a_muted_participant_is_absent_for_exactly_the_packages_of_those_ticks(cuda, oracle_port, platform):
    T, P, n = 130, 3, 6
    local = talkers(77, T, n)
    mute = lambda t, p: p == 1 and 40 <= t < 80  # noqa: E731
    want = bridge_port(oracle_port, local, P, 0, platform, mute=mute)
    got = gpu_bridge(cuda, local, P, 0, platform, mute=mute)
    for k in ("play", "far", "out"):
        assert np.array_equal(got[k], want[k]), k
    # a package loaded in tick t is played `lead` ticks later (the drain of tick t + 1 is VIEW_PLAY_CORRECT behind the cursor)
    lead = 1 + L.PLATFORMS[platform][1] // (2 * N)
    out, play = got["out"], got["play"]
    for t in range(T - lead):
        if 40 <= t < 80:
            assert np.array_equal(play[t + lead, 0], out[t, 2]) and np.array_equal(play[t + lead, 2], out[t, 0]), t
        else:
            assert np.array_equal(play[t + lead, 0], volume_add(out[t, 1], out[t, 2])), t
            assert np.array_equal(play[t + lead, 2], volume_add(out[t, 0], out[t, 1])), t
        assert np.array_equal(play[t + lead, 1], volume_add(out[t, 0], out[t, 2])), t  # the muted one hears the others all along
        assert np.array_equal(play[t + lead, 4], volume_add(out[t, 3], out[t, 5])), t  # the other conference is not touched
    assert out[40:80, 1].any()


@pytest.mark.parametrize("platform", ["alsa", "t31"])
def test_bridge_off_and_on_again_starts_from_a_fresh_cursor(cuda, oracle_port, wmx, platform):
    """On for ticks [0, 50), off, on again from 90: the second run starts from a fresh cursor (head + VIEW_PLAY_CORRECT), so every
    loudspeaker is silent from where the first run's last package ended until the second run's first package comes up.  And the
    bridge and rwTest exclude each other."""
    from wmix_amd.tick import TickBatch
    T, P, n = 130, 3, 3
    local = talkers(91, T, n)
    on = lambda t: t < 50 or t >= 90  # noqa: E731
    want = bridge_port(oracle_port, local, P, 0, platform, on=on)
    got = gpu_bridge(cuda, local, P, 0, platform, on=on)
    for k in ("play", "far", "out"):
        assert np.array_equal(got[k], want[k]), k
    correct = L.PLATFORMS[platform][1]
    lead = 1 + correct // (2 * N)
    # where a cursor-less load of tick 90 lands (src/wmix.c:1666-1673): VIEW_PLAY_CORRECT in front of the head, or at the START of
    # the ring when that is behind its end -- with platform/alsa's 3 200 bytes it is, in tick 90 -- which a continued cursor never does
    head = 91 * 2 * N % 16000
    fresh = head + correct if head + correct < 16000 else 0
    first = 91 + (fresh - head) % 16000 // (2 * N)
    assert got["play"][49 + lead].any() and not got["play"][50 + lead:first].any() and got["play"][first].any()
    whole = gpu_bridge(cuda, local, P, 0, platform)
    assert np.array_equal(whole["play"][:50 + lead], got["play"][:50 + lead])
    tb = TickBatch.for_platform(platform, 6, 1, stages=0)
    tb.bridge(3)
    assert wmx.wmx_tick_rw_test(tb._h, 1) == EINVAL
    tb.bridge(0)
    tb.rw_test(True)
    assert wmx.wmx_tick_bridge(tb._h, 3) == EINVAL
    tb.rw_test(False)
    assert wmx.wmx_tick_bridge(tb._h, 4) == EINVAL and wmx.wmx_tick_bridge(tb._h, 1) == EINVAL  # 4 does not divide 6
    tb.close()
    two = TickBatch.for_platform(platform, 6, 2, stages=0)  # two record streams per group: not a conference of call legs
    assert wmx.wmx_tick_bridge(two._h, 3) == EINVAL
    two.close()


def test_host_tick_with_a_bridge(tmp_path, oracle_port):
    """examples/host_tick.c --bridge P: the same conference from plain C (the room on the host), against one daemon per participant."""
    import json
    import os
    import subprocess
    if not conftest.host_powf_is_the_products():
        pytest.skip("the float path through a feedback loop is bit-exact only against an oracle that links the product's powf")
    exe = os.path.join(conftest.ROOT, "examples", "host_tick")
    assert os.path.exists(exe), "examples/host_tick missing: run __graft_entry__.build()"
    T, P, n = 90, 3, 6
    local = talkers(123, T, n)
    np.zeros((T, n, 1, N), "<i2").tofile(tmp_path / "src.i16")  # no task thread plays anything: the legs hear each other only
    local.astype("<i2").tofile(tmp_path / "local.i16")
    cmd = [exe, str(tmp_path / "src.i16"), str(tmp_path / "local.i16"), str(tmp_path / "out.i16"), str(n), "1", "1", str(T), "8000", "1",
           "--platform", "t31", "--bridge", str(P)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["rc"] == 0 and info["bridge_parties"] == P
    got = np.fromfile(tmp_path / "out.i16", dtype="<i2").reshape(T, 3 * n, N)
    want = bridge_port(oracle_port, local, P, 15, "t31")
    assert want["play"].any()
    assert np.array_equal(got[:, :n], want["play"]) and np.array_equal(got[:, n:2 * n], want["far"]) and np.array_equal(got[:, 2 * n:], want["out"])
    bad = subprocess.run(cmd[:-1] + ["4"], capture_output=True, text=True, timeout=60)  # 4 does not divide 6
    assert bad.returncode == 4 and "wmx_tick_bridge" in bad.stderr
