"""Talker selection on the device (wmx_mix_select_speakers / _conf in wmix_amd/csrc/mix.hip, wmx_tick_bridge_speakers in tick.hip):
the kernel against the numpy model of the rule (tests/speakers_model.py, which tests/test_speakers_host.py ties to speakers.h), the
mask it writes fed to the bridge load against one reference mixer per leg (the helpers of tests/test_bridge_gpu.py and
tests/test_bridge_ragged_gpu.py), and its place in the tick pinned by a second tick that is told the same mask from outside.
Integers throughout: np.array_equal."""
import json
import os
import subprocess

import numpy as np
import pytest

from conf_inputs import EINVAL, NULL_HEAD
import conftest
from leg_oracle_model import OracleRings
from speakers_model import SpeakersModel, row_of_level, uniform_layout
from test_bridge_gpu import N, oracle_minus, room, talkers
from test_bridge_ragged_gpu import oracle_minus_conf

pytestmark = pytest.mark.gpu

NS_, AEC_, AGC_, VAD_ = 1, 2, 4, 8


# ---------------------------------------------------------------- crafted levels
def crafted_ticks(confs, n, n_el):
    """8 ticks of levels by ring for the conferences `confs` (lists of rings, list order = position), with the parameters of each tick:
    silence with floor 0; a row of all -32768; that talker falling silent and being held; a full tie with no hold (shift 0); a tie of two
    at the top; an envelope that equals the floor; the loudest leg muted by the host; max_speakers >= the size with shift 31."""
    rng = np.random.default_rng(7 + n + n_el)
    A = 20 * n_el
    live = [c for c in confs if len(c) >= 2]
    ticks = []

    def levels(fn):
        lv = np.zeros(n, np.int64)
        for k, mem in enumerate(live):
            for p, r in enumerate(mem):
                lv[r] = fn(k, p, len(mem))
        return lv

    quiet = lambda: int(rng.integers(A, 2 * A))  # noqa: E731
    ticks.append(dict(levels=levels(lambda k, p, P: 0), max=2, floor=0, shift=3))
    ticks.append(dict(levels=levels(lambda k, p, P: 32768 * n_el if p == k % P else quiet()), max=1, floor=1, shift=3))
    ticks.append(dict(levels=levels(lambda k, p, P: 0 if p == k % P else quiet()), max=1, floor=1, shift=3))
    ticks.append(dict(levels=levels(lambda k, p, P: 3 * A), max=2, floor=0, shift=0))
    ticks.append(dict(levels=levels(lambda k, p, P: 5 * A if p in (0, P - 1) else quiet()), max=1, floor=0, shift=3))
    held = 5 * A - (5 * A >> 3)
    ticks.append(dict(levels=levels(lambda k, p, P: held - 1 if p == 1 else 0), max=32, floor=held, shift=3))
    mute = np.zeros(n, np.uint8)
    for k, mem in enumerate(live):
        mute[mem[(k + 1) % len(mem)]] = 1
    ticks.append(dict(levels=levels(lambda k, p, P: 50 * A if p == (k + 1) % P else quiet()), max=1, floor=0, shift=3, mute=mute))
    ticks.append(dict(levels=levels(lambda k, p, P: int(rng.integers(0, A))), max=32, floor=0, shift=31))
    return ticks


def rows_for(levels, n_el, row, rng):
    """[n, row] int16: ring r's first n_el elements have level levels[r]; what lies behind them (the look-ahead frame, the padding of an
    odd stride) is loud and must not be counted"""
    rows = np.full((len(levels), row), 30000, np.int16)
    for r, lv in enumerate(levels):
        rows[r, :n_el] = row_of_level(int(lv), n_el, rng)
    return rows


def check_against_model(model, mb, out, want, tag):
    sp, mo = want
    got_sp, got_env = mb.export_speakers()
    assert np.array_equal(out.cpu().numpy(), mo), (tag, "mute_out")
    assert np.array_equal(got_sp, sp), (tag, "speaking")
    assert np.array_equal(got_env, model.env), (tag, "env", np.flatnonzero(got_env != model.env)[:8])


# ---------------------------------------------------------------- 1. the uniform form
#         P   ring        n_el  padding of the row stride
UNIFORM = [(2, (1, 8000), 160, 0), (3, (1, 8000), 160, 0), (5, (1, 8000), 160, 0), (32, (1, 8000), 160, 0),
           (3, (2, 16000), 640, 1)]  # 20 ms of 2 x 16000; the stride is odd, so the rows start at every offset from a 16-byte boundary


@pytest.mark.parametrize("P,ring,n_el,odd", UNIFORM)
def test_select_speakers_against_the_model_and_the_load_against_one_mixer_per_leg(cuda, oracle_port, P, ring, n_el, odd):
    import torch
    from wmix_amd.mix import MixBatch
    ring_chn, ring_freq = ring
    n_conf, sbytes = 3, 2 * n_el
    n = n_conf * P
    row = n_el + ring_chn + odd
    layout = uniform_layout(n, P)
    ticks = crafted_ticks(layout, n, n_el)
    rng = np.random.default_rng(P)
    model = SpeakersModel(n)
    orc = OracleRings(oracle_port, n, ring_chn, ring_freq, 0, 1)
    mb = MixBatch(n, ring_chn, ring_freq)
    cur_o = cur_d = (NULL_HEAD, 0)
    seen = []
    for t, tk in enumerate(ticks):
        src = rows_for(tk["levels"], n_el, row, rng).reshape(n_conf, P, row)
        mute = tk.get("mute")
        want = model.step(layout, src.reshape(n, row)[:, :n_el], tk["max"], tk["floor"], tk["shift"], mute)
        seen.append(want[0].reshape(n_conf, P))
        d = torch.from_numpy(src).to(cuda)
        assert d.stride(1) == row and (odd == 0 or row % 2 == 1)
        dm = torch.from_numpy(mute).to(cuda) if mute is not None else None
        out = mb.select_speakers(d, P, sbytes, tk["max"], tk["floor"], tk["shift"], mute=dm)
        check_against_model(model, mb, out, want, ("tick", t))
        cur_d = mb.load_minus(d, P, sbytes, ring_freq, ring_chn, mute=out, head=cur_d[0], tick=cur_d[1])
        cur_o = oracle_minus(orc, P, src, sbytes, ring_freq, ring_chn, 1, cur_o, want[1])
        assert cur_d == cur_o, t
    for k in range(n):
        assert np.array_equal(mb.export(k)[0], orc.ring(k)), ("ring", k)
    mb.close()
    # ---- what the crafted ticks were for, on the model alone
    first = [1] * min(2, P) + [0] * (P - min(2, P))
    assert all(seen[0][c].tolist() == first for c in range(n_conf))                      # silence, floor 0: the first two of the list
    for c in range(n_conf):
        assert seen[1][c].tolist() == [int(p == c % P) for p in range(P)]                # the row of -32768
        assert seen[2][c].tolist() == seen[1][c].tolist()                                # silent now, held above the others
        assert seen[3][c].tolist() == first                                              # a full tie, nothing held
        assert seen[4][c].tolist() == [1] + [0] * (P - 1)                                # 0 and P - 1 tie at the top: the earlier one
        assert seen[5][c][0] == 1 and (P == 2 or seen[5][c][1] == 0)                     # env' == floor speaks, floor - 1 does not
        assert seen[6][c][(c + 1) % P] == 0 and seen[6][c].sum() == 1                    # the loudest is muted by the host
        assert seen[7][c].all()                                                          # max_speakers >= the size


# ---------------------------------------------------------------- 2. the layout form
def descending_layout():
    """sizes 2, 1, 7, 32, 0, 4 over 52 rings, six of them idle; every member list is descending and not consecutive"""
    idle = [50, 30, 17, 9, 4, 0]
    pool = np.random.default_rng(3).permutation([r for r in range(52) if r not in idle]).tolist()
    layout = []
    for size in (2, 1, 7, 32, 0, 4):
        layout.append(sorted((pool.pop() for _ in range(size)), reverse=True))
    assert not pool and all(any(a - b > 1 for a, b in zip(m, m[1:])) for m in layout if len(m) > 1)
    return layout, idle


def test_select_speakers_conf_over_a_layout_that_changes(cuda, oracle_port):
    import torch
    from wmix_amd.mix import MixBatch
    n, n_el, row = 52, 160, 161
    layout, idle = descending_layout()
    ticks = crafted_ticks(layout, n, n_el)
    rng = np.random.default_rng(11)
    model = SpeakersModel(n)
    orc = OracleRings(oracle_port, n, 1, 8000, 0, 1)
    mb = MixBatch(n, 1, 8000)
    mb.set_conferences(layout)
    heads, tks = [NULL_HEAD] * 6, [0] * 6

    def one(t, tk, lay):
        nonlocal heads, tks
        src = rows_for(tk["levels"], n_el, row, rng)
        mute = tk.get("mute")
        want = model.step(lay, src[:, :n_el], tk["max"], tk["floor"], tk["shift"], mute)
        d = torch.from_numpy(src).to(cuda)
        dm = torch.from_numpy(mute).to(cuda) if mute is not None else None
        out = mb.select_speakers_conf(d, 320, tk["max"], tk["floor"], tk["shift"], mute=dm)
        check_against_model(model, mb, out, want, ("tick", t))
        got = mb.load_minus_conf(d, 320, 8000, 1, mute=out, head=heads, tick=tks)
        heads, tks = oracle_minus_conf(orc, lay, src, 320, 8000, 1, 1, heads, tks, want[1])
        assert got[0].tolist() == heads and got[1].tolist() == tks, t
        return want[0]

    seen = [one(t, tk, layout) for t, tk in enumerate(ticks)]
    seven = layout[2]
    assert seven[0] > seven[6] and seen[4][seven[0]] == 1 and seen[4][seven[6]] == 0  # the tie inside the 7: the earlier position, the HIGHER ring
    assert not any(s[layout[1] + idle].any() for s in seen) and not model.env[layout[1] + idle].any()
    # ---- one leg leaves the 7, an idle ring joins the 4: the envelopes of the rings that stay are carried, the leaver's is left alone
    left, joined = seven[3], idle[2]
    after = [list(m) for m in layout]
    after[2].remove(left)
    after[5].insert(1, joined)
    mb.set_conferences(after)
    before = model.env.copy()
    assert before[left] > 0
    lv = np.zeros(n, np.int64)
    lv[after[2][0]] = 1  # nearly silent: every envelope of the 7 is its held value
    lv[left] = 123456    # the leaver's row is not looked at
    seen.append(one(8, dict(levels=lv, max=3, floor=1, shift=2), after))
    assert model.env[left] == before[left] and seen[-1][left] == 0
    stay = [r for r in after[2] + after[3] + after[0]]
    assert all(model.env[r] == max(lv[r], before[r] - (before[r] >> 2)) for r in stay) and model.env[stay].any()
    for k in range(n):
        assert np.array_equal(mb.export(k)[0], orc.ring(k)), ("ring", k)
    # reset: the listed rings only, then every ring
    mb.reset_speakers([after[2][0], left])
    model.reset([after[2][0], left])
    assert np.array_equal(mb.export_speakers()[1], model.env) and model.env.any()
    mb.reset_speakers()
    assert not mb.export_speakers()[1].any()
    mb.close()


# ---------------------------------------------------------------- 3. the tick, in lockstep with a tick that is told the mask
def lockstep_inputs(seed, T, n):
    """talkers whose loudness order changes every three ticks"""
    local = talkers(seed, T, n).astype(np.int32)
    for t in range(T):
        for k in range(n):
            local[t, k] = local[t, k] * ((3 * k + 5 * (t // 3)) % 7) // 6
    return np.clip(local, -32768, 32767).astype(np.int16)


class TickRun:
    """one TickBatch stepped a tick at a time over local [T, n, 160] (the room of tests/test_bridge_gpu.py on the device)"""

    def __init__(self, cuda, local, stages, platform, form):
        import torch
        from wmix_amd.tick import TickBatch
        self.torch, self.n = torch, local.shape[1]
        self.tb = TickBatch.for_platform(platform, self.n, 1, stages=stages)
        self.dloc = torch.from_numpy(np.ascontiguousarray(local)).to(cuda)
        self.prev = torch.zeros((self.n, N), dtype=torch.int16, device=cuda)
        self.cuda = cuda
        if form is not None:
            self.bridge_on(form)

    def bridge_on(self, form):
        if isinstance(form, int):
            self.tb.bridge(form)
        else:
            self.tb.bridge_conferences(form)

    def step(self, t):
        """-> (play, out) of tick t as numpy [n, 160]"""
        torch = self.torch
        play = torch.zeros((self.n, N), dtype=torch.int16, device=self.cuda)
        f = self.tb.play(play)
        out = room(self.dloc[t], f, self.prev)
        self.prev = f.clone()
        assert self.tb.record(out) == 0  # no zoom buffer
        return play.cpu().numpy(), out.cpu().numpy()

    def rings(self):
        from wmix_amd._lib import lib
        mix = lib().wmx_tick_mix(self.tb._h)
        size = lib().wmx_mix_ring_bytes(mix) // 2
        res = []
        for k in range(self.n):
            ring = np.zeros(size, np.int16)
            assert lib().wmx_mix_export(mix, k, ring.ctypes.data, None, None) == 0
            res.append(ring)
        return np.stack(res)


def form_layout(form, n):
    return uniform_layout(n, form) if isinstance(form, int) else form


FORMS = {"bridge4": (8, 4), "ragged": (11, [[0, 1, 2], [3, 4], [5, 6, 7, 8, 9]])}  # leg 10 of the ragged one is idle
FLOOR = 20000


def speakers_run(cuda, local, stages, platform, form, mx=2, floor=FLOOR, shift=3):
    """the tick with selection on, alone: -> (play, out: [T, n, 160], speaking: [T, n])"""
    a = TickRun(cuda, local, stages, platform, form)
    a.tb.bridge_speakers(mx, floor, shift)
    play, out, speaking = [], [], []
    for t in range(local.shape[0]):
        p, o = a.step(t)
        play.append(p), out.append(o), speaking.append(a.tb.bridge_speaking()[0])
    a.tb.close()
    return np.stack(play), np.stack(out), np.stack(speaking)


@pytest.mark.parametrize("stages", [0, NS_ | AEC_ | AGC_ | VAD_])
@pytest.mark.parametrize("name", sorted(FORMS))
def test_tick_with_selection_equals_a_tick_that_is_told_the_same_mask(cuda, name, stages):
    """A selects on the device; B never has selection on and is given A's choice of this tick as its host mute before its own record
    side runs.  Equal play and record outputs at every tick say that A's load used exactly that mask and that the selection looked at
    the chain's OUTPUT of this tick: the model applied to A's record output gives the same speakers."""
    n, form = FORMS[name]
    T = 12
    local = lockstep_inputs(60 + n, T, n)
    layout = form_layout(form, n)
    a, b = (TickRun(cuda, local, stages, "t31", form) for _ in range(2))
    a.tb.bridge_speakers(2, FLOOR, 3)
    model = SpeakersModel(n)
    chosen = []
    for t in range(T):
        pa, oa = a.step(t)
        speaking, env = a.tb.bridge_speaking()
        want = model.step(layout, oa, 2, FLOOR, 3)
        assert np.array_equal(speaking, want[0]) and np.array_equal(env, model.env), t
        b.tb.bridge_mute(1 - speaking)
        pb, ob = b.step(t)
        assert np.array_equal(pa, pb) and np.array_equal(oa, ob), t
        chosen.append(speaking)
    assert np.array_equal(a.rings(), b.rings())
    chosen = np.stack(chosen)
    for mem in layout:
        assert (chosen[:, mem].sum(1) <= 2).all() and chosen[:, mem].any()
    assert len({tuple(c) for c in chosen}) >= 3 and pa.any()  # the choice moves, and what was chosen is played
    if name == "ragged":
        assert not chosen[:, 10].any()
    a.tb.close()
    b.tb.close()


# ---------------------------------------------------------------- 4. off is today
@pytest.mark.parametrize("name", sorted(FORMS))
def test_selection_off_or_unbounded_is_the_tick_without_it(cuda, name):
    n, form = FORMS[name]
    T = 8
    local = lockstep_inputs(70 + n, T, n)
    stages = AGC_ | VAD_
    was_on, unbounded, never = (TickRun(cuda, local, stages, "t31", None) for _ in range(3))
    was_on.tb.bridge_speakers(1, FLOOR, 3)  # on while no bridge is: nothing to select for
    for t in range(2):
        res = [r.step(t) for r in (was_on, unbounded, never)]
        assert all(np.array_equal(res[0][1], r[1]) for r in res[1:])
    was_on.tb.bridge_speakers(0, 0, 0)
    unbounded.tb.bridge_speakers(32, 0, 3)
    for r in (was_on, unbounded, never):
        r.bridge_on(form)
    for t in range(2, T):
        res = [r.step(t) for r in (was_on, unbounded, never)]
        for other in res[:2]:
            assert np.array_equal(other[0], res[2][0]) and np.array_equal(other[1], res[2][1]), t
    want = never.rings()
    assert want.any() and np.array_equal(was_on.rings(), want) and np.array_equal(unbounded.rings(), want)
    assert not was_on.tb.bridge_speaking()[1].any()  # it never ran
    live = sorted(r for mem in form_layout(form, n) for r in mem)
    assert unbounded.tb.bridge_speaking()[0][live].all()
    for r in (was_on, unbounded, never):
        r.tb.close()


# ---------------------------------------------------------------- 5. refusals
def test_refusals_leave_envelopes_and_rings_alone(cuda, wmx):
    import torch
    from wmix_amd.mix import MixBatch
    from wmix_amd.tick import TickBatch
    n, per = 12, 160
    mb = MixBatch(n, 1, 8000)
    rng = np.random.default_rng(9)
    src = torch.from_numpy(rng.integers(-20000, 20000, size=(4, 3, per + 1), dtype=np.int16)).to(cuda)
    big = torch.zeros(300000, dtype=torch.int16, device=cuda)
    out = mb.select_speakers(src, 3, 320, 1, 0, 3)
    mb.load_minus(src, 3, 320, 8000, 1, mute=out)
    sp0, env0 = mb.export_speakers()
    rings0 = [mb.export(k)[0] for k in range(n)]
    assert env0.all() and sp0.sum() == 4 and any(r.any() for r in rings0)
    keep = out.clone()
    stream = torch.cuda.current_stream().cuda_stream

    def uniform(parties=3, sbytes=320, mx=1, shift=3, src_ptr=src.data_ptr(), out_ptr=out.data_ptr(), cs=3 * (per + 1), ss=per + 1):
        return wmx.wmx_mix_select_speakers(mb._h, parties, src_ptr, sbytes, cs, ss, None, mx, 0, shift, out_ptr, stream)

    def conf(sbytes=320, mx=1, shift=3, out_ptr=out.data_ptr()):
        return wmx.wmx_mix_select_speakers_conf(mb._h, src.data_ptr(), sbytes, per + 1, None, mx, 0, shift, out_ptr, stream)

    for mx in (0, 33, -1):
        assert uniform(mx=mx) == EINVAL and b"max_speakers" in wmx.wmx_last_error(), mx
    for shift in (-1, 32):
        assert uniform(shift=shift) == EINVAL and b"decay_shift" in wmx.wmx_last_error(), shift
    assert uniform(out_ptr=None) == EINVAL
    for parties in (1, 33, 5, 8, -2):  # 5 and 8 do not divide 12
        assert uniform(parties=parties) == EINVAL and b"parties" in wmx.wmx_last_error(), parties
    assert uniform(sbytes=2 * 131072, src_ptr=big.data_ptr(), cs=0, ss=0) == EINVAL and b"overflow" in wmx.wmx_last_error()
    assert conf() == EINVAL and b"layout" in wmx.wmx_last_error()  # no layout yet
    mb.set_conferences([[3, 1], [7, 5, 9]])
    for bad in (dict(mx=0), dict(mx=33), dict(shift=-1), dict(shift=32), dict(out_ptr=None), dict(sbytes=2 * 131072)):
        assert conf(**bad) == EINVAL, bad
    bad_idx = np.array([0, 12], np.int32)
    assert wmx.wmx_mix_reset_speakers(mb._h, bad_idx.ctypes.data, 2, stream) == EINVAL
    sp1, env1 = mb.export_speakers()
    assert np.array_equal(sp1, sp0) and np.array_equal(env1, env0) and torch.equal(out, keep)
    for k in range(n):
        assert np.array_equal(mb.export(k)[0], rings0[k]), k
    mb.close()
    tb = TickBatch.for_platform("t31", 6, 1, stages=0)
    for mx, shift in ((-1, 3), (33, 3), (2, -1), (2, 32)):
        assert wmx.wmx_tick_bridge_speakers(tb._h, mx, 0, shift) == EINVAL, (mx, shift)
    assert wmx.wmx_tick_bridge_speakers(tb._h, 32, 0xFFFFFFFF, 31) == 0 and wmx.wmx_tick_bridge_speakers(tb._h, 0, 0, 0) == 0
    sp, env = tb.bridge_speaking()
    assert not sp.any() and not env.any()
    tb.close()


# ---------------------------------------------------------------- 6. the C host
def test_host_tick_with_speakers(tmp_path, cuda):
    """examples/host_tick.c --bridge-sizes 3,2,5 --speakers 2,<floor>: the ragged run of the lockstep test from plain C (the room on the
    host), against the same run through the Python mirror"""
    exe = os.path.join(conftest.ROOT, "examples", "host_tick")
    assert os.path.exists(exe), "examples/host_tick missing: run __graft_entry__.build()"
    n, form = FORMS["ragged"]
    T = 12
    local = lockstep_inputs(60 + n, T, n)
    np.zeros((T, n, 1, N), "<i2").tofile(tmp_path / "src.i16")  # no task thread plays anything: the legs hear each other only
    local.astype("<i2").tofile(tmp_path / "local.i16")
    cmd = [exe, str(tmp_path / "src.i16"), str(tmp_path / "local.i16"), str(tmp_path / "out.i16"), str(n), "1", "1", str(T), "8000", "1",
           "--platform", "t31", "--bridge-sizes", "3,2,5", "--speakers"]
    r = subprocess.run(cmd + ["2,%d" % FLOOR], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["rc"] == 0 and info["bridge_sizes"] == [3, 2, 5] and info["speakers"] == 2 and info["speakers_floor"] == FLOOR
    got = np.fromfile(tmp_path / "out.i16", dtype="<i2").reshape(T, 3 * n, N)
    play, out, speaking = speakers_run(cuda, local, NS_ | AEC_ | AGC_ | VAD_, "t31", form)
    assert play.any() and np.array_equal(got[:, :n], play) and np.array_equal(got[:, 2 * n:], out)
    assert info["speaking"] == int(speaking[-1].sum()) and 0 < info["speaking"] <= 6
    # the defaults: floor 0, shift 3
    r = subprocess.run(cmd + ["2"], capture_output=True, text=True, timeout=600)
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and info["speakers"] == 2 and info["speakers_floor"] == 0 and info["speakers_shift"] == 3 and info["speaking"] == 6
    for bad, code, word in (("33", 4, "wmx_tick_bridge_speakers"), ("2,5,32", 4, "wmx_tick_bridge_speakers"), ("x", 2, "--speakers"), ("2,x", 2, "--speakers")):
        b = subprocess.run(cmd + [bad], capture_output=True, text=True, timeout=60)
        assert b.returncode == code and word in b.stderr, bad
    b = subprocess.run(cmd[:-3] + ["--speakers", "2"], capture_output=True, text=True, timeout=60)  # without a bridge
    assert b.returncode == 2 and "--bridge" in b.stderr
