"""wmx_aecm_process_legs (wmix_amd/csrc/aecm.hip, aecm_legs_kernel): echo control over the ragged rows of a bridge's legs, the kernel
alone.  9 legs (two full workgroups of four waves and one with a single wave) over 60 ticks; per leg one of six call patterns (one row
a tick, 0 .. 3 random, 30 empty ticks first, two a tick, bursts of four, a gap and a burst) and one of four reported delays (0, 20,
200, 500 ms); far rows of speech-like audio, near rows an echo of them under another talker; max_packets 3 and 4, without call lists
and with random ones; rows that are not taken hold random bytes.  Every plane and the four exports behind every tick equal
tests/leg_echo_model.py (one oracle handle per leg) bit for bit; the same far rows and near rows through the dense
wmx_aecm_run_cohorts, one cohort per leg, stepped call by call, give the same rows.  Integers, np.array_equal."""
import functools

import numpy as np
import pytest

from conf_inputs import EINVAL
from leg_echo_inputs import DELAYS, TICKS, patterns, talk
from leg_echo_model import LegsEchoModel
from leg_rows_model import ROW
from leg_seq_model import pack
from leg_stage_inputs import OTHER_LENS, random_list
from legs_kernel_harness import Stage, blobs, odd_address_is_refused, refusals

pytestmark = pytest.mark.gpu

N = 9
ESTATE = -10003
DELAY_OF = [DELAYS[g % len(DELAYS)] for g in range(N)]
RESET_AT, RESET_LEGS = 40, [1, 6]


def make(n=N, delays=None):
    from wmix_amd.aecm import AecmBatch
    b = AecmBatch.create_legs(n)
    for g, d in enumerate(delays or []):
        b.set_delay_legs(d, [g])
    return b


def cohort_handle(n=6, chn=1, freq=8000, interval_ms=20):
    from wmix_amd.aecm import AecmBatch
    return AecmBatch(n, chn, freq, interval_ms)


STAGE = Stage(make, (1, ROW), None, "wmx_aecm_process_legs", b"wmx_aecm_create_legs", (None, 0))


@functools.lru_cache(maxsize=None)
def script(k_slots, with_lists, pad=8, ticks=TICKS):
    """-> per tick (plane int16 [N, k_slots, 160 + pad], lens uint32 [N, k_slots], lists or None), far int16 [ticks, N, 160]"""
    rng = np.random.default_rng(1000 + 10 * k_slots + int(with_lists))
    pats = list(patterns().values())
    far = np.stack([talk(ticks * ROW, 100 + g).reshape(ticks, ROW) for g in range(N)], axis=1)
    src = []
    for g in range(N):
        line = far[:, g].reshape(-1).astype(np.float64)
        echo = np.concatenate([np.zeros(517), 0.3 * line])[:line.size]
        other = talk(4 * ticks * ROW, 200 + g, amp=800).astype(np.float64)
        src.append(np.clip(np.rint(np.resize(echo, other.size) + other), -32768, 32767).astype(np.int16))
    at, out = [0] * N, []
    for t in range(ticks):
        plane = rng.integers(-32768, 32768, size=(N, k_slots, ROW + pad)).astype(np.int16)  # rows not taken hold anything
        lens = rng.choice(OTHER_LENS, size=(N, k_slots)).astype(np.uint32)
        for g in range(N):
            for k in rng.permutation(k_slots)[:min(pats[g % len(pats)][t], k_slots)]:
                lens[g, k] = 320
                plane[g, k, :ROW] = src[g][at[g]:at[g] + ROW]
                at[g] += ROW
        out.append((plane, lens, [random_list(rng, lens[g], k_slots) for g in range(N)] if with_lists else None))
    return out, far


@functools.lru_cache(maxsize=None)
def model_run(k_slots, with_lists, pad=8, reset=False):
    """the model over the script -> per tick (plane, the four exports), per tick and leg the slots fed"""
    from oracle import loader
    ticks, far = script(k_slots, with_lists, pad)
    m = LegsEchoModel(loader.port(), N, DELAY_OF)
    out, fed = [], []
    for t, (plane, lens, lists) in enumerate(ticks):
        if reset and t == RESET_AT:
            m.reset(RESET_LEGS)
        p = plane.copy()
        fed.append(m.tick(p, lens, lists))
        m.far(far[t])
        out.append((p, m.export()))
    m.close()
    return out, fed


def upload(cuda, plane, lens, lists, offset=0):
    import torch
    buf = torch.zeros(plane.size + offset + 8, dtype=torch.int16, device=cuda)
    d = buf[offset:offset + plane.size].view(plane.shape)
    d.copy_(torch.from_numpy(plane))
    d_lens = torch.from_numpy(lens.view(np.int32)).to(cuda)
    d_calls = None if lists is None else torch.from_numpy(np.array([pack(c) for c in lists], np.uint32).view(np.int32)).to(cuda)
    return d, d_lens, d_calls


def run(cuda, ticks, far, batch, offset=0, split=False, before=None):
    """the kernel over the script -> per tick (the plane as it left it, the four exports).  split: a rows-only call, then a far-only
    one; before: {tick: f(batch)} run in front of that tick"""
    import torch
    got = []
    for t, (plane, lens, lists) in enumerate(ticks):
        if before and t in before:
            before[t](batch)
        d, d_lens, d_calls = upload(cuda, plane, lens, lists, offset)
        d_far = torch.from_numpy(far[t]).to(cuda)
        if split:
            batch.process_legs(d[:, :, :ROW], d_lens, d_calls)
            batch.process_legs(None, None, None, d_far)
        else:
            batch.process_legs(d[:, :, :ROW], d_lens, d_calls, d_far)
        got.append((d.cpu().numpy(), batch.export_legs()))
    return got


def same(got, want, legs=None):
    for t, ((p, e), (wp, we)) in enumerate(zip(got, want)):
        sel = slice(None) if legs is None else legs
        assert np.array_equal(p[sel], wp[sel]), ("plane, tick", t, "legs", np.flatnonzero((p != wp).any(axis=(1, 2))))
        for name, a, b in zip(("startup", "far_ms", "known_delay", "delay_blocks"), e, we):
            assert np.array_equal(a[sel], b[sel]), (name, "tick", t, a, b)


def dense_rows(cuda, wmx, ticks, far, fed):
    """the same far rows and near rows through wmx_aecm_run_cohorts on a handle with one cohort per leg, call by call: per tick the
    r-th row of every leg that has one (the others' cohorts switched off), mode 2; then every leg's far row, mode 1
    -> per tick the plane with the rows taken replaced"""
    import torch
    from wmix_amd.aecm import AecmBatch
    dense = AecmBatch(N, 1, 8000, 20, n_cohorts=N)
    for g in range(1, N):
        dense.reset_streams([g], cohort=g)
    stream = torch.cuda.current_stream().cuda_stream
    delays, codes, out = np.array(DELAY_OF, np.int32), np.zeros(N, np.int32), []
    for t, (plane, _, _) in enumerate(ticks):
        p = plane.copy()
        for r in range(max(len(f) for f in fed[t])):
            on = np.array([len(f) > r for f in fed[t]], np.uint8)
            rows = np.stack([plane[g, fed[t][g][r], :ROW] if on[g] else np.zeros(ROW, np.int16) for g in range(N)])
            d = torch.from_numpy(rows).to(cuda)
            assert wmx.wmx_aecm_run_cohorts(dense._h, 2, None, 0, 0, d.data_ptr(), d.data_ptr(), 1, ROW, ROW, delays.ctypes.data,
                                            on.ctypes.data, codes.ctypes.data, stream) == 0
            res = d.cpu().numpy()
            for g in np.flatnonzero(on):
                p[g, fed[t][g][r], :ROW] = res[g]
        d_far = torch.from_numpy(far[t]).to(cuda)
        assert wmx.wmx_aecm_run_cohorts(dense._h, 1, d_far.data_ptr(), ROW, ROW, None, None, 1, 0, 0, delays.ctypes.data, None,
                                        codes.ctypes.data, stream) == 0
        out.append(p)
    torch.cuda.synchronize()
    dense.close()
    return out


@pytest.mark.parametrize("k_slots,with_lists", [(3, False), (4, False), (3, True), (4, True)])
def test_ragged_rows_equal_the_model_and_the_dense_call(cuda, wmx, oracle_port, k_slots, with_lists):
    ticks, far = script(k_slots, with_lists)
    want, fed = model_run(k_slots, with_lists)
    b = make(N, DELAY_OF)
    got = run(cuda, ticks, far, b)
    same(got, want)
    # the script reaches what it is for: legs past their start-up whose rows the canceller rewrites, a first delay estimate, a known
    # delay that has moved, bursts of four rows where there are four slots, and calls that add nothing where there are lists
    startup, _, known, blocks = got[-1][1]
    assert (startup == 0).sum() >= N - 1 and (blocks >= 0).any() and (known > 0).any()
    changed = sum(int((got[t][0][g, k, :ROW] != ticks[t][0][g, k, :ROW]).any()) for t in range(TICKS) for g in range(N) for k in fed[t][g])
    assert changed > 100 and max(len(f) for ft in fed for f in ft) == k_slots
    if with_lists:
        assert any(("S", None) in c for _, _, ls in ticks for c in ls)
    for t, p in enumerate(dense_rows(cuda, wmx, ticks, far, fed)):
        assert np.array_equal(p, got[t][0]), ("dense, tick", t)
    b.close()


def test_far_only_and_rows_only_compose_and_the_plane_one_sample_in_is_the_same(cuda, oracle_port):
    ticks, far = script(3, True, pad=1)  # rows of 161 samples: every other row is off the 4-byte grid as well
    want, _ = model_run(3, True, pad=1)
    b0, b1 = make(N, DELAY_OF), make(N, DELAY_OF)
    same(run(cuda, ticks[:30], far, b0), want)
    same(run(cuda, ticks[:30], far, b1, offset=1, split=True), want)
    assert all(np.array_equal(a, c) for a, c in zip(blobs(b0), blobs(b1)))
    b0.close()
    b1.close()


def test_an_odd_address_is_refused(cuda, wmx):
    ticks, far = script(3, True, pad=1)
    b = make(N, DELAY_OF)
    run(cuda, ticks[:2], far, b)
    odd_address_is_refused(STAGE, cuda, wmx, b, ticks[0][0], ticks[0][1])
    b.close()


def test_refusals_launch_nothing(cuda, wmx):
    import torch
    d_far = torch.zeros((6, ROW), dtype=torch.int16, device=cuda)
    # a handle that was not made by wmx_aecm_create_legs
    refusals(STAGE, cuda, wmx, [cohort_handle(), cohort_handle(6, 1, 16000, 10), cohort_handle(6, 2, 8000, 20)], c_extras=(d_far.data_ptr(), ROW))
    b = make(6)
    plane = np.zeros((6, 3, ROW), np.int16)
    d, d_lens = torch.from_numpy(plane).to(cuda), torch.full((6, 3), 320, dtype=torch.int32, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    b.process_legs(d.clone(), d_lens, None, d_far)
    before, entry = blobs(b), wmx.wmx_aecm_process_legs
    rows = (d.data_ptr(), 3 * ROW, ROW, 3, d_lens.data_ptr(), None)
    for args, message in [(rows + (d_far.data_ptr() + 1, ROW), b"2-byte"), (rows + (d_far.data_ptr(), ROW - 1), b"overlap"),
                          ((None, 0, 0, 1, None, None, None, 0), b"neither"), ((None, 0, 0, 1, None, None, d_far.data_ptr() + 1, ROW), b"2-byte")]:
        assert entry(b._h, *args, stream) == EINVAL and message in wmx.wmx_last_error(), (message, wmx.wmx_last_error())
    # a refused delay changes nothing; the cohort entry points have nothing to work on
    for bad in (-1, 501):
        assert wmx.wmx_aecm_set_delay_legs(b._h, None, 0, bad, stream) == EINVAL
    codes, delays = np.zeros(1, np.int32), np.zeros(1, np.int32)
    assert wmx.wmx_aecm_run(b._h, 3, d_far.data_ptr(), ROW, d.data_ptr(), d.data_ptr(), 1, 3 * ROW, ROW, 0, stream) == ESTATE
    assert b"wmx_aecm_create_legs" in wmx.wmx_last_error()
    assert wmx.wmx_aecm_run_cohorts(b._h, 3, d_far.data_ptr(), ROW, 0, d.data_ptr(), d.data_ptr(), 1, 3 * ROW, ROW, delays.ctypes.data, None,
                                    codes.ctypes.data, stream) == ESTATE
    assert wmx.wmx_aecm_cohorts(b._h) == ESTATE and wmx.wmx_aecm_reset_cohort(b._h, 0, stream) == ESTATE
    assert wmx.wmx_aecm_cohort_state_bytes(b._h) == ESTATE and wmx.wmx_aecm_live_cohorts(b._h) == ESTATE
    torch.cuda.synchronize()
    assert all(np.array_equal(a, c) for a, c in zip(before, blobs(b))) and not d.cpu().numpy().any()
    b.close()


def test_a_leg_switched_off_gets_neither_rows_nor_far(cuda):
    ticks, far = script(3, False)
    b, off = make(N, DELAY_OF), [2, 4, 8]
    fresh = blobs(b)
    mask = np.ones(N, bool)
    mask[off] = False
    b.set_active(mask)
    t = 5  # every leg but the one that starts late has a row
    got = run(cuda, ticks[t:t + 1], far[t:], b)[0][0]
    after = blobs(b)
    for g in range(N):
        has_rows = bool((ticks[t][1][g] == 320).any())
        assert np.array_equal(after[g], fresh[g]) == (g in off), g
        assert np.array_equal(got[g], ticks[t][0][g]) or (has_rows and g not in off), g
    b.set_active(None)
    run(cuda, ticks[t:t + 1], far[t:], b)
    assert all(not np.array_equal(a, c) for a, c in zip(blobs(b), fresh))
    b.close()


def test_reset_streams_mid_script_is_a_fresh_leg_with_its_delay_kept(cuda, oracle_port):
    ticks, far = script(3, False)
    want, _ = model_run(3, False, reset=True)
    b = make(N, DELAY_OF)
    same(run(cuda, ticks, far, b, before={RESET_AT: lambda x: x.reset_streams(RESET_LEGS)}), want)
    b.close()


def test_a_leg_exported_at_tick_30_continues_in_another_handle(cuda, oracle_port):
    ticks, far = script(3, False)
    want, _ = model_run(3, False)
    a, b, src, dst = make(N, DELAY_OF), make(N), 3, 5
    run(cuda, ticks[:30], far, a)
    blob = a.export_stream(src)
    assert blob.size == a.export_stream(0).size > 45000  # near state, far-end slab, control plane and delay
    b.import_stream(dst, blob)
    moved, moved_far = [], far.copy()
    for plane, lens, _ in ticks[30:]:
        p, ln = plane.copy(), lens.copy()
        p[dst], ln[dst] = plane[src], lens[src]
        moved.append((p, ln, None))
    moved_far[:, dst] = far[:, src]
    got = run(cuda, moved, moved_far[30:], b)
    for t, (p, e) in enumerate(got):
        wp, we = want[30 + t]
        assert np.array_equal(p[dst], wp[src]), ("tick", 30 + t)
        assert all(x[dst] == y[src] for x, y in zip(e, we)), ("exports, tick", 30 + t)
    a.close()
    b.close()
