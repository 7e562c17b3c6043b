"""wmx_nsx_process_legs (wmix_amd/csrc/nsx.hip): the fixed-point noise suppressor over the ragged rows of a bridge's legs, the kernel
alone.  37 legs (the last workgroup is part full) over 40 ticks of seeded random rows: 0 .. max_packets rows per leg and tick, lens
other than 0 and 320 among them, without call lists and with random ones.  Every row taken equals tests/leg_denoise_model.py (the
oracle over the leg's ordered rows), every other byte of the plane is unchanged, and outputs and exported state equal wmx_nsx_process
over a dense plane of the same rows in the same order.  Integers, np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from conf_inputs import EINVAL
from leg_denoise_model import ROW, rows_taken, suppress
from leg_seq_model import pack

pytestmark = pytest.mark.gpu

N, TICKS, IDLE_LEG = 37, 40, 5
OTHER_LENS = (0, 0, 0, 172, 318, 322, 640, 160)  # what a slot that holds no row says
AMPS = (3, 40, 400, 3000, 12000, 30000)


def signal(rng, g, n):
    """n samples of leg g: noise at the leg's level under a tone that comes and goes"""
    t = np.arange(n)
    x = rng.normal(0, AMPS[g % len(AMPS)], n) + 0.5 * AMPS[(g + 2) % len(AMPS)] * np.sin(2 * np.pi * (200 + 37 * g) * t / 8000) * (t % 4000 < 2000)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def random_list(rng, lens, k_slots):
    """a call list over one leg's slots: a permuted subset of the readable slots, silence calls between them, now and then a data call
    naming a slot that holds no row or lies beyond max_packets; often filled up to four calls"""
    readable = [k for k in range(k_slots) if lens[k] == 320]
    rng.shuffle(readable)
    calls = [("D", k) for k in readable[:len(readable) if rng.integers(0, 2) else int(rng.integers(0, len(readable) + 1))]]
    unreadable = [k for k in range(4) if k >= k_slots or lens[k] != 320]
    if unreadable and len(calls) < 4 and rng.integers(0, 3) == 0:
        calls.insert(int(rng.integers(0, len(calls) + 1)), ("D", int(rng.choice(unreadable))))
    target = 4 if rng.integers(0, 2) else int(rng.integers(len(calls), 5))
    while len(calls) < target:
        calls.insert(int(rng.integers(0, len(calls) + 1)), ("S", None))
    return calls


def script(seed, k_slots, with_lists, n=N, ticks=TICKS, pad=8):
    """-> per tick (plane int16 [n, k_slots, 160 + pad], lens uint32 [n, k_slots], lists or None)"""
    rng = np.random.default_rng(seed)
    src = [signal(rng, g, ticks * k_slots * ROW) for g in range(n)]
    at, out = [0] * n, []
    for t in range(ticks):
        plane = rng.integers(-32768, 32768, size=(n, k_slots, ROW + pad)).astype(np.int16)  # rows not taken hold anything
        lens = rng.choice(OTHER_LENS, size=(n, k_slots)).astype(np.uint32)
        for g in range(n):
            if g == IDLE_LEG:
                continue
            for k in rng.permutation(k_slots)[:int(rng.integers(0, k_slots + 1))]:
                lens[g, k] = 320
                plane[g, k, :ROW] = src[g][at[g]:at[g] + ROW]
                at[g] += ROW
        lists = [random_list(rng, lens[g], k_slots) for g in range(n)] if with_lists else None
        if with_lists:
            lists[IDLE_LEG] = [c for c in lists[IDLE_LEG] if c[0] == "S"]
        out.append((plane, lens, lists))
    return out


def blobs(nb):
    return [nb.export_stream(g) for g in range(nb.n_streams)]


def run_legs(cuda, ticks, nb=None, offset=0):
    """the kernel over a script -> (the planes as it left them, the handle).  offset: the plane starts that many int16 into its buffer"""
    import torch
    from wmix_amd.nsx import NsxBatch
    nb = nb or NsxBatch(ticks[0][0].shape[0], 1, 8000)
    got = []
    for plane, lens, lists in ticks:
        buf = torch.zeros(plane.size + offset, dtype=torch.int16, device=cuda)
        d = buf[offset:].view(plane.shape)
        d.copy_(torch.from_numpy(plane))
        d_lens = torch.from_numpy(lens.view(np.int32)).to(cuda)
        d_calls = None if lists is None else torch.from_numpy(np.array([pack(c) for c in lists], np.uint32).view(np.int32)).to(cuda)
        nb.process_legs(d[:, :, :ROW], d_lens, d_calls)
        got.append(d.cpu().numpy())
    return got, nb


def check_against_model(lib, ticks, got):
    """assertions 1 and 2 -> per leg the (tick, slot) fed, in order"""
    n = ticks[0][0].shape[0]
    fed = [[] for _ in range(n)]
    for t, (plane, lens, lists) in enumerate(ticks):
        keep = np.ones(plane.shape, bool)
        for g in range(n):
            for k in rows_taken(lens[g], None if lists is None else lists[g]):
                fed[g].append((t, k))
                keep[g, k, :ROW] = False
        assert np.array_equal(got[t][keep], plane[keep]), ("a row that was not taken changed, tick", t)
    for g in range(n):
        want = suppress(lib, [ticks[t][0][g, k, :ROW] for t, k in fed[g]])
        have = np.array([got[t][g, k, :ROW] for t, k in fed[g]], np.int16).reshape(-1, ROW)
        assert np.array_equal(have, want), ("leg", g, "first row that differs", int(np.argwhere((have != want).any(1))[0]))
    return fed


def check_against_dense(cuda, ticks, got, fed, nb):
    """assertion 3: wmx_nsx_process, every stream the same number of rows per call, the streams with fewer switched off"""
    import torch
    from wmix_amd.nsx import NsxBatch
    n = ticks[0][0].shape[0]
    dense = NsxBatch(n, 1, 8000)
    for t, (plane, _, _) in enumerate(ticks):
        mine = [[k for u, k in fed[g] if u == t] for g in range(n)]
        for r in range(max(len(m) for m in mine)):
            live = np.array([len(m) > r for m in mine])
            rows = np.stack([plane[g, mine[g][r], :ROW] if live[g] else np.zeros(ROW, np.int16) for g in range(n)])
            dense.set_active(live)
            out = dense.process(torch.from_numpy(rows.reshape(n, 2, 80)).to(cuda)).cpu().numpy().reshape(n, ROW)
            for g in np.flatnonzero(live):
                assert np.array_equal(out[g], got[t][g, mine[g][r], :ROW]), ("tick", t, "leg", g)
    for g, (a, b) in enumerate(zip(blobs(nb), blobs(dense))):
        assert np.array_equal(a, b), ("state of leg", g)
    dense.close()


@pytest.mark.parametrize("k_slots,with_lists", [(1, False), (3, False), (4, False), (1, True), (3, True), (4, True)])
def test_ragged_rows_equal_the_model_and_the_dense_call(cuda, oracle_port, k_slots, with_lists):
    from wmix_amd.nsx import NsxBatch
    ticks = script(100 * k_slots + int(with_lists), k_slots, with_lists)
    fresh = NsxBatch(N, 1, 8000)
    idle_before = fresh.export_stream(IDLE_LEG)
    got, nb = run_legs(cuda, ticks, fresh)
    fed = check_against_model(oracle_port, ticks, got)
    counts = [len(f) for f in fed]
    assert counts[IDLE_LEG] == 0 and min(c for g, c in enumerate(counts) if g != IDLE_LEG) > 0 and max(counts) >= TICKS // 4
    if with_lists:  # the lists reach what they are for
        lists = [c for _, _, ls in ticks for c in ls]
        assert any(len(c) == 4 for c in lists) and any(("S", None) in c for c in lists)
        assert any(kind == "D" and k >= k_slots for c in lists for kind, k in c) or k_slots == 4
        assert any([k for _, k in c if k is not None] != sorted(k for _, k in c if k is not None) for c in lists) or k_slots == 1
    check_against_dense(cuda, ticks, got, fed, nb)
    # assertion 4: a leg given nothing has the state of a fresh stream
    other = NsxBatch(1, 1, 8000)
    assert np.array_equal(nb.export_stream(IDLE_LEG), idle_before) and np.array_equal(idle_before, other.export_stream(0))
    other.close()
    nb.close()


def test_the_long_run_reaches_the_histogram_update(cuda, oracle_port):
    """3 legs, 2 rows a tick, 140 ticks: 560 blocks, past the suppressor's first feature update from its histograms"""
    rng = np.random.default_rng(7)
    n, ticks_n = 3, 140
    src = [signal(rng, 2 + g, ticks_n * 2 * ROW).reshape(ticks_n, 2, ROW) for g in range(n)]
    ticks = [(np.stack([src[g][t] for g in range(n)]), np.full((n, 2), 320, np.uint32), None) for t in range(ticks_n)]
    got, nb = run_legs(cuda, ticks)
    fed = check_against_model(oracle_port, ticks, got)
    assert all(len(f) == 2 * ticks_n for f in fed)
    check_against_dense(cuda, ticks, got, fed, nb)
    nb.close()


def test_rows_on_a_two_byte_boundary_are_taken_and_an_odd_address_is_refused(cuda, wmx, oracle_port):
    import torch
    ticks = script(9, 3, True, n=6, ticks=6, pad=1)  # rows of 161 samples: every other row is off the 4-byte grid as well
    aligned, nb0 = run_legs(cuda, ticks)
    shifted, nb1 = run_legs(cuda, ticks, offset=1)
    check_against_model(oracle_port, ticks, shifted)
    assert all(np.array_equal(a, b) for a, b in zip(aligned, shifted))
    assert all(np.array_equal(a, b) for a, b in zip(blobs(nb0), blobs(nb1)))
    # one byte further: refused, nothing launched
    plane, lens, _ = ticks[0]
    buf = torch.zeros(plane.size + 4, dtype=torch.int16, device=cuda)
    d_lens = torch.from_numpy(lens.view(np.int32)).to(cuda)
    before = blobs(nb1)
    stream = torch.cuda.current_stream().cuda_stream
    assert buf.data_ptr() % 4 == 0
    assert wmx.wmx_nsx_process_legs(nb1._h, buf.data_ptr() + 1, 3 * 161, 161, 3, d_lens.data_ptr(), None, stream) == EINVAL
    assert b"2-byte" in wmx.wmx_last_error()
    assert wmx.wmx_nsx_process_legs(nb1._h, buf.data_ptr() + 2, 3 * 161, 161, 3, d_lens.data_ptr(), None, stream) == 0
    torch.cuda.synchronize()
    assert not all(np.array_equal(a, b) for a, b in zip(before, blobs(nb1)))  # that one ran
    nb0.close()
    nb1.close()


def test_refusals_launch_nothing(cuda, wmx):
    import torch
    from wmix_amd.nsx import NsxBatch
    n, k = 6, 3
    rng = np.random.default_rng(3)
    plane = rng.integers(-3000, 3000, size=(n, k, ROW)).astype(np.int16)
    d, d_lens = torch.from_numpy(plane).to(cuda), torch.full((n, k), 320, dtype=torch.int32, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    nb = NsxBatch(n, 1, 8000)
    nb.process_legs(d.clone(), d_lens)  # a state that is not the fresh one
    before = blobs(nb)
    p, ln = d.data_ptr(), d_lens.data_ptr()
    bad = [(nb._h, p, k * ROW, ROW, 0, ln), (nb._h, p, k * ROW, ROW, 5, ln), (nb._h, p, k * ROW, ROW, -1, ln),  # max_packets
           (nb._h, None, k * ROW, ROW, k, ln), (nb._h, p, k * ROW, ROW, k, None),                               # NULL
           (nb._h, p, k * ROW, ROW - 1, k, ln), (nb._h, p, k * ROW - 1, ROW, k, ln), (nb._h, p, 0, ROW, k, ln),  # rows that overlap
           (nb._h, p + 1, k * ROW, ROW, k, ln), (None, p, k * ROW, ROW, k, ln)]
    others = [NsxBatch(n, 2, 8000), NsxBatch(n, 1, 16000), NsxBatch(n, 1, 32000)]
    bad += [(o._h, p, k * ROW, ROW, k, ln) for o in others]  # a handle that is not 1 x 8000
    others_before = [blobs(o) for o in others]
    for h, pcm, ls, ps, kk, lens in bad:
        assert wmx.wmx_nsx_process_legs(h, pcm, ls, ps, kk, lens, None, stream) == EINVAL, (ls, ps, kk)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), plane) and all(np.array_equal(a, b) for a, b in zip(before, blobs(nb)))
    for o, was in zip(others, others_before):
        assert all(np.array_equal(a, b) for a, b in zip(was, blobs(o)))
    for o in others + [nb]:
        o.close()
