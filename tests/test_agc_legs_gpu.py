"""wmx_agc_process_legs (wmix_amd/csrc/agc.hip): the AGC over the ragged rows of a bridge's legs, the kernel alone.  70 legs (one full
workgroup and a part-full one) over 40 ticks of seeded rows at levels from 3 to 30 000: 0 .. max_packets rows per leg and tick, lens
other than 0 and 320 among them, one leg that never gets a row, without call lists and with random ones, every leg on the batch's
compression gain and with legs 1, 9 and 66 on gains of their own (the per-lane gain tables).  Every row taken equals
tests/leg_level_model.py (the oracle over the leg's ordered rows), every other byte of the plane is unchanged, and outputs and exported
state equal wmx_agc_process over a dense plane of the same rows in the same order.  Integers, np.array_equal."""
import numpy as np
import pytest

from conf_inputs import EINVAL
from leg_level_model import ROW, level, rows_taken
from leg_seq_model import pack
from test_nsx_legs_gpu import IDLE_LEG, TICKS, script

pytestmark = pytest.mark.gpu

N, VALUE = 70, 20
OWN = {1: 6, 9: 30, 66: 12}  # leg -> a compression gain of its own


def make(n=N, own=None):
    from wmix_amd.agc import AgcBatch
    ab = AgcBatch(n, 1, 8000, VALUE)
    for g, v in (own or {}).items():
        ab.set_gain_streams([g], v)
    return ab


def blobs(ab):
    return [ab.export_stream(g) for g in range(ab.n_streams)]


def run_legs(cuda, ticks, ab, offset=0, watch=None):
    """the kernel over a script -> the planes as it left them.  offset: the plane starts that many int16 into its buffer; watch: a leg
    whose state blob is exported after every tick -> (planes, blobs)"""
    import torch
    got, seen = [], []
    for plane, lens, lists in ticks:
        buf = torch.zeros(plane.size + offset, dtype=torch.int16, device=cuda)
        d = buf[offset:].view(plane.shape)
        d.copy_(torch.from_numpy(plane))
        d_lens = torch.from_numpy(lens.view(np.int32)).to(cuda)
        d_calls = None if lists is None else torch.from_numpy(np.array([pack(c) for c in lists], np.uint32).view(np.int32)).to(cuda)
        ab.process_legs(d[:, :, :ROW], d_lens, d_calls)
        got.append(d.cpu().numpy())
        if watch is not None:
            seen.append(ab.export_stream(watch))
    return (got, seen) if watch is not None else got


def check_against_model(lib, ticks, got, own=None):
    """assertions 1 and 2 -> per leg the (tick, slot) fed, in order"""
    n = ticks[0][0].shape[0]
    fed = [[] for _ in range(n)]
    for t, (plane, lens, lists) in enumerate(ticks):
        keep = np.ones(plane.shape, bool)
        for g in range(n):
            for k in rows_taken(lens[g], None if lists is None else lists[g]):
                fed[g].append((t, k))
                keep[g, k, :ROW] = False
        assert np.array_equal(got[t][keep], plane[keep]), ("a byte outside the rows taken changed, tick", t)
    for g in range(n):
        # a leg on a gain of its own: a handle made with the batch's value, agc_addition in front of its first call
        want = level(lib, [ticks[t][0][g, k, :ROW] for t, k in fed[g]], VALUE, {0: own[g]} if own and g in own else None)
        have = np.array([got[t][g, k, :ROW] for t, k in fed[g]], np.int16).reshape(-1, ROW)
        assert np.array_equal(have, want), ("leg", g, "first row that differs", int(np.argwhere((have != want).any(1))[0]))
    return fed


def check_against_dense(cuda, ticks, got, fed, ab, own=None):
    """assertion 3: wmx_agc_process, every stream the same number of rows per call, the streams with fewer switched off"""
    import torch
    n = ticks[0][0].shape[0]
    dense = make(n, own)
    for t, (plane, _, _) in enumerate(ticks):
        mine = [[k for u, k in fed[g] if u == t] for g in range(n)]
        for r in range(max(len(m) for m in mine)):
            live = np.array([len(m) > r for m in mine])
            rows = np.stack([plane[g, mine[g][r], :ROW] if live[g] else np.zeros(ROW, np.int16) for g in range(n)])
            dense.set_active(live)
            out = dense.process(torch.from_numpy(rows.reshape(n, 2, 80)).to(cuda)).cpu().numpy().reshape(n, ROW)
            for g in np.flatnonzero(live):
                assert np.array_equal(out[g], got[t][g, mine[g][r], :ROW]), ("tick", t, "leg", g)
    for g, (a, b) in enumerate(zip(blobs(ab), blobs(dense))):
        assert np.array_equal(a, b), ("state of leg", g)
    dense.close()


@pytest.mark.parametrize("own", [None, OWN], ids=["one_gain", "own_gains"])
@pytest.mark.parametrize("k_slots,with_lists", [(1, False), (3, False), (4, False), (1, True), (3, True), (4, True)])
def test_ragged_rows_equal_the_model_and_the_dense_call(cuda, oracle_port, k_slots, with_lists, own):
    ticks = script(100 * k_slots + int(with_lists), k_slots, with_lists, n=N)
    ab = make(N, own)
    idle_before = ab.export_stream(IDLE_LEG)
    got, idle_seen = run_legs(cuda, ticks, ab, watch=IDLE_LEG)
    fed = check_against_model(oracle_port, ticks, got, own)
    counts = [len(f) for f in fed]
    assert counts[IDLE_LEG] == 0 and min(c for g, c in enumerate(counts) if g != IDLE_LEG) > 0 and max(counts) >= TICKS // 4
    # the levels reach what they are for: full-scale samples come out of the loud legs, on both sides
    taken = np.concatenate([got[t][g, k, :ROW] for g in range(N) for t, k in fed[g]])
    assert (taken == 32767).any() and (taken == -32768).any()
    if with_lists:
        lists = [c for _, _, ls in ticks for c in ls]
        assert any(len(c) == 4 for c in lists) and any(("S", None) in c for c in lists)
    check_against_dense(cuda, ticks, got, fed, ab, own)
    # assertion 6: the leg given nothing never changes its state -- that of a fresh stream
    assert all(np.array_equal(b, idle_before) for b in idle_seen)
    other = make(1)
    assert np.array_equal(idle_before, other.export_stream(0))
    if own:
        assert [ab.stream_gain(g) for g in (0, 1, 9, 66)] == [VALUE, OWN[1], OWN[9], OWN[66]]
    other.close()
    ab.close()


def test_rows_on_a_two_byte_boundary_are_taken_and_an_odd_address_is_refused(cuda, wmx, oracle_port):
    import torch
    ticks = script(9, 3, True, n=N, ticks=6, pad=1)  # rows of 161 samples: every other row is off the 4-byte grid as well
    ab0, ab1 = make(N, OWN), make(N, OWN)
    aligned = run_legs(cuda, ticks, ab0)
    shifted = run_legs(cuda, ticks, ab1, offset=1)
    check_against_model(oracle_port, ticks, shifted, OWN)
    assert all(np.array_equal(a, b) for a, b in zip(aligned, shifted))
    assert all(np.array_equal(a, b) for a, b in zip(blobs(ab0), blobs(ab1)))
    # one byte further: refused, nothing launched
    plane, lens, _ = ticks[0]
    buf = torch.zeros(plane.size + 4, dtype=torch.int16, device=cuda)
    d_lens = torch.from_numpy(lens.view(np.int32)).to(cuda)
    before = blobs(ab1)
    stream = torch.cuda.current_stream().cuda_stream
    assert buf.data_ptr() % 4 == 0
    assert wmx.wmx_agc_process_legs(ab1._h, buf.data_ptr() + 1, 3 * 161, 161, 3, d_lens.data_ptr(), None, stream) == EINVAL
    assert b"2-byte" in wmx.wmx_last_error()
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(before, blobs(ab1))) and not buf.cpu().numpy().any()
    ab0.close()
    ab1.close()


def test_a_leg_switched_off_keeps_its_rows_and_its_state(cuda):
    """wmx_agc_set_active's mask holds here as in wmx_nsx_process_legs: a leg that is switched off is a leg without a row"""
    import torch
    off = [2, 64, N - 1]
    rng = np.random.default_rng(4)
    plane = rng.integers(-3000, 3000, size=(N, 3, ROW)).astype(np.int16)
    d_lens = torch.full((N, 3), 320, dtype=torch.int32, device=cuda)
    ab = make(N, OWN)
    fresh = blobs(ab)
    mask = np.ones(N, bool)
    mask[off] = False
    ab.set_active(mask)
    got = ab.process_legs(torch.from_numpy(plane).to(cuda), d_lens).cpu().numpy()
    after = blobs(ab)
    for g in range(N):
        assert np.array_equal(got[g], plane[g]) == (g in off) and np.array_equal(after[g], fresh[g]) == (g in off), g
    ab.set_active(None)
    got = ab.process_legs(torch.from_numpy(plane).to(cuda), d_lens).cpu().numpy()
    assert all(not np.array_equal(got[g], plane[g]) and not np.array_equal(a, b) for g, (a, b) in enumerate(zip(blobs(ab), fresh)))
    ab.close()


def test_refusals_launch_nothing(cuda, wmx):
    import torch
    from wmix_amd.agc import AgcBatch
    n, k = 6, 3
    rng = np.random.default_rng(3)
    plane = rng.integers(-3000, 3000, size=(n, k, ROW)).astype(np.int16)
    d, d_lens = torch.from_numpy(plane).to(cuda), torch.full((n, k), 320, dtype=torch.int32, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    ab = make(n)
    ab.process_legs(d.clone(), d_lens)  # a state that is not the fresh one
    before = blobs(ab)
    assert not np.array_equal(before[0], make(1).export_stream(0))
    p, ln = d.data_ptr(), d_lens.data_ptr()
    bad = [((ab._h, p, k * ROW, ROW, 0, ln), b"max_packets"), ((ab._h, p, k * ROW, ROW, 5, ln), b"max_packets"),
           ((ab._h, p, k * ROW, ROW, -1, ln), b"max_packets"),
           ((ab._h, None, k * ROW, ROW, k, ln), b"NULL"), ((ab._h, p, k * ROW, ROW, k, None), b"NULL"),
           ((ab._h, p, k * ROW, ROW - 1, k, ln), b"overlap"), ((ab._h, p, k * ROW - 1, ROW, k, ln), b"overlap"),
           ((ab._h, p, 0, ROW, k, ln), b"overlap"),
           ((ab._h, p + 1, k * ROW, ROW, k, ln), b"2-byte"), ((None, p, k * ROW, ROW, k, ln), b"1 x 8000")]
    others = [AgcBatch(n, 2, 8000, VALUE), AgcBatch(n, 1, 16000, VALUE), AgcBatch(n, 1, 32000, VALUE)]
    bad += [((o._h, p, k * ROW, ROW, k, ln), b"1 x 8000") for o in others]  # a handle that is not 1 x 8000
    others_before = [blobs(o) for o in others]
    for (h, pcm, ls, ps, kk, lens), message in bad:
        assert wmx.wmx_agc_process_legs(h, pcm, ls, ps, kk, lens, None, stream) == EINVAL, (ls, ps, kk)
        assert message in wmx.wmx_last_error(), (message, wmx.wmx_last_error())
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), plane) and all(np.array_equal(a, b) for a, b in zip(before, blobs(ab)))
    for o, was in zip(others, others_before):
        assert all(np.array_equal(a, b) for a, b in zip(was, blobs(o)))
    for o in others + [ab]:
        o.close()
