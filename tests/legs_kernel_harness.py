"""The kernel tests of the bridge's per-leg stages (tests/test_nsx_legs_gpu.py, test_agc_legs_gpu.py, test_vad_legs_gpu.py): the kernel
over a script of ragged rows, the comparisons with the stage's model and with its dense entry point, and the bodies of the tests the
stages share.  A stage is described by a Stage: how its batch is made, the [packets, samples] its dense call takes a row as, what its
model makes of a leg's ordered rows, its C entry point, what that says of a handle of another shape, and the arguments the entry point
takes between the call lists and the stream.  Integers, np.array_equal."""
from collections import namedtuple

import numpy as np

from conf_inputs import EINVAL
from leg_rows_model import ROW, rows_taken
from leg_seq_model import pack

# make(n) -> the batch; dense_shape: a row as the dense call's [packets, samples]; model(lib, rows [r, 160], leg) -> [r, 160];
# entry: the name in libwmix_amd.so; handle_message: in the error text for a handle that is not the stage's shape; c_extras: the
# entry point's arguments between d_calls and stream, as a test that has none of its own passes them
Stage = namedtuple("Stage", "make dense_shape model entry handle_message c_extras")


def blobs(batch):
    return [batch.export_stream(g) for g in range(batch.n_streams)]


def run_legs(cuda, ticks, batch, offset=0, extras=(), watch=None):
    """the kernel over a script -> (the planes as it left them, behind every tick {leg: state blob} of the legs in `watch`).  offset:
    the plane starts that many int16 into its buffer; extras: what process_legs takes behind the call lists"""
    import torch
    got, seen = [], []
    for plane, lens, lists in ticks:
        buf = torch.zeros(plane.size + offset + 8, dtype=torch.int16, device=cuda)
        d = buf[offset:offset + plane.size].view(plane.shape)
        d.copy_(torch.from_numpy(plane))
        d_lens = torch.from_numpy(lens.view(np.int32)).to(cuda)
        d_calls = None if lists is None else torch.from_numpy(np.array([pack(c) for c in lists], np.uint32).view(np.int32)).to(cuda)
        batch.process_legs(d[:, :, :ROW], d_lens, d_calls, *extras)
        got.append(d.cpu().numpy())
        seen.append({g: batch.export_stream(g) for g in watch or ()})
    return got, seen


def check_against_model(stage, lib, ticks, got):
    """every byte outside the rows taken is what it was, and every row taken is the model's over the leg's ordered rows
    -> per leg the (tick, slot) fed, in order"""
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
        want = stage.model(lib, [ticks[t][0][g, k, :ROW] for t, k in fed[g]], g)
        have = np.array([got[t][g, k, :ROW] for t, k in fed[g]], np.int16).reshape(-1, ROW)
        assert np.array_equal(have, want), ("leg", g, "first row that differs", int(np.argwhere((have != want).any(1))[0]))
    return fed


def check_against_dense(stage, cuda, ticks, got, fed, batch):
    """the stage's dense entry point, every stream the same number of rows per call, the streams with fewer switched off: the rows and
    the exported state of every leg.  fed: per leg the (tick, slot) fed, in order"""
    import torch
    n = ticks[0][0].shape[0]
    dense = stage.make(n)
    for t, (plane, _, _) in enumerate(ticks):
        mine = [[k for u, k in fed[g] if u == t] for g in range(n)]
        for r in range(max(len(m) for m in mine)):
            live = np.array([len(m) > r for m in mine])
            rows = np.stack([plane[g, mine[g][r], :ROW] if live[g] else np.zeros(ROW, np.int16) for g in range(n)])
            dense.set_active(live)
            out = dense.process(torch.from_numpy(rows.reshape((n,) + stage.dense_shape)).to(cuda)).cpu().numpy().reshape(n, ROW)
            for g in np.flatnonzero(live):
                assert np.array_equal(out[g], got[t][g, mine[g][r], :ROW]), ("tick", t, "leg", g)
    for g, (a, b) in enumerate(zip(blobs(batch), blobs(dense))):
        assert np.array_equal(a, b), ("state of leg", g)
    dense.close()


# ---- the bodies of the tests the stages share
def odd_address_is_refused(stage, cuda, wmx, batch, plane, lens):
    """d_pcm on an odd byte (rows of 161 samples, three slots): refused with the 2-byte message, no state moves and no byte is written;
    one byte further the call runs.  plane, lens: a tick of the script `batch` has been run over"""
    import torch
    entry = getattr(wmx, stage.entry)
    buf = torch.zeros(plane.size + 4, dtype=torch.int16, device=cuda)
    d_lens = torch.from_numpy(lens.view(np.int32)).to(cuda)
    before = blobs(batch)
    stream = torch.cuda.current_stream().cuda_stream
    assert buf.data_ptr() % 4 == 0 and plane.shape[1:] == (3, 161)
    assert entry(batch._h, buf.data_ptr() + 1, 3 * 161, 161, 3, d_lens.data_ptr(), None, *stage.c_extras, stream) == EINVAL
    assert b"2-byte" in wmx.wmx_last_error()
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(before, blobs(batch))) and not buf.cpu().numpy().any()
    buf[1:1 + plane.size].copy_(torch.from_numpy(plane.reshape(-1)))
    assert entry(batch._h, buf.data_ptr() + 2, 3 * 161, 161, 3, d_lens.data_ptr(), None, *stage.c_extras, stream) == 0
    torch.cuda.synchronize()
    assert not all(np.array_equal(a, b) for a, b in zip(before, blobs(batch)))  # that one ran


def two_byte_boundary(stage, cuda, wmx, lib, ticks):
    """ticks: a script with rows of 161 samples, so every other row is off the 4-byte grid as well.  The plane one sample into its
    buffer gives the model's rows, and the planes and states of the same script on the buffer's start; an odd address is refused"""
    b0, b1 = stage.make(ticks[0][0].shape[0]), stage.make(ticks[0][0].shape[0])
    aligned, _ = run_legs(cuda, ticks, b0)
    shifted, _ = run_legs(cuda, ticks, b1, offset=1)
    check_against_model(stage, lib, ticks, shifted)
    assert all(np.array_equal(a, b) for a, b in zip(aligned, shifted))
    assert all(np.array_equal(a, b) for a, b in zip(blobs(b0), blobs(b1)))
    odd_address_is_refused(stage, cuda, wmx, b1, ticks[0][0], ticks[0][1])
    b0.close()
    b1.close()


def switched_off(stage, cuda, n, off, extras=()):
    """set_active's mask holds in the ragged call: a leg that is switched off is a leg without a row -- its rows and its state stay; the
    others' move.  Switched on again every leg is taken.  extras go with the first call -> the plane, the mask, what the second call left"""
    import torch
    rng = np.random.default_rng(4)
    plane = rng.integers(-3000, 3000, size=(n, 3, ROW)).astype(np.int16)
    d_lens = torch.full((n, 3), 320, dtype=torch.int32, device=cuda)
    batch = stage.make(n)
    fresh = blobs(batch)
    mask = np.ones(n, bool)
    mask[off] = False
    batch.set_active(mask)
    got = batch.process_legs(torch.from_numpy(plane).to(cuda), d_lens, *extras).cpu().numpy()
    after = blobs(batch)
    for g in range(n):
        assert np.array_equal(got[g], plane[g]) == (g in off) and np.array_equal(after[g], fresh[g]) == (g in off), g
    batch.set_active(None)
    again = batch.process_legs(torch.from_numpy(plane).to(cuda), d_lens).cpu().numpy()
    assert all(not np.array_equal(a, b) for a, b in zip(blobs(batch), fresh))
    batch.close()
    return plane, mask, again


def refusals(stage, cuda, wmx, others, c_extras=None):
    """every argument the entry point refuses, with the text it sets: nothing is launched -- the rows, the state of a handle that has
    run before and the states of `others` (handles of another shape, closed here) stay"""
    import torch
    entry, c_extras = getattr(wmx, stage.entry), stage.c_extras if c_extras is None else c_extras
    n, k = 6, 3
    rng = np.random.default_rng(3)
    plane = rng.integers(-3000, 3000, size=(n, k, ROW)).astype(np.int16)
    d, d_lens = torch.from_numpy(plane).to(cuda), torch.full((n, k), 320, dtype=torch.int32, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    batch, fresh = stage.make(n), stage.make(1)
    batch.process_legs(d.clone(), d_lens)  # a state that is not the fresh one
    before = blobs(batch)
    assert not np.array_equal(before[0], fresh.export_stream(0))
    p, ln = d.data_ptr(), d_lens.data_ptr()
    bad = [((batch._h, p, k * ROW, ROW, 0, ln), b"max_packets"), ((batch._h, p, k * ROW, ROW, 5, ln), b"max_packets"),
           ((batch._h, p, k * ROW, ROW, -1, ln), b"max_packets"),
           ((batch._h, None, k * ROW, ROW, k, ln), b"NULL"), ((batch._h, p, k * ROW, ROW, k, None), b"NULL"),
           ((batch._h, p, k * ROW, ROW - 1, k, ln), b"overlap"), ((batch._h, p, k * ROW - 1, ROW, k, ln), b"overlap"),
           ((batch._h, p, 0, ROW, k, ln), b"overlap"),
           ((batch._h, p + 1, k * ROW, ROW, k, ln), b"2-byte"), ((None, p, k * ROW, ROW, k, ln), stage.handle_message)]
    bad += [((o._h, p, k * ROW, ROW, k, ln), stage.handle_message) for o in others]
    others_before = [blobs(o) for o in others]
    for (h, pcm, ls, ps, kk, lens), message in bad:
        assert entry(h, pcm, ls, ps, kk, lens, None, *c_extras, stream) == EINVAL, (ls, ps, kk)
        assert stage.entry.encode() in wmx.wmx_last_error() and message in wmx.wmx_last_error(), (message, wmx.wmx_last_error())
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), plane) and all(np.array_equal(a, b) for a, b in zip(before, blobs(batch)))
    for o, was in zip(others, others_before):
        assert all(np.array_equal(a, b) for a, b in zip(was, blobs(o)))
    for o in others + [batch, fresh]:
        o.close()
