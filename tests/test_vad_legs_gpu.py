"""wmx_vad_process_legs (wmix_amd/csrc/vad.hip): the voice-activity gate over the ragged rows of a bridge's legs, the kernel alone.
70 legs (one full workgroup and one of 6 lanes) over 40 ticks of tests/leg_gate_inputs.py: the alternating spurts at a phase per leg, a
quiet leg, a sigma = 400 noise leg and a random-codes leg; 0 .. max_packets rows per leg and tick, ticks in which the second workgroup
brings nothing, lens other than 0 and 320 among them, without call lists and with random ones.  Every plane equals
tests/leg_gate_model.py's (the oracle's handle per leg over the leg's ordered rows; every byte outside the rows taken is the sentinel
it was), `reduce` and the voice counts equal the model's, a leg without a row keeps its state blob byte for byte (read on a dozen
legs of both workgroups behind every tick), and outputs and exported state equal wmx_vad_process over each leg's gathered rows.
tests/test_leg_gate_model_host.py holds the script against what it is for.  Integers, np.array_equal."""
import numpy as np
import pytest

from conf_inputs import EINVAL
from leg_gate_inputs import CASES, N, QUIET_LEG, ROW, case_seed, script
from leg_gate_model import LegsGateModel
from leg_seq_model import pack

pytestmark = pytest.mark.gpu


def make(n=N, interval_ms=20, chn=1, freq=8000):
    from wmix_amd.vad import VadBatch
    return VadBatch(n, chn, freq, interval_ms)


def blobs(vb):
    return [vb.export_stream(g) for g in range(vb.n_streams)]


WATCHED = [0, 3, 10, 17, 31, 63] + list(range(64, N))  # legs of both workgroups whose state blob is read behind every tick


def run_legs(cuda, ticks, vb, offset=0, voice=None, watch=False):
    """the kernel over a script -> the planes as it left them (watch: and the WATCHED legs' state blobs behind every tick).  offset:
    the plane starts that many int16 into its buffer"""
    import torch
    got, seen = [], []
    for plane, lens, lists in ticks:
        buf = torch.zeros(plane.size + offset + 8, dtype=torch.int16, device=cuda)
        d = buf[offset:offset + plane.size].view(plane.shape)
        d.copy_(torch.from_numpy(plane))
        d_lens = torch.from_numpy(lens.view(np.int32)).to(cuda)
        d_calls = None if lists is None else torch.from_numpy(np.array([pack(c) for c in lists], np.uint32).view(np.int32)).to(cuda)
        vb.process_legs(d[:, :, :ROW], d_lens, d_calls, voice)
        got.append(d.cpu().numpy())
        if watch:
            seen.append({g: vb.export_stream(g) for g in WATCHED})
    return (got, seen) if watch else got


def replay(lib, ticks):
    """the model over a script -> (the planes as it leaves them, per tick and leg the slots fed, the model)"""
    m = LegsGateModel(lib, ticks[0][0].shape[0])
    want, fed = [], []
    for plane, lens, lists in ticks:
        p = plane.copy()
        fed.append(m.tick(p, lens, lists))
        want.append(p)
    return want, fed, m


def check_against_dense(cuda, ticks, got, fed, vb):
    """wmx_vad_process, one call of one packet, every stream the same number of rows per tick, the streams with fewer switched off"""
    import torch
    n = ticks[0][0].shape[0]
    dense = make(n)
    for t, (plane, _, _) in enumerate(ticks):
        mine = fed[t]
        for r in range(max(len(m) for m in mine)):
            live = np.array([len(m) > r for m in mine])
            rows = np.stack([plane[g, mine[g][r], :ROW] if live[g] else np.zeros(ROW, np.int16) for g in range(n)])
            dense.set_active(live)
            out = dense.process(torch.from_numpy(rows.reshape(n, 1, ROW)).to(cuda)).cpu().numpy().reshape(n, ROW)
            for g in np.flatnonzero(live):
                assert np.array_equal(out[g], got[t][g, mine[g][r], :ROW]), ("tick", t, "leg", g)
    for g, (a, b) in enumerate(zip(blobs(vb), blobs(dense))):
        assert np.array_equal(a, b), ("state of leg", g)
    dense.close()


@pytest.mark.parametrize("k_slots,with_lists", CASES)
def test_ragged_rows_equal_the_model_and_the_dense_call(cuda, oracle_port, k_slots, with_lists):
    import torch
    ticks = script(case_seed(k_slots, with_lists), k_slots, with_lists)
    want, fed, m = replay(oracle_port, ticks)
    vb = make()
    fresh = {g: vb.export_stream(g) for g in WATCHED}
    voice = torch.zeros((2, N), dtype=torch.int32, device=cuda)
    got, seen = run_legs(cuda, ticks, vb, voice=voice, watch=True)
    for t in range(len(ticks)):
        # the rows taken are the model's, and every other byte of the plane -- untaken rows, their sentinels -- is what it was
        assert np.array_equal(got[t], want[t]), ("tick", t, "legs", np.flatnonzero((got[t] != want[t]).any((1, 2)))[:6])
        before = fresh if t == 0 else seen[t - 1]
        for g in WATCHED:
            same = np.array_equal(seen[t][g], before[g])
            assert same or fed[t][g], ("a leg without a row moved its state: tick", t, "leg", g)
            assert not same or not fed[t][g] or g == QUIET_LEG, ("a leg with a row kept its state: tick", t, "leg", g)
    assert any(not np.array_equal(w, p) for w, (p, _, _) in zip(want, ticks))  # the gate did attenuate something
    assert any(not fed[t][g] for t in range(len(ticks)) for g in WATCHED) and all(any(fed[t][g] for t in range(len(ticks))) for g in WATCHED)
    assert np.array_equal(vb.export_reduce(), m.reduce.astype(np.int16)), (vb.export_reduce(), m.reduce)
    counts = voice.cpu().numpy().view(np.uint32)
    assert np.array_equal(counts[0], m.voiced) and np.array_equal(counts[1], m.unvoiced), (counts, m.voiced, m.unvoiced)
    check_against_dense(cuda, ticks, got, fed, vb)
    m.close()
    vb.close()


def test_rows_on_a_two_byte_boundary_go_through_memory_and_give_the_same_bits(cuda, wmx, oracle_port):
    """d_pcm one sample off the 4-byte grid with packet_stride 161 (the memory path) against the model, and against the same rows packed
    on 16-byte boundaries (rows as 16-byte words through registers); d_voice NULL on the one, given on the other"""
    import torch
    ticks = script(9, 3, True, ticks=10, pad=1)
    packed = [(np.ascontiguousarray(plane[:, :, :ROW]), lens, lists) for plane, lens, lists in ticks]
    want, _, m = replay(oracle_port, ticks)
    vb0, vb1 = make(), make()
    voice = torch.zeros((2, N), dtype=torch.int32, device=cuda)
    aligned = run_legs(cuda, packed, vb0, voice=voice)
    shifted = run_legs(cuda, ticks, vb1, offset=1)
    for t in range(len(ticks)):
        assert np.array_equal(shifted[t], want[t]), ("tick", t)
        assert np.array_equal(aligned[t], want[t][:, :, :ROW]), ("tick", t)
    assert all(np.array_equal(a, b) for a, b in zip(blobs(vb0), blobs(vb1)))
    counts = voice.cpu().numpy().view(np.uint32)
    assert np.array_equal(counts[0], m.voiced) and np.array_equal(counts[1], m.unvoiced) and counts.sum() > 0
    # one byte further: refused, nothing launched
    plane, lens, _ = ticks[0]
    buf = torch.zeros(plane.size + 4, dtype=torch.int16, device=cuda)
    d_lens = torch.from_numpy(lens.view(np.int32)).to(cuda)
    before = blobs(vb1)
    stream = torch.cuda.current_stream().cuda_stream
    assert buf.data_ptr() % 4 == 0
    assert wmx.wmx_vad_process_legs(vb1._h, buf.data_ptr() + 1, 3 * 161, 161, 3, d_lens.data_ptr(), None, None, stream) == EINVAL
    assert b"2-byte" in wmx.wmx_last_error()
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(before, blobs(vb1))) and not buf.cpu().numpy().any()
    m.close()
    vb0.close()
    vb1.close()


def test_a_leg_switched_off_keeps_its_rows_and_its_state(cuda):
    """wmx_vad_set_active's mask holds here as in wmx_nsx_process_legs: a leg that is switched off is a leg without a row"""
    import torch
    off = [2, 64, N - 1]
    rng = np.random.default_rng(4)
    plane = rng.integers(-3000, 3000, size=(N, 3, ROW)).astype(np.int16)
    d_lens = torch.full((N, 3), 320, dtype=torch.int32, device=cuda)
    vb = make()
    fresh = blobs(vb)
    mask = np.ones(N, bool)
    mask[off] = False
    vb.set_active(mask)
    voice = torch.zeros((2, N), dtype=torch.int32, device=cuda)
    got = vb.process_legs(torch.from_numpy(plane).to(cuda), d_lens, None, voice).cpu().numpy()
    after = blobs(vb)
    for g in range(N):
        assert np.array_equal(got[g], plane[g]) == (g in off) and np.array_equal(after[g], fresh[g]) == (g in off), g
    assert np.array_equal(voice.cpu().numpy().sum(0), np.where(mask, 3, 0))
    vb.set_active(None)
    vb.process_legs(torch.from_numpy(plane).to(cuda), d_lens)
    assert all(not np.array_equal(a, b) for a, b in zip(blobs(vb), fresh))  # switched on again: every leg is taken
    vb.close()


def test_refusals_launch_nothing(cuda, wmx):
    import torch
    n, k = 6, 3
    rng = np.random.default_rng(3)
    plane = rng.integers(-3000, 3000, size=(n, k, ROW)).astype(np.int16)
    d, d_lens = torch.from_numpy(plane).to(cuda), torch.full((n, k), 320, dtype=torch.int32, device=cuda)
    voice = torch.zeros((2, n), dtype=torch.int32, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    vb = make(n)
    vb.process_legs(d.clone(), d_lens)  # a state that is not the fresh one
    before = blobs(vb)
    fresh = make(1)
    assert not np.array_equal(before[0], fresh.export_stream(0))
    p, ln = d.data_ptr(), d_lens.data_ptr()
    bad = [((vb._h, p, k * ROW, ROW, 0, ln), b"max_packets"), ((vb._h, p, k * ROW, ROW, 5, ln), b"max_packets"),
           ((vb._h, p, k * ROW, ROW, -1, ln), b"max_packets"),
           ((vb._h, None, k * ROW, ROW, k, ln), b"NULL"), ((vb._h, p, k * ROW, ROW, k, None), b"NULL"),
           ((vb._h, p, k * ROW, ROW - 1, k, ln), b"overlap"), ((vb._h, p, k * ROW - 1, ROW, k, ln), b"overlap"),
           ((vb._h, p, 0, ROW, k, ln), b"overlap"),
           ((vb._h, p + 1, k * ROW, ROW, k, ln), b"2-byte"), ((None, p, k * ROW, ROW, k, ln), b"160 samples")]
    others = [make(n, 10), make(n, 20, chn=2), make(n, 20, freq=16000), make(n, 20, freq=32000)]  # a packet that is not 160 samples of 1 x 8000
    bad += [((o._h, p, k * ROW, ROW, k, ln), b"160 samples") for o in others]
    others_before = [blobs(o) for o in others]
    for (h, pcm, ls, ps, kk, lens), message in bad:
        assert wmx.wmx_vad_process_legs(h, pcm, ls, ps, kk, lens, None, voice.data_ptr(), stream) == EINVAL, (ls, ps, kk)
        assert message in wmx.wmx_last_error(), (message, wmx.wmx_last_error())
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), plane) and all(np.array_equal(a, b) for a, b in zip(before, blobs(vb)))
    assert not voice.cpu().numpy().any()
    for o, was in zip(others, others_before):
        assert all(np.array_equal(a, b) for a, b in zip(was, blobs(o)))
    for o in others + [vb, fresh]:
        o.close()
