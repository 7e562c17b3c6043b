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

from leg_gate_inputs import CASES, N, QUIET_LEG, ROW, case_seed, script
from leg_gate_model import LegsGateModel, gate
from legs_kernel_harness import Stage, blobs, check_against_dense, odd_address_is_refused, refusals, run_legs, switched_off

pytestmark = pytest.mark.gpu


def make(n=N, interval_ms=20, chn=1, freq=8000):
    from wmix_amd.vad import VadBatch
    return VadBatch(n, chn, freq, interval_ms)


# the entry point takes d_voice between the call lists and the stream
STAGE = Stage(make, (1, ROW), lambda lib, rows, g: gate(lib, rows)[0], "wmx_vad_process_legs", b"160 samples", (None,))
WATCHED = [0, 3, 10, 17, 31, 63] + list(range(64, N))  # legs of both workgroups whose state blob is read behind every tick


def replay(lib, ticks):
    """the model over a script -> (the planes as it leaves them, per tick and leg the slots fed, the model)"""
    m = LegsGateModel(lib, ticks[0][0].shape[0])
    want, fed = [], []
    for plane, lens, lists in ticks:
        p = plane.copy()
        fed.append(m.tick(p, lens, lists))
        want.append(p)
    return want, fed, m


@pytest.mark.parametrize("k_slots,with_lists", CASES)
def test_ragged_rows_equal_the_model_and_the_dense_call(cuda, oracle_port, k_slots, with_lists):
    import torch
    ticks = script(case_seed(k_slots, with_lists), k_slots, with_lists)
    want, fed, m = replay(oracle_port, ticks)
    vb = make()
    fresh = {g: vb.export_stream(g) for g in WATCHED}
    voice = torch.zeros((2, N), dtype=torch.int32, device=cuda)
    got, seen = run_legs(cuda, ticks, vb, extras=(voice,), watch=WATCHED)
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
    check_against_dense(STAGE, cuda, ticks, got, [[(t, k) for t in range(len(ticks)) for k in fed[t][g]] for g in range(N)], vb)
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
    aligned, _ = run_legs(cuda, packed, vb0, extras=(voice,))
    shifted, _ = run_legs(cuda, ticks, vb1, offset=1)
    for t in range(len(ticks)):
        assert np.array_equal(shifted[t], want[t]), ("tick", t)
        assert np.array_equal(aligned[t], want[t][:, :, :ROW]), ("tick", t)
    assert all(np.array_equal(a, b) for a, b in zip(blobs(vb0), blobs(vb1)))
    counts = voice.cpu().numpy().view(np.uint32)
    assert np.array_equal(counts[0], m.voiced) and np.array_equal(counts[1], m.unvoiced) and counts.sum() > 0
    odd_address_is_refused(STAGE, cuda, wmx, vb1, ticks[0][0], ticks[0][1])  # one byte further: refused, nothing launched
    m.close()
    vb0.close()
    vb1.close()


def test_a_leg_switched_off_keeps_its_rows_and_its_state(cuda):
    """wmx_vad_set_active's mask holds here as in wmx_nsx_process_legs: a leg that is switched off is a leg without a row"""
    import torch
    voice = torch.zeros((2, N), dtype=torch.int32, device=cuda)
    _, mask, _ = switched_off(STAGE, cuda, N, [2, 64, N - 1], extras=(None, voice))
    assert np.array_equal(voice.cpu().numpy().sum(0), np.where(mask, 3, 0))  # of the call under the mask, which alone was given it


def test_refusals_launch_nothing(cuda, wmx):
    import torch
    voice = torch.zeros((2, 6), dtype=torch.int32, device=cuda)
    others = [make(6, 10), make(6, 20, chn=2), make(6, 20, freq=16000), make(6, 20, freq=32000)]  # a packet that is not 160 samples of 1 x 8000
    refusals(STAGE, cuda, wmx, others, c_extras=(voice.data_ptr(),))
    assert not voice.cpu().numpy().any()
