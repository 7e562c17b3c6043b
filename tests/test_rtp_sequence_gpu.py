"""wmx_rtp_sequence_legs / wmx_rtp_reset_sequence / wmx_rtp_export_sequence (wmix_amd/csrc/rtp.hip, leg_seq.h) alone, through the Python
mirror, against tests/leg_seq_model.py: 130 legs -- two full waves and a ragged third -- whose senders lose, duplicate, swap, delay
and restart, 30 ticks; the call lists, the rewritten d_len and the exported state and counters are compared after every tick.
Integers, np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from conf_inputs import EINVAL
from leg_seq_model import COUNTERS, LegsSeqModel

pytestmark = pytest.mark.gpu

N, T = 130, 30


def arrivals(seed, n, ticks, K):
    """-> seq_raw uint16 [ticks, n, K] as ingest stores it (header bytes 2..3, no ntohs), lens uint32 [ticks, n, K] (320 or 0).  Per leg
    a sender that counts from a random start (some near the uint16 wrap); a packet is lost, sent twice, held back one tick, tagged
    with a payload type that is no audio (len 0: a gap), or follows a restart of the sender at a far number; what a tick delivers is
    shuffled now and then and laid into random slots."""
    rng = np.random.default_rng(seed)
    raw, lens = np.zeros((ticks, n, K), np.uint16), np.zeros((ticks, n, K), np.uint32)
    for g in range(n):
        seq = int(rng.choice([0, 65530, int(rng.integers(0, 65536))]))
        held = []
        for t in range(ticks):
            now, held = held, []
            for _ in range(int(rng.choice([0, 1, 1, 1, 1, 2, 3]))):
                what = rng.integers(0, 20)
                if what == 0:
                    seq = (seq + int(rng.integers(17, 60000))) % 65536  # the sender restarts
                pkt = (seq, 0 if what == 1 else 320)                     # a payload type that is no audio
                seq = (seq + 1) % 65536
                if what in (2, 3):
                    continue                                              # lost
                if what == 4:
                    now += [pkt, pkt]                                     # sent twice
                elif what == 5:
                    held.append(pkt)                                      # a tick late
                elif what == 6 and K > 1:
                    now += [pkt, ((pkt[0] - int(rng.integers(1, 30))) % 65536, 320)]  # and something old beside it
                else:
                    now.append(pkt)
            if rng.integers(0, 4) == 0:
                rng.shuffle(now)
            now = now[:K]
            for k, (s, ln) in zip(sorted(rng.choice(K, size=len(now), replace=False)), now):
                raw[t, g, k] = ((s & 0xFF) << 8) | (s >> 8)
                lens[t, g, k] = ln
    return raw, lens


def device_seq(raw_t, cuda, aligned):
    """the tick's sequence numbers on the device; not aligned: the same values two bytes off an 8-byte boundary"""
    import torch
    if aligned:
        return torch.from_numpy(raw_t.view(np.int16)).to(cuda)
    store = torch.zeros(raw_t.size + 4, dtype=torch.int16, device=cuda)
    view = store[1:1 + raw_t.size].view(raw_t.shape)
    view.copy_(torch.from_numpy(raw_t.view(np.int16)))
    assert view.data_ptr() % 8 == 2
    return view


def check_tick(snd, model, raw_t, lens_t, max_gap, cuda, aligned, what):
    import torch
    dlen = torch.from_numpy(lens_t.view(np.int32).copy()).to(cuda)
    calls = snd.sequence_legs(device_seq(raw_t, cuda, aligned), dlen, max_gap)
    want_calls, want_len, _ = model.tick(raw_t, lens_t, max_gap)
    got_calls, got_len = calls.cpu().numpy().view(np.uint32), dlen.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_calls, want_calls), (what, "calls of legs", np.flatnonzero(got_calls != want_calls)[:8])
    assert np.array_equal(got_len, want_len), (what, "d_len of legs", np.argwhere(got_len != want_len)[:8])
    got, want = snd.export_sequence(), model.export()
    for name in want:
        assert np.array_equal(got[name], want[name]), (what, name, np.flatnonzero(got[name] != want[name])[:8])
    return want


@pytest.mark.parametrize("K,aligned,max_gap", [(1, True, 3), (3, True, 3), (4, True, 3), (4, False, 2), (3, True, 0)])
def test_every_tick_equals_the_model(cuda, K, aligned, max_gap):
    from wmix_amd.rtp import RtpSenders
    raw, lens = arrivals(100 + K, N, T, K)
    snd, model = RtpSenders(N), LegsSeqModel(N)
    first = snd.export_sequence()
    assert not any(first[name].any() for name in first)  # before any call: unsynced, zero
    for t in range(T):
        want = check_tick(snd, model, raw[t], lens[t], max_gap, cuda, aligned, ("tick", t))
    # the script did what it is for
    assert want["synced"].all()
    for name in COUNTERS:
        # one slot holds neither a duplicate nor too many calls; without silence calls three slots are three calls at the most
        if not (name in ("overflow", "dup") and K == 1) and not (name in ("lost", "overflow") and max_gap == 0):
            assert want[name].sum() >= 3, (name, want[name].sum())
    snd.close()


def test_reset_of_some_legs_in_mid_run(cuda):
    from wmix_amd.rtp import RtpSenders
    K = 3
    raw, lens = arrivals(7, N, T, K)
    snd, model = RtpSenders(N), LegsSeqModel(N)
    some = [0, 63, 64, 65, 127, 128, 129]
    for t in range(T):
        if t == 12:
            before = model.export()
            assert before["synced"][some].all() and sum(int(before[c][some].sum()) for c in COUNTERS) > 0
            snd.reset_sequence(some)
            model.reset(some)
            got, want = snd.export_sequence(), model.export()
            assert all(np.array_equal(got[name], want[name]) for name in want)
            assert not want["synced"][some].any() and want["synced"].sum() == before["synced"].sum() - len(some)
        if t == 20:
            snd.reset_sequence()
            model.reset()
            got = snd.export_sequence()
            assert not any(got[name].any() for name in got)
        check_tick(snd, model, raw[t], lens[t], 3, cuda, True, ("tick", t))
    snd.close()


def test_refusals_leave_state_and_outputs_alone(cuda, wmx):
    import torch
    from wmix_amd.rtp import RtpSenders
    K = 3
    raw, lens = arrivals(9, N, 6, K)
    snd, model = RtpSenders(N), LegsSeqModel(N)
    for t in range(5):
        check_tick(snd, model, raw[t], lens[t], 3, cuda, True, ("tick", t))
    stream = torch.cuda.current_stream().cuda_stream
    seq = torch.from_numpy(raw[5].view(np.int16)).to(cuda)
    dlen = torch.from_numpy(lens[5].view(np.int32).copy()).to(cuda)
    calls = torch.full((N,), 0x5A5A5A5A, dtype=torch.int32, device=cuda)
    before = snd.export_sequence()
    f = wmx.wmx_rtp_sequence_legs
    refused = [f(None, K, 3, seq.data_ptr(), dlen.data_ptr(), calls.data_ptr(), stream),
               f(snd._h, K, 3, None, dlen.data_ptr(), calls.data_ptr(), stream),
               f(snd._h, K, 3, seq.data_ptr(), None, calls.data_ptr(), stream),
               f(snd._h, K, 3, seq.data_ptr(), dlen.data_ptr(), None, stream)]
    refused += [f(snd._h, k, 3, seq.data_ptr(), dlen.data_ptr(), calls.data_ptr(), stream) for k in (0, 5, -1)]
    refused += [f(snd._h, K, g, seq.data_ptr(), dlen.data_ptr(), calls.data_ptr(), stream) for g in (-1, 4)]
    bad = np.array([3, N], np.int32)
    refused.append(wmx.wmx_rtp_reset_sequence(snd._h, bad.ctypes.data, 2, stream))
    refused.append(wmx.wmx_rtp_reset_sequence(None, None, 0, stream))
    refused.append(wmx.wmx_rtp_export_sequence(None, None, None, None, None, None, None, None, stream))
    assert refused == [EINVAL] * len(refused), refused
    after = snd.export_sequence()
    assert all(np.array_equal(before[name], after[name]) for name in before)
    assert (calls.cpu().numpy() == 0x5A5A5A5A).all() and np.array_equal(dlen.cpu().numpy().view(np.uint32), lens[5])
    # any pointer of the export may be NULL
    late = np.zeros(N, np.uint32)
    assert wmx.wmx_rtp_export_sequence(snd._h, None, None, None, late.ctypes.data, None, None, None, stream) == 0
    assert np.array_equal(late, before["late"])
    # and the handle still works
    check_tick(snd, model, raw[5], lens[5], 3, cuda, True, "after the refusals")
    snd.close()
