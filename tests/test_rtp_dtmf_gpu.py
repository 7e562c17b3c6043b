"""wmx_rtp_detect_dtmf_legs / wmx_rtp_reset_dtmf / wmx_rtp_export_dtmf (wmix_amd/csrc/rtp.hip, leg_dtmf.h) alone, through the Python
mirror, against tests/leg_dtmf_model.py.  The kernel gives half a wave to a leg and eight legs to a block, so 1, 5 and 67 legs are a
block that is nearly empty, one partly empty, and eight full blocks with a ragged ninth; 1, 3 and 4 slots per leg; PCM rows of 160
samples (on the 4-byte grid) and of 161 (every other row off it); slot order, and call lists with silence calls between tone packets,
slots out of order, duplicates that were discarded (d_len 0) and data calls naming rows that are not readable.  Every leg plays a
stream of its own -- keys of one to four packets, pauses of one to three, voice -- cut into ticks of 0 .. max_packets packets, with
event packets in the slots left over.  count, ring and the PCM rows are compared after every tick.  Integers, np.array_equal."""
import numpy as np
import pytest

from conf_inputs import EINVAL
from leg_dtmf_model import FROM_PACKET, ROW, LegsDtmfModel, event_row, noise, tone
from leg_plc_model import D, S, pack

pytestmark = pytest.mark.gpu

T = 8
SENTINEL = 0x5A5A


def leg_stream(rng, n_blocks):
    """-> n_blocks rows [160] of one leg: keys held for 1 .. 4 packets, pauses of 1 .. 3, stretches of voice"""
    out, n0 = [], 0
    while len(out) < n_blocks:
        kind = int(rng.integers(0, 4))
        if kind <= 1:
            code, amp, ratio = int(rng.integers(0, 16)), float(rng.uniform(600, 12000)), float(rng.uniform(0.75, 1.35))
            for _ in range(int(rng.integers(1, 5))):
                out.append(tone(code, amp, amp * ratio, n0=n0, ph_row=1.0, ph_col=2.0))
                n0 += ROW
        elif kind == 2:
            out += [np.zeros(ROW, np.int16)] * int(rng.integers(1, 4))
        else:
            out += [noise(rng, float(rng.uniform(200, 6000))) for _ in range(int(rng.integers(1, 3)))]
    return out[:n_blocks]


def script(seed, n, K, row, lists_on):
    """-> per tick (packets uint8 [n, K, 172], recv int32 [n, K], pcm int16 [n, K, row], lens uint32 [n, K], lists or None)"""
    rng = np.random.default_rng(seed)
    streams = [leg_stream(rng, T * K) for _ in range(n)]
    at, ev_ts, ev_left, ev_code = [0] * n, [0] * n, [0] * n, [0] * n
    ticks = []
    for _ in range(T):
        pk = rng.integers(0, 256, size=(n, K, 172)).astype(np.uint8)
        pk[:, :, 1] = np.where(rng.integers(0, 2, size=(n, K)) == 0, 8, 0x80 | 0)  # G.711 audio, some with the marker bit
        recv, lens = np.zeros((n, K), np.int32), np.zeros((n, K), np.uint32)
        pcm = np.full((n, K, row), SENTINEL, np.int16)
        pcm[:, :, :ROW] = 0
        lists = []
        for g in range(n):
            n_audio = int(rng.integers(0, K + 1)) if g % 7 != 6 else 0  # one leg in seven sends no audio at all
            slots = [int(k) for k in (rng.permutation(K) if lists_on else np.arange(K))]
            audio_slots = slots[:n_audio] if lists_on else sorted(slots[:n_audio])
            for k in audio_slots:
                pcm[g, k, :ROW], recv[g, k], lens[g, k] = streams[g][at[g]], 172, 320
                at[g] += 1
            for k in slots[n_audio:]:  # what is left: nothing, an event packet, or a packet too short to be one
                what = int(rng.integers(0, 4))
                if what == 0:
                    continue
                if ev_left[g] == 0:
                    ev_ts[g], ev_left[g], ev_code[g] = int(rng.integers(0, 2 ** 32)), int(rng.integers(1, 5)), int(rng.integers(0, 18))
                pk[g, k, :16] = event_row(ev_code[g], ev_ts[g], pt=101 if what < 3 else 96, end=ev_left[g] == 1, marker=bool(rng.integers(0, 2)))
                recv[g, k] = 172 if rng.integers(0, 6) else 15
                ev_left[g] -= 1
            if lists_on:
                calls = [D(k) for k in audio_slots]
                if calls and rng.integers(0, 3) == 0:  # a gap: silence calls in front of one of them
                    j = int(rng.integers(0, len(calls)))
                    calls[j:j] = [S] * int(rng.integers(1, 3))
                if calls and rng.integers(0, 5) == 0:  # a duplicate the sequencer discarded: still in its row, d_len 0, not named
                    lens[g, calls.pop(int(rng.integers(0, len(calls))))[1]] = 0
                if rng.integers(0, 6) == 0:  # a data call that names a row that is not readable
                    k = int(rng.integers(0, 4))
                    if k >= K or lens[g, k] != 320:
                        calls.insert(int(rng.integers(0, len(calls) + 1)), D(k))
                lists.append(calls[:4])
        ticks.append((pk, recv, pcm, lens, lists if lists_on else None))
    return ticks


def check_tick(snd, model, tick, cuda, what, event_pt=101, suppress=True):
    import torch
    pk, recv, pcm, lens, lists = tick
    d_pk, d_recv = torch.from_numpy(pk).to(cuda), torch.from_numpy(recv).to(cuda)
    d_pcm, d_lens = torch.from_numpy(pcm).to(cuda), torch.from_numpy(lens.view(np.int32)).to(cuda)
    words = None if lists is None else np.array([pack(c) for c in lists], np.uint32)
    d_calls = None if lists is None else torch.from_numpy(words.view(np.int32)).to(cuda)
    snd.detect_dtmf_legs(d_pk, d_recv, d_pcm, d_lens, d_calls, event_pt, suppress)
    want_pcm = pcm.copy()
    digits = model.tick(pk, recv, want_pcm, lens, lists, event_pt, suppress)
    got, want = snd.export_dtmf(), model.export()
    assert np.array_equal(got["count"], want["count"]), (what, "count of legs", np.flatnonzero(got["count"] != want["count"])[:8])
    assert np.array_equal(got["ring"], want["ring"]), (what, "ring of legs", np.flatnonzero((got["ring"] != want["ring"]).any(1))[:8])
    got_pcm = d_pcm.cpu().numpy()
    assert np.array_equal(got_pcm, want_pcm), (what, "rows of (leg, slot)", np.argwhere((got_pcm != want_pcm).any(2))[:8])
    # everything else is only read
    assert np.array_equal(d_pk.cpu().numpy(), pk) and np.array_equal(d_recv.cpu().numpy(), recv)
    assert np.array_equal(d_lens.cpu().numpy().view(np.uint32), lens)
    assert words is None or np.array_equal(d_calls.cpu().numpy().view(np.uint32), words)
    tones = sum(d is not None for leg in digits for d in leg)
    return tones, int((want_pcm != pcm).any(2).sum())


@pytest.mark.parametrize("n,K,row,lists_on", [(1, 1, 160, False), (5, 3, 161, False), (5, 4, 160, True), (67, 3, 161, True), (67, 4, 160, False),
                                              (67, 1, 160, True)])
def test_every_tick_equals_the_model(cuda, n, K, row, lists_on):
    from wmix_amd.rtp import RtpSenders
    # the single leg's eight packets: a seed under which it presses a key long enough and sends another as packets
    ticks = script(26 if n == 1 else 100 * n + 10 * K + row + lists_on, n, K, row, lists_on)
    snd, model = RtpSenders(n), LegsDtmfModel(n)
    first = snd.export_dtmf()
    assert not first["count"].any() and not first["ring"].any()  # before any call: fresh
    some = [0, n - 1]
    tones = zeroed = 0
    for t in range(T):
        if t == 5:
            snd.reset_dtmf(some)
            model.reset(some)
            got, want = snd.export_dtmf(), model.export()
            assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["ring"], want["ring"]) and not want["count"][some].any()
        a, b = check_tick(snd, model, ticks[t], cuda, ("tick", t))
        tones, zeroed = tones + a, zeroed + b
    want = model.export()
    assert tones >= 1 and zeroed >= 1 and zeroed <= tones, (tones, zeroed)
    if n >= 5 and K >= 3:
        in_band = sum(int(not (b & FROM_PACKET)) for g in range(n) for b in want["ring"][g][:min(8, want["count"][g])])
        from_packet = sum(int(bool(b & FROM_PACKET)) for g in range(n) for b in want["ring"][g][:min(8, want["count"][g])])
        assert in_band >= 2 and from_packet >= 2, (in_band, from_packet)
    snd.reset_dtmf()
    got = snd.export_dtmf()
    assert not got["count"].any() and not got["ring"].any()
    snd.close()


def test_without_suppression_no_row_changes_and_the_digits_are_the_same(cuda):
    from wmix_amd.rtp import RtpSenders
    n, K = 5, 3
    ticks = script(77, n, K, 160, False)
    on, off, model = RtpSenders(n), RtpSenders(n), LegsDtmfModel(n)
    for t in range(T):
        check_tick(on, model, ticks[t], cuda, ("suppress, tick", t), suppress=True)
    model_off = LegsDtmfModel(n)
    for t in range(T):
        _, zeroed = check_tick(off, model_off, ticks[t], cuda, ("plain, tick", t), suppress=False)
        assert zeroed == 0
    a, b = on.export_dtmf(), off.export_dtmf()
    assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["ring"], b["ring"]) and a["count"].sum() >= 2
    on.close()
    off.close()


def test_another_event_payload_type_reads_other_packets(cuda):
    from wmix_amd.rtp import RtpSenders
    n, K = 5, 3
    ticks = script(78, n, K, 160, False)
    counts = {}
    for pt in (101, 96, 127):
        snd, model = RtpSenders(n), LegsDtmfModel(n)
        for t in range(T):
            check_tick(snd, model, ticks[t], cuda, ("pt", pt, "tick", t), event_pt=pt, suppress=False)
        counts[pt] = int(sum(bool(b & FROM_PACKET) for g in range(n) for b in model.export()["ring"][g][:min(8, model.export()["count"][g])]))
        snd.close()
    assert counts[101] >= 1 and counts[96] >= 1 and counts[127] == 0, counts


def test_refusals_leave_state_and_rows_alone(cuda, wmx):
    import torch
    from wmix_amd.rtp import RtpSenders
    n, K = 5, 3
    ticks = script(79, n, K, 160, True)
    snd, model = RtpSenders(n), LegsDtmfModel(n)
    for t in range(4):
        check_tick(snd, model, ticks[t], cuda, ("tick", t))
    stream = torch.cuda.current_stream().cuda_stream
    pk, recv, pcm, lens, lists = ticks[4]
    d_pk, d_recv = torch.from_numpy(pk).to(cuda), torch.from_numpy(recv).to(cuda)
    d_pcm, d_lens = torch.from_numpy(pcm).to(cuda), torch.from_numpy(lens.view(np.int32)).to(cuda)
    d_calls = torch.from_numpy(np.array([pack(c) for c in lists], np.uint32).view(np.int32)).to(cuda)
    before = snd.export_dtmf()
    f = wmx.wmx_rtp_detect_dtmf_legs
    good = [snd._h, K, d_pk.data_ptr(), K * 172, 172, d_recv.data_ptr(), d_pcm.data_ptr(), K * 160, 160, d_lens.data_ptr(), d_calls.data_ptr(), 101, 1,
            stream]
    refused = []
    for at in (0, 2, 5, 6, 9):  # every pointer but d_calls NULL in turn
        refused.append(f(*[None if i == at else a for i, a in enumerate(good)]))
    for k in (0, 5, -1):
        refused.append(f(*[k if i == 1 else a for i, a in enumerate(good)]))
    for pt in (95, 128, 0, 8, -1):
        refused.append(f(*[pt if i == 11 else a for i, a in enumerate(good)]))
    refused.append(f(*[171 if i == 4 else a for i, a in enumerate(good)]))          # a datagram row shorter than a datagram
    refused.append(f(*[159 if i == 8 else a for i, a in enumerate(good)]))          # a PCM row overlaps the next
    refused.append(f(*[K * 160 - 1 if i == 7 else a for i, a in enumerate(good)]))  # a leg's rows overlap the next leg's
    refused.append(f(*[K * 172 - 1 if i == 3 else a for i, a in enumerate(good)]))
    bad = np.array([3, n], np.int32)
    refused.append(wmx.wmx_rtp_reset_dtmf(snd._h, bad.ctypes.data, 2, stream))
    refused.append(wmx.wmx_rtp_reset_dtmf(None, None, 0, stream))
    refused.append(wmx.wmx_rtp_export_dtmf(None, None, None, stream))
    assert refused == [EINVAL] * len(refused), refused
    assert b"event_pt" in wmx.wmx_last_error() or b"wmx_rtp" in wmx.wmx_last_error()
    after = snd.export_dtmf()
    assert np.array_equal(before["count"], after["count"]) and np.array_equal(before["ring"], after["ring"])
    assert np.array_equal(d_pcm.cpu().numpy(), pcm)
    count = np.zeros(n, np.uint32)  # either pointer of the export may be NULL
    assert wmx.wmx_rtp_export_dtmf(snd._h, count.ctypes.data, None, stream) == 0 and np.array_equal(count, before["count"])
    assert wmx.wmx_rtp_export_dtmf(snd._h, None, None, stream) == 0
    for t in range(4, T):  # and the handle still works
        check_tick(snd, model, ticks[t], cuda, ("after the refusals, tick", t))
    snd.close()
