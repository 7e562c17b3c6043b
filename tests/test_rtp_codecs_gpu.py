"""A G.711 codec per stream (wmix_amd/csrc/rtp.hip, leg_codec.h): wmx_rtp_set_codecs, wmx_rtp_ingest_legs_codecs and the per-stream law
of wmx_rtp_egress / wmx_rtp_egress_rings.  Ingest against tests/leg_codec_model.py (the rule's table over the oracle's two decoders),
send against the oracle's senders (orc_rtp_sender_init(s, law) + orc_rtp_egress) and against wmx_mix_drain + wmx_rtp_egress on a twin.
Bytes and integers, np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from conf_inputs import EINVAL
from leg_codec_model import BY_PT, LAW_A, LAW_U, PCMA, PCMU, REFERENCE, Decoders, ingest, slot
from oracle import loader as L

pytestmark = pytest.mark.gpu

CODECS = [REFERENCE, PCMA, PCMU, BY_PT, PCMU]  # neighbouring rows, and so the lanes of one wave, differ
LEGS = len(CODECS)
PTS = [8, 0, 101, 97, None]  # PCMA, PCMU, telephone-event, the AAC tag, nothing arrived
LAWS = [LAW_A, LAW_U, LAW_U, LAW_A, LAW_U, LAW_A]
RINGS, RING = len(LAWS), 16000


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def senders(n, codecs=None, laws=None, law="a"):
    from wmix_amd.rtp import RtpSenders
    snd = RtpSenders(n, law)
    for g in range(n):
        if codecs is not None or laws is not None:
            snd.set_codecs([g], REFERENCE if codecs is None else codecs[g], LAW_A if laws is None else laws[g])
    return snd


def ticks_of(K, n_ticks=2):
    """per tick: datagram rows [LEGS, K, 172] and recv [LEGS, K]; the payload type cycles over PTS per slot, a leg's consecutive slots
    carry the codes 0 .. 159, 160 .. 255, 0 .. 63, ... (rotated per leg): all 256 across two slots"""
    out, nth = [], [0] * LEGS
    for tick in range(n_ticks):
        pk, recv = np.full((LEGS, K, 172), 0xEE, np.uint8), np.zeros((LEGS, K), np.int32)
        for g in range(LEGS):
            for k in range(K):
                pt = PTS[(2 * g + k + 3 * tick) % 5]
                if pt is None:
                    recv[g, k] = -1 if (g + k) % 2 else 0
                    continue
                recv[g, k] = 172
                pk[g, k, :12] = 0
                pk[g, k, 0], pk[g, k, 1] = 0x80, (0x80 if k % 2 else 0) | pt
                pk[g, k, 2], pk[g, k, 3] = 0x10 + g, 16 * tick + k + 1
                pk[g, k, 12:] = (np.arange(160) + 160 * nth[g] + 37 * g) % 256
                nth[g] += 1
        out.append((pk, recv))
    return out


@pytest.mark.parametrize("aligned", [True, False], ids=["rows_aligned", "rows_unaligned"])
@pytest.mark.parametrize("K", [1, 3, 4])
def test_ingest_per_leg_against_the_model(cuda, oracle_port, wmx, K, aligned):
    import torch
    dec = Decoders(oracle_port)
    snd = senders(LEGS, codecs=CODECS)
    want_refused = np.zeros(LEGS, np.uint32)
    decoded = {"a": set(), "u": set()}
    for tick, (pk, recv) in enumerate(ticks_of(K)):
        want_pcm, want_len, want_seq = ingest(dec, pk, recv, CODECS, want_refused)
        for g in range(LEGS):
            for k in range(K):
                call, law, _ = slot(recv[g, k] > 0, pk[g, k, 1] & 0x7F, CODECS[g])
                if call:
                    decoded[law] |= set(pk[g, k, 12:].tolist())
        drecv = torch.from_numpy(recv).to(cuda)
        if aligned:  # 176-byte rows on a 4-byte boundary, PCM rows on 8-byte boundaries: four codes per lane
            dpk = torch.full((LEGS, K, 176), 0x55, dtype=torch.uint8, device=cuda)
            dpk[:, :, :172] = torch.from_numpy(pk).to(cuda)
            pcm = torch.full((LEGS, K, 160), 1234, dtype=torch.int16, device=cuda)
            assert dpk.data_ptr() % 4 == 0 and pcm.data_ptr() % 8 == 0
        else:  # 173-byte rows from a base pointer off by one byte, PCM rows 161 elements apart: one code per lane, and the gaps stay
            flat = torch.full((LEGS * K * 173 + 1,), 0x55, dtype=torch.uint8, device=cuda)
            dpk = flat[1:].view(LEGS, K, 173)
            dpk[:, :, :172] = torch.from_numpy(pk).to(cuda)
            pcm = torch.full((LEGS, K, 161), 1234, dtype=torch.int16, device=cuda)
            assert dpk.data_ptr() % 4 == 1
        lens = torch.full((LEGS, K), 7, dtype=torch.int32, device=cuda)
        seq = torch.full((LEGS, K), 7, dtype=torch.int16, device=cuda)
        rc = wmx.wmx_rtp_ingest_legs_codecs(snd._h, K, dpk.data_ptr(), dpk.stride(0), dpk.stride(1), drecv.data_ptr(), pcm.data_ptr(), pcm.stride(0),
                                            pcm.stride(1), lens.data_ptr(), seq.data_ptr(), stream())
        assert rc == 0, wmx.wmx_last_error()
        got = pcm.cpu().numpy()
        assert aligned or (got[:, :, 160] == 1234).all()
        assert np.array_equal(lens.cpu().numpy().view(np.uint32), want_len), (tick, lens.cpu().numpy(), want_len)
        assert np.array_equal(seq.cpu().numpy().view(np.uint16), want_seq), tick
        assert np.array_equal(got[:, :, :160], want_pcm), (tick, np.argwhere((got[:, :, :160] != want_pcm).any(2)))
        assert not got[:, :, :160][want_len == 0].any()  # a refused slot is a zeroed row, whatever was there
        st = snd.export_codecs()
        assert np.array_equal(st["refused"], want_refused), (tick, st["refused"], want_refused)  # the second tick counts on
        assert st["in_codec"].tolist() == CODECS and st["out_law"].tolist() == [LAW_A] * LEGS
    assert want_refused.sum() >= 2 and (K == 1 or (want_refused[[1, 2, 4]] > 0).all())  # the other law on the strict legs among them
    if K > 1:
        assert len(decoded["a"]) == 256 and len(decoded["u"]) == 256
    snd.close()


def ring_audio(seed):
    """[RINGS, 1, 4 * 160 + 1]: four packages per ring that hold every G.711 segment boundary of both laws (the A-law ones at
    0x100 << i, 8 lower for negative samples; the mu-law ones 0x84 lower) with its neighbours, +-32767 and -32768"""
    edge = [b + d for b in (0x100 << np.arange(8)).tolist() for d in (-0x85, -0x84, -0x83, -9, -8, -7, -1, 0, 1, 7, 8, 9, 0x83)]
    edge = np.clip(np.array(edge + [-v for v in edge] + [32767, -32767, -32768, 0, -1, 1, -8, 8, 255], np.int64), -32768, 32767).astype(np.int16)
    assert edge.size <= 3 * 160
    rng = np.random.default_rng(seed)
    audio = rng.integers(-32768, 32768, size=(RINGS, 1, 4 * 160 + 1), dtype=np.int16)
    for g in range(RINGS):
        audio[g, 0, :edge.size] = np.roll(edge, 17 * g)  # every ring, so every law, sees every edge inside the three packages played
    return audio


@pytest.mark.parametrize("out_stride", [172, 173], ids=["rows_aligned", "rows_unaligned"])
@pytest.mark.parametrize("start", [0, 4010], ids=["head_on_four_samples", "head_on_an_odd_sample"])
def test_send_with_mixed_laws_is_drain_then_egress_and_the_oracles_senders(cuda, oracle_port, start, out_stride):
    import torch
    from wmix_amd.mix import MixBatch
    assert (start // 2) % 4 == 0 or (start // 2) % 2 == 1
    eg = L._fn(oracle_port, "orc_rtp_egress", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p])
    init = L._fn(oracle_port, "orc_rtp_sender_init", None, [C.c_void_p, C.c_int])
    orc = [(C.c_uint8 * 16)() for _ in range(RINGS)]
    for g in range(RINGS):
        init(orc[g], LAWS[g])
    pair, fused = (MixBatch(RINGS, 1, 8000), senders(RINGS, laws=LAWS)), (MixBatch(RINGS, 1, 8000), senders(RINGS, laws=LAWS))
    src = torch.from_numpy(ring_audio(9)).to(cuda)
    for mb, _ in (pair, fused):
        mb.set_play_correct(0)
        mb.set(start, 0, 1)
        mb.load(src, 4 * 320, 8000, 1)
    for t in range(3):  # seq and timestamp advance
        pcm = pair[0].drain(320)
        want = pair[1].egress(pcm, 1, 8000, 1, 8000).cpu().numpy()
        rows = torch.full((RINGS * out_stride + 4,), 0xEE, dtype=torch.uint8, device=cuda)[:RINGS * out_stride].view(RINGS, out_stride)
        got = fused[1].egress_rings(fused[0], rows[:, :172]).cpu().numpy()
        assert np.array_equal(got, want), (t, np.argwhere(got != want)[:6])
        assert (rows[:, 172:].cpu().numpy() == 0xEE).all()
        played = pcm.cpu().numpy()
        for g in range(RINGS):
            row, out = np.ascontiguousarray(played[g]), np.zeros(172, np.uint8)
            assert eg(orc[g], 1, 8000, row.ctypes.data, 320, 1, 8000, out.ctypes.data) == 172
            assert np.array_equal(got[g], out), ("the oracle's sender", t, g, np.argwhere(got[g] != out)[:6])
            assert got[g, 1] == (0x88 if LAWS[g] == LAW_A else 0x80) and got[g, 2:4].tolist() == [0, t]
            a, b = pair[0].export(g), fused[0].export(g)
            assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], ("ring / head / tick", t, g)
            assert pair[1].state(g) == fused[1].state(g) == (t + 1, 160 * (t + 1)), ("seq / timestamp", t, g)
    assert not np.array_equal(got[0, 12:], got[1, 12:])  # the same samples (rolled) in two laws
    # the plain egress kernel too (rows off the 4-byte boundary): per stream law there as well
    pcm = torch.from_numpy(ring_audio(10)[:, 0, :160].copy()).to(cuda)
    rows = torch.full((RINGS, 173), 0xEE, dtype=torch.uint8, device=cuda)
    got = pair[1].egress(pcm, 1, 8000, 1, 8000, rows).cpu().numpy()
    for g in range(RINGS):
        row, out = np.ascontiguousarray(pcm[g].cpu().numpy()), np.zeros(172, np.uint8)
        assert eg(orc[g], 1, 8000, row.ctypes.data, 320, 1, 8000, out.ctypes.data) == 172
        assert np.array_equal(got[g], out), ("the oracle's sender, rows unaligned", g)
    for mb, snd in (pair, fused):
        mb.close()
        snd.close()


def test_refusals_change_nothing(cuda, wmx):
    snd = senders(LEGS, codecs=CODECS, laws=LAWS[:LEGS])
    before = snd.export_codecs()
    assert before["in_codec"].tolist() == CODECS and before["out_law"].tolist() == LAWS[:LEGS] and not before["refused"].any()
    bad, good = np.array([1, LEGS], np.int32), np.array([1, 2], np.int32)
    assert wmx.wmx_rtp_set_codecs(snd._h, bad.ctypes.data, 2, PCMA, LAW_A, stream()) == EINVAL and b"outside" in wmx.wmx_last_error()
    assert wmx.wmx_rtp_set_codecs(snd._h, np.array([-1], np.int32).ctypes.data, 1, PCMA, LAW_A, stream()) == EINVAL
    assert wmx.wmx_rtp_set_codecs(snd._h, good.ctypes.data, 2, 4, LAW_A, stream()) == EINVAL
    assert wmx.wmx_rtp_set_codecs(snd._h, good.ctypes.data, 2, -1, LAW_A, stream()) == EINVAL
    assert wmx.wmx_rtp_set_codecs(snd._h, good.ctypes.data, 2, PCMA, 2, stream()) == EINVAL
    assert wmx.wmx_rtp_set_codecs(snd._h, None, 0, 4, LAW_A, stream()) == EINVAL and wmx.wmx_rtp_set_codecs(snd._h, None, 0, PCMA, 2, stream()) == EINVAL
    assert wmx.wmx_rtp_set_codecs(None, None, 0, PCMA, LAW_A, stream()) == EINVAL
    assert wmx.wmx_rtp_export_codecs(None, None, None, None, stream()) == EINVAL
    assert wmx.wmx_rtp_ingest_legs_codecs(None, 3, None, 0, 0, None, None, 0, 0, None, None, stream()) == EINVAL
    after = snd.export_codecs()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    assert wmx.wmx_rtp_export_codecs(snd._h, None, None, None, stream()) == 0  # any pointer may be NULL
    snd.close()
    fresh = senders(3, law="u").export_codecs()  # a handle that was never told anything
    assert fresh["in_codec"].tolist() == [REFERENCE] * 3 and fresh["out_law"].tolist() == [LAW_U] * 3 and not fresh["refused"].any()


def test_back_to_the_default_is_a_handle_that_was_never_told_anything(cuda, oracle_port):
    """wmx_rtp_set_codecs(all, REFERENCE, the law of create) after mixed codecs: ingest and send give the bytes of a fresh handle, and of
    the stateless wmx_rtp_ingest_legs; reset_streams and reset_sequence keep a stream's codec"""
    import torch
    from wmix_amd import rtp
    from wmix_amd.mix import MixBatch
    K = 3
    pk, recv = ticks_of(K)[0]
    dpk, drecv = torch.from_numpy(pk).to(cuda), torch.from_numpy(recv).to(cuda)
    told, never = senders(LEGS, codecs=CODECS, laws=LAWS[:LEGS], law="u"), senders(LEGS, law="u")
    mixed = told.ingest_legs(dpk, drecv)
    told.reset_streams([1, 2])
    told.reset_sequence([2])
    st = told.export_codecs()
    assert st["in_codec"].tolist() == CODECS and st["out_law"].tolist() == LAWS[:LEGS]
    assert st["refused"][2] == 0 and st["refused"][[1, 4]].all()  # reset_sequence zeroes the leg's receive counters, this one among them
    told.set_codecs(None, REFERENCE, LAW_U)
    plain = rtp.ingest_legs(dpk, drecv)
    a, b = told.ingest_legs(dpk, drecv), never.ingest_legs(dpk, drecv)
    for x, y, z in zip(a, b, plain):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy()) and np.array_equal(x.cpu().numpy(), z.cpu().numpy())
    assert not np.array_equal(mixed[0].cpu().numpy(), a[0].cpu().numpy())  # the mu-law legs were decoded otherwise
    want = ingest(Decoders(oracle_port), pk, recv, [REFERENCE] * LEGS)
    assert np.array_equal(a[0].cpu().numpy(), want[0]) and np.array_equal(a[1].cpu().numpy().view(np.uint32), want[1])
    src = torch.from_numpy(ring_audio(11)[:LEGS]).to(cuda)
    sent = []
    for snd in (told, never):
        mb = MixBatch(LEGS, 1, 8000)
        mb.set_play_correct(0)
        mb.load(src, 320, 8000, 1)
        sent.append(snd.egress_rings(mb).cpu().numpy())
        mb.close()
    assert np.array_equal(sent[0], sent[1]) and (sent[0][:, 1] == 0x80).all()
    told.close()
    never.close()
