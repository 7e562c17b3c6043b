"""wmx_rtp_ingest_legs (wmix_amd/csrc/rtp.hip) against the oracle's ingest slot by slot: the receive loop's `ret > 0 && retSize > 0`
(src/wmixTask.c:1278-1284) for legs that deliver up to three datagrams in a tick.  Integer results, np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from oracle import loader as L

pytestmark = pytest.mark.gpu

LEGS, SLOTS = 8, 3


def slots(seed):
    """datagram rows [LEGS, SLOTS, 172] with random payloads, and what recvfrom returned per slot: PCMA and PCMU datagrams, a foreign
    payload type and an AAC one, slots where nothing arrived (0, -1: EAGAIN) -- in the middle of a burst too -- and a short datagram"""
    rng = np.random.default_rng(seed)
    pk = rng.integers(0, 256, size=(LEGS, SLOTS, 172), dtype=np.uint8)
    pk[:, :, 0] = 0x80
    pk[:, :, 1] = 0x88                   # m = 1, pt 8: PCMA
    recv = np.full((LEGS, SLOTS), 172, np.int32)
    pk[1, :, 1] = 0x00                   # pt 0: PCMU, no marker
    pk[2, 1, 1] = 0x80 | 96              # a foreign payload type between two PCMA datagrams
    pk[3, 0, 1] = 97                     # AAC
    recv[4, :] = 0                       # nothing in the tick
    recv[5, 1] = -1                      # a hole in a burst
    recv[6, 0], recv[6, 2] = -1, 0       # only the middle slot
    recv[7, 2] = 40                      # a short datagram: the reference decodes what lies in its buffer
    return pk, recv


def oracle_slots(lib, pk, recv):
    ing = L._fn(lib, "orc_rtp_ingest", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    pcm, lens, seq = np.zeros((LEGS, SLOTS, 160), np.int16), np.zeros((LEGS, SLOTS), np.int32), np.zeros((LEGS, SLOTS), np.uint16)
    for r in range(LEGS):
        for k in range(SLOTS):
            if recv[r, k] <= 0:
                continue
            row, out, s = np.ascontiguousarray(pk[r, k]), np.zeros(160, np.int16), C.c_uint16(0)
            lens[r, k] = ing(row.ctypes.data, out.ctypes.data, C.byref(s))
            seq[r, k] = s.value
            pcm[r, k] = out  # zero where the oracle decoded nothing
    return pcm, lens, seq


@pytest.mark.parametrize("aligned", [True, False])
def test_ingest_legs_against_the_oracle_per_slot(cuda, oracle_port, wmx, aligned):
    import torch
    from wmix_amd import rtp
    pk, recv = slots(11)
    want_pcm, want_len, want_seq = oracle_slots(oracle_port, pk, recv)
    assert set(want_len.ravel()) == {0, 320} and want_len[2].tolist() == [320, 0, 320] and want_len[3, 0] == 0 and want_len[7, 2] == 320
    drecv = torch.from_numpy(recv).to(cuda)
    if aligned:  # rows on 4 / 8-byte boundaries: four codes per lane
        pcm, lens, seq = rtp.ingest_legs(torch.from_numpy(pk).to(cuda), drecv, look_ahead=4)
        assert not pcm[:, :, 160:].any()
        pcm = pcm[:, :, :160]
    else:  # datagram rows 173 bytes apart, PCM rows 161 elements apart, both pre-filled: one code per lane, and the gaps stay
        dpk = torch.full((LEGS, SLOTS, 173), 0x55, dtype=torch.uint8, device=cuda)
        dpk[:, :, :172] = torch.from_numpy(pk).to(cuda)
        pcm = torch.full((LEGS, SLOTS, 161), 1234, dtype=torch.int16, device=cuda)
        lens = torch.full((LEGS, SLOTS), 7, dtype=torch.int32, device=cuda)
        seq = torch.full((LEGS, SLOTS), 7, dtype=torch.int16, device=cuda)
        rc = wmx.wmx_rtp_ingest_legs(LEGS, SLOTS, dpk.data_ptr(), dpk.stride(0), dpk.stride(1), drecv.data_ptr(), pcm.data_ptr(), pcm.stride(0),
                                     pcm.stride(1), lens.data_ptr(), seq.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        assert bool((pcm[:, :, 160] == 1234).all())
        pcm = pcm[:, :, :160]
    assert np.array_equal(lens.cpu().numpy(), want_len)
    assert np.array_equal(seq.cpu().numpy().view(np.uint16), want_seq)
    got = pcm.cpu().numpy()
    assert np.array_equal(got, want_pcm)
    # a slot that made no call has a zeroed row, whatever its datagram row held
    assert not got[want_len == 0].any() and got[want_len == 320].any(1).all()


def test_ingest_legs_refusals(cuda, wmx):
    import torch
    pk = torch.zeros((2, 3, 172), dtype=torch.uint8, device=cuda)
    recv = torch.zeros((2, 3), dtype=torch.int32, device=cuda)
    pcm = torch.zeros((2, 3, 160), dtype=torch.int16, device=cuda)
    lens = torch.zeros((2, 3), dtype=torch.int32, device=cuda)

    def call(n=2, k=3, p=pk.data_ptr(), ls=3 * 172, ps=172, r=recv.data_ptr(), o=pcm.data_ptr(), ss=3 * 160, os_=160, ln=lens.data_ptr()):
        return wmx.wmx_rtp_ingest_legs(n, k, p, ls, ps, r, o, ss, os_, ln, None, None)

    assert call() == 0 and call(n=0) == 0
    for bad in (dict(k=0), dict(k=5), dict(p=None), dict(r=None), dict(o=None), dict(ln=None), dict(ps=171), dict(os_=159), dict(ls=2 * 172),
                dict(ss=2 * 160), dict(n=-1)):
        assert call(**bad) == -10001, bad
    torch.cuda.synchronize()
