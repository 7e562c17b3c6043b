"""The codec rule of an RTP leg, written from its table (include/wmix_amd.h, "A G.711 codec per stream") and not from
wmix_amd/csrc/leg_codec.h: what tests/test_leg_codec_host.py holds the header against and the GPU tests the kernels.

    arrived = recvfrom returned > 0;  pt = header byte 1 & 0x7F;  g711 = arrived and pt in (8, 0)
    REFERENCE 0   a call when g711               decoded as A-law
    PCMA      1   a call when g711 and pt == 8   decoded as A-law
    PCMU      2   a call when g711 and pt == 0   decoded as mu-law
    BY_PT     3   a call when g711               mu-law if pt == 0, else A-law
    refused = arrived and not call
"""
import ctypes as C

import numpy as np

REFERENCE, PCMA, PCMU, BY_PT = 0, 1, 2, 3
LAW_A, LAW_U = 0, 1
TABLE = {  # in_codec: {payload type that makes a call: the law it is decoded with}
    REFERENCE: {8: "a", 0: "a"},
    PCMA: {8: "a"},
    PCMU: {0: "u"},
    BY_PT: {8: "a", 0: "u"},
}


def slot(arrived, pt, in_codec):
    """-> (call, law "a" / "u" / None, refused)"""
    law = TABLE[in_codec].get(pt) if arrived else None
    return law is not None, law, bool(arrived) and law is None


def out_pt(out_law):
    return {LAW_A: 8, LAW_U: 0}[out_law]


class Decoders:
    """the oracle's two decoders over 160 codes (orc_G711a2PCM, orc_G711u2PCM)"""

    def __init__(self, lib):
        from oracle import loader as L
        sig = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        self.dec = {"a": L._fn(lib, "orc_G711a2PCM", C.c_int, sig), "u": L._fn(lib, "orc_G711u2PCM", C.c_int, sig)}

    def __call__(self, law, codes):
        src, out = np.ascontiguousarray(codes, dtype=np.uint8), np.zeros(len(codes), np.int16)
        assert self.dec[law](src.ctypes.data, out.ctypes.data, len(codes), 0) == 2 * len(codes)
        return out


def ingest(dec, pk, recv, in_codec, refused=None):
    """what wmx_rtp_ingest_legs_codecs leaves for datagram rows pk [legs, K, >= 172] and recv [legs, K] under in_codec [legs]:
    (pcm int16 [legs, K, 160], lens uint32 [legs, K], seq_raw uint16 [legs, K]); refused [legs] (uint32) is counted on in place"""
    n, k = recv.shape
    pcm, lens, seq = np.zeros((n, k, 160), np.int16), np.zeros((n, k), np.uint32), np.zeros((n, k), np.uint16)
    for g in range(n):
        for j in range(k):
            arrived = recv[g, j] > 0
            call, law, ref = slot(arrived, int(pk[g, j, 1]) & 0x7F, int(in_codec[g]))
            if arrived:
                seq[g, j] = int(pk[g, j, 2]) | (int(pk[g, j, 3]) << 8)
            if call:
                pcm[g, j], lens[g, j] = dec(law, pk[g, j, 12:172]), 320
            if ref and refused is not None:
                refused[g] += 1
    return pcm, lens, seq
