"""The per-leg state of wmx_rtp (wmix_amd/csrc/rtp.hip: one table of columns per rule, made on first use, reset for a list of legs or
for all, exported) through the Python mirror: the senders' seq / timestamp and the sequence, codec, concealment and DTMF rule's state
of 1, 5 (odd: every column behind the first starts off the wider grid) and 9 legs (one more than a block of the DTMF kernel).  What
the rules compute is the per-rule files' to check against their models; here a fixed script of three ticks moves every exported
column of every leg, and the exports are compared with themselves and with the documented defaults around resets.  Integers,
np.array_equal."""
import numpy as np
import pytest

from conf_inputs import EINVAL

pytestmark = pytest.mark.gpu

K, EVENT_PT = 4, 101


def packet(pt, seq, ts, leg):
    p = np.zeros(172, np.uint8)
    p[0], p[1], p[2], p[3] = 0x80, pt, seq >> 8, seq & 0xFF
    p[4:8] = [(ts >> s) & 0xFF for s in (24, 16, 8, 0)]
    p[12:] = (np.arange(160) * 7 + 13 * leg + seq) % 120 + 8  # codes that decode to something, another row per leg and packet
    return p


def script(n):
    """-> per tick (packets uint8 [n, K, 172], recv int32 [n, K]).  Leg g's sender counts from b = 100 + g.
    tick 0: b, b + 1 and a telephone event (refused by the audio path, reported as a digit): the leg syncs
    tick 1: b + 1 again (late), b + 2 twice (dup), b + 4 (b + 3 lost: a silence call, concealed)
    tick 2: b + 25 (a restart: resync), b + 28 (two lost) and b + 30, which no longer fits in four calls (overflow)"""
    ticks = []
    for t in range(3):
        pk, recv = np.zeros((n, K, 172), np.uint8), np.zeros((n, K), np.int32)
        for g in range(n):
            b = 100 + g
            rows = [[(8, b), (0, b + 1), (EVENT_PT, 7)], [(8, b + 1), (0, b + 2), (8, b + 2), (8, b + 4)], [(8, b + 25), (0, b + 28), (8, b + 30)]][t]
            for k, (pt, seq) in enumerate(rows):
                pk[g, k], recv[g, k] = packet(pt, seq, 160 * seq + 1, g), 172
                if pt == EVENT_PT:
                    pk[g, k, 12] = 1 + g % 9  # the event: a digit
        ticks.append((pk, recv))
    return ticks


def exports(snd):
    r = {}
    for name, part in (("sequence", snd.export_sequence()), ("codecs", snd.export_codecs()), ("conceal", snd.export_conceal()),
                       ("dtmf", snd.export_dtmf())):
        r.update({name + "." + k: v for k, v in part.items()})
    sent = np.array([snd.state(g) for g in range(snd.n)], np.int64)
    r["send.seq"], r["send.timestamp"] = sent[:, 0], sent[:, 1]
    return r


def assert_fresh(r, legs, law, in_codec, what):
    """the documented defaults; the codecs are the leg's own, not state a reset of a leg touches"""
    for k, v in r.items():
        want = {"codecs.in_codec": in_codec, "codecs.out_law": law}.get(k, 0)
        assert (v[legs] == want).all(), (what, k, v[legs])


def run_script(snd, n, cuda):
    import torch
    for pk, recv in script(n):
        packets, recv_d = torch.from_numpy(pk).to(cuda), torch.from_numpy(recv).to(cuda)
        pcm, lens, seq_raw = snd.ingest_legs(packets, recv_d)
        calls = snd.sequence_legs(seq_raw, lens)
        snd.detect_dtmf_legs(packets, recv_d, pcm, lens, calls, event_pt=EVENT_PT)
        snd.conceal_legs(pcm, lens, calls)
        snd.egress(pcm[:, 0, :].contiguous(), 1, 8000, 1, 8000)


@pytest.mark.parametrize("n", [1, 5, 9])
def test_defaults_then_resets_of_some_legs_of_all_and_of_a_bad_index(cuda, wmx, n):
    import torch
    from wmix_amd.rtp import RtpSenders
    snd = RtpSenders(n, law="u")
    everyone = np.arange(n)
    assert_fresh(exports(snd), everyone, 1, 0, "before any state exists")  # WMX_CODEC_REFERENCE and the law of create
    snd.set_codecs(None, "by_pt", "a")
    run_script(snd, n, cuda)
    moved = exports(snd)
    for k, v in moved.items():  # the script did what it is for: every column of every leg has left its default
        if k not in ("codecs.out_law",):  # WMX_LAW_A is 0
            assert v.reshape(n, -1).any(axis=1).all(), (k, v)
    assert (moved["codecs.in_codec"] == 3).all() and (moved["codecs.out_law"] == 0).all()

    resets = [wmx.wmx_rtp_reset_streams, wmx.wmx_rtp_reset_sequence, wmx.wmx_rtp_reset_conceal, wmx.wmx_rtp_reset_dtmf]
    stream = torch.cuda.current_stream().cuda_stream
    bad = np.array([0, n], np.int32)
    assert [f(snd._h, bad.ctypes.data, 2, stream) for f in resets] == [EINVAL] * 4
    after = exports(snd)
    assert all(np.array_equal(moved[k], after[k]) for k in moved), "a refused reset changed something"

    some = [1, 3] if n > 1 else [0]
    others = np.setdiff1d(everyone, some)
    for reset in (snd.reset_streams, snd.reset_sequence, snd.reset_conceal, snd.reset_dtmf):
        reset(some)
    after = exports(snd)
    for k in moved:
        assert np.array_equal(after[k][others], moved[k][others]), ("a reset of", some, "changed", k, "of another leg")
    assert_fresh(after, some, 0, 3, "the legs reset")  # in_codec / out_law are kept, refused is zeroed by wmx_rtp_reset_sequence

    for reset in (snd.reset_streams, snd.reset_sequence, snd.reset_conceal, snd.reset_dtmf):
        reset()
    assert_fresh(exports(snd), everyone, 0, 3, "every leg reset")
    snd.close()
