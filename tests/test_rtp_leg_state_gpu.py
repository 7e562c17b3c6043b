"""The per-leg state tables of the bridge (wmix_amd/csrc/leg_state.h: one table of columns per rule, made on first use, reset for a
list of legs or for all, exported) through the Python mirror.  wmx_rtp: the senders' seq / timestamp and the sequence, codec,
concealment and DTMF rule's state of 1, 5 (odd: every column behind the first starts off the wider grid) and 9 legs (one more than a
block of the DTMF kernel).  wmx_mix: the cursor per leg and the talkers' envelopes of 2, 5 and 9 legs.  wmx_conf: the gate's two
counters of 5 legs.  What the rules compute is the per-rule files' to check against their models; here a fixed script moves every
exported column of every leg, and the exports are compared with themselves and with the documented defaults around resets.
Integers, np.array_equal."""
import numpy as np
import pytest

from conf_harness import bridge, run
from conf_inputs import EINVAL, NULL_HEAD

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


# ---- the mixer's two tables: head, tick and dropped of the cursor per leg; env and speaking of talker selection
MIX_FRESH = {"head": NULL_HEAD, "tick": 0, "dropped": 0, "env": 0, "speaking": 0}


def mix_exports(mb):
    head, tick, dropped = mb.export_leg_cursors()
    speaking, env = mb.export_speakers()
    return {"head": head, "tick": tick, "dropped": dropped, "env": env, "speaking": speaking}


@pytest.mark.parametrize("n,layout", [(2, [[0, 1]]), (5, [[0, 1], [2, 3, 4]]), (9, [[0, 1, 2, 3], [4, 5, 6, 7, 8]])])
def test_the_mixers_cursors_and_envelopes_around_resets(cuda, wmx, n, layout):
    import torch
    from wmix_amd.mix import MixBatch
    mb = MixBatch(n, 1, 8000)
    mb.set_conferences(layout)
    everyone = np.arange(n)
    for k, v in mix_exports(mb).items():
        assert (v == MIX_FRESH[k]).all(), ("before any state exists", k, v)
    # rows of 160 samples, four packets per leg per load and no drain: the rings fill, and every leg drops calls
    rows = np.zeros((n, K, 168), np.int16)  # a row's 160 samples and room behind them for the load's look-ahead frame
    rows[..., :160] = np.random.default_rng(n).integers(2000, 20000, (n, K, 160)) * np.where(np.arange(160) % 2, 1, -1)
    src, lens = torch.from_numpy(rows).to(cuda), torch.full((n, K), 320, dtype=torch.int32, device=cuda)
    bound = mb.ring_bytes // 320 + 2
    for load in range(bound):
        mb.select_speakers_legs(src, 320, lens, 2)
        mb.load_minus_legs(src, 320, 8000, 1, lens)
        if mb.export_leg_cursors()[2].all():
            break
    else:
        pytest.fail("a leg has dropped nothing after %d loads" % bound)
    moved = mix_exports(mb)
    print("loads", load + 1, {k: v.tolist() for k, v in moved.items()})
    assert all((moved[k] != MIX_FRESH[k]).all() for k in ("head", "tick", "dropped", "env")) and moved["speaking"].any()

    stream = torch.cuda.current_stream().cuda_stream
    bad = np.array([0, n], np.int32)
    for f in (wmx.wmx_mix_reset_leg_cursors, wmx.wmx_mix_reset_speakers):
        assert f(mb._h, bad.ctypes.data, 2, stream) == EINVAL and b"%d is outside the mixer's %d" % (n, n) in wmx.wmx_last_error()
    after = mix_exports(mb)
    assert all(np.array_equal(moved[k], after[k]) for k in moved), "a refused reset changed something"

    some = [g for g in (1, 3) if g < n]
    others = np.setdiff1d(everyone, some)
    mb.reset_leg_cursors(some)
    mb.reset_speakers(some)
    after = mix_exports(mb)
    for k in moved:
        assert np.array_equal(after[k][others], moved[k][others]), ("a reset of", some, "changed", k, "of another leg")
        if k != "speaking":
            assert (after[k][some] == MIX_FRESH[k]).all(), ("the legs reset", k, after[k][some])
    assert np.array_equal(after["speaking"], moved["speaking"])  # the next selection's to write: no reset touches it

    mb.reset_leg_cursors()
    mb.reset_speakers()
    after = mix_exports(mb)
    assert all((after[k] == MIX_FRESH[k]).all() for k in ("head", "tick", "dropped", "env")) and np.array_equal(after["speaking"], moved["speaking"])
    mb.close()


# ---- the conference handle's table: the gate's two counters, beside the gate's own `reduce`
GATE_FRESH = {"reduce": 4, "voiced": 0, "unvoiced": 0}


def test_the_handles_gate_counters_around_resets(cuda, wmx):
    n, ticks = 5, 3
    cb = bridge(n, 3, [list(range(n))], 1)
    for k, v in cb.export_gate().items():
        assert (v == GATE_FRESH[k]).all(), ("before the first switch-on", k, v)
    cb.gate(True)
    rng = np.random.default_rng(5)
    pk, recv = np.zeros((ticks, n, 1, 172), np.uint8), np.full((ticks, n, 1), 172, np.int32)
    for t in range(ticks):
        for g in range(n):
            pk[t, g, 0] = packet(8, 100 + g + t, 160 * t, g)
            pk[t, g, 0, 12:] = rng.integers(0, 256, 160)  # random codes: loud, and voice to the gate
    run(cb, pk, recv, "wait")
    moved = cb.export_gate()
    print({k: v.tolist() for k, v in moved.items()})
    # one row per leg and tick: every row was judged one way or the other, and a gate that has heard voice has begun to open
    assert (moved["voiced"].astype(np.int64) + moved["unvoiced"] == ticks).all() and moved["voiced"].all() and (moved["reduce"] < 4).all()

    bad = np.array([0, n], np.int32)
    assert wmx.wmx_conf_reset_legs(cb._h, bad.ctypes.data, 2, cb._stream()) == EINVAL
    assert b"wmx_conf_reset_legs: leg %d is outside the handle's %d" % (n, n) in wmx.wmx_last_error()
    after = cb.export_gate()
    assert all(np.array_equal(moved[k], after[k]) for k in moved), "a refused reset changed something"

    some, others = [1, 3], [0, 2, 4]
    cb.reset_legs(some)
    after = cb.export_gate()
    for k in moved:
        assert np.array_equal(after[k][others], moved[k][others]), ("a reset of", some, "changed", k, "of another leg")
        assert (after[k][some] == GATE_FRESH[k]).all(), ("the legs reset", k, after[k][some])

    cb.reset_legs()
    for k, v in cb.export_gate().items():
        assert (v == GATE_FRESH[k]).all(), ("every leg reset", k, v)
    cb.close()
