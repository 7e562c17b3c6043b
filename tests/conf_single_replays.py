"""The single-purpose replays of the conference tests, each written when its stage came: the whole-script replay the C examples are
held against, and tick by tick the layout / mute / new-call replay, sequencing, concealment, a codec per leg, and a codec per leg
sequenced and selected.  They are independent texts of what ConfReplay (tests/conf_replay_model.py) composes, and
tests/test_conf_replay_model.py anchors the composed model against every one of them: they are not written in terms of it."""
import ctypes as C

import numpy as np

from conf_inputs import CHANGE_AT, G, LATER_ULAW_LEG, LAYOUT, RESET_AT, RESET_LEG, T, rewritten_script, seq_raw_of
from conf_stories import start
from leg_codec_model import LAW_U, PCMU
from leg_oracle_model import CodecReplay, LegsOracle, Replay
from leg_plc_model import LegsPlcModel
from leg_seq_model import LegsSeqModel, repaired_rows
from oracle import loader as L
from speakers_legs_model import SpeakersLegsModel


def replay(lib, pk, recv, layout, platform):
    """the oracle's ingest, one reference ring per leg with a cursor per source leg, the drain and the oracle's egress over the whole
    script -> (datagrams [T, G, 172], the load calls made)"""
    T, G = recv.shape[:2]
    ing = L._fn(lib, "orc_rtp_ingest", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    eg = L._fn(lib, "orc_rtp_egress", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p])
    senders = [(C.c_uint8 * 16)() for _ in range(G)]
    for s in senders:
        L._fn(lib, "orc_rtp_sender_init", None, [C.c_void_p, C.c_int])(s, 0)
    orc = LegsOracle(lib, G, (1, 8000), 1, L.PLATFORMS[platform][1])
    out = np.zeros((T, G, 172), np.uint8)
    calls = 0
    for t in range(T):
        pcm, lens = np.zeros((G, 3, 161), np.int16), np.zeros((G, 3), np.uint32)
        for g in range(G):
            for k in range(3):
                if recv[t, g, k] > 0:
                    row, dec = np.ascontiguousarray(pk[t, g, k]), np.zeros(160, np.int16)
                    lens[g, k] = ing(row.ctypes.data, dec.ctypes.data, None)
                    pcm[g, k, :160] = dec
        calls += int((lens == 320).sum())
        orc.load(layout, pcm, lens, 320, 8000, 1, 160, None)
        play = orc.drain()
        for g in range(G):
            row = np.ascontiguousarray(play[g])
            assert eg(senders[g], 1, 8000, row.ctypes.data, 320, 1, 8000, out[t, g].ctypes.data) == 172
    return out, calls


def replay_with(lib, pk, recv, layout_at, mute_at=None, fresh_at=None, select=None):
    """-> (datagrams [T, n, 172], per tick (speaking, env) when `select` = (max_speakers, floor, shift) is given)"""
    n = recv.shape[1]
    rp, model, out, sel = Replay(lib, n), SpeakersLegsModel(n), np.zeros((recv.shape[0], n, 172), np.uint8), []
    for t in range(recv.shape[0]):
        if fresh_at and t in fresh_at:
            rp.fresh(fresh_at[t])
            model.reset(fresh_at[t])
        pcm, lens = rp.decode(pk[t], recv[t])
        mute = mute_at(t) if mute_at else None
        if select:
            sp, mute = model.step_legs(layout_at(t), pcm, lens, 320, select[0], select[1], select[2], mute)
            sel.append((sp.copy(), model.env.copy()))
        out[t] = rp.tick(pcm, lens, layout_at(t), mute)
    return out, sel


def replay_seq(lib, pk, recv, max_gap=3, fresh_at=None, select=None, rewrite=True):
    """the tick-by-tick replay fed the model's repaired rows -> (datagrams [T, G, 172], the model, per tick (speaking, env)).
    rewrite=False: the selection is fed the lens as ingest left them (what the device must NOT do)"""
    rp, model, spk = Replay(lib, G), LegsSeqModel(G), SpeakersLegsModel(G)
    out, sel = np.zeros((T, G, 172), np.uint8), []
    for t in range(T):
        if fresh_at and t in fresh_at:
            rp.fresh(fresh_at[t])
            model.reset(fresh_at[t])
            spk.reset(fresh_at[t])
        pcm, lens = rp.decode(pk[t], recv[t])
        _, new_lens, lists = model.tick(seq_raw_of(pk[t], recv[t]), lens, max_gap)
        mute = None
        if select:
            sp, mute = spk.step_legs(LAYOUT, pcm, new_lens if rewrite else lens, 320, select[0], select[1], select[2], None)
            sel.append((sp.copy(), spk.env.copy()))
        rows, rlens = repaired_rows(pcm, lists)
        out[t] = rp.tick(rows, rlens, LAYOUT, mute)
    return out, model, sel


def replay_conceal(lib, pk, recv, max_gap=3, fresh_at=None, plc_fresh=True):
    """the tick-by-tick replay fed the concealment model's rows -> (datagrams [ticks, G, 172], the sequence model, the concealment
    model, the replay).  plc_fresh=False: a reset leaves the concealment state as it was (what the device must NOT do)"""
    rp, seq, plc = Replay(lib, G), LegsSeqModel(G), LegsPlcModel(G)
    out = np.zeros((recv.shape[0], G, 172), np.uint8)
    for t in range(recv.shape[0]):
        if fresh_at and t in fresh_at:
            rp.fresh(fresh_at[t])
            seq.reset(fresh_at[t])
            if plc_fresh:
                plc.reset(fresh_at[t])
        pcm, lens = rp.decode(pk[t], recv[t])
        _, new_lens, lists = seq.tick(seq_raw_of(pk[t], recv[t]), lens, max_gap)
        rows, rlens = plc.tick(pcm, new_lens, lists)
        wide = np.zeros((G, 4, 161), np.int16)  # the oracle's look-ahead element
        wide[:, :, :160] = rows
        out[t] = rp.tick(wide, rlens, LAYOUT)
    return out, seq, plc, rp


def codec_story(lib):
    """the script, every datagram the replay sends, its codec state at the end and leg 6's refused count in front of its reset"""
    pk, recv = rewritten_script()
    rp, out, seen = CodecReplay(lib, G), np.zeros((T, G, 172), np.uint8), {}
    start(rp)
    for t in range(T):
        if t == CHANGE_AT:
            rp.set_codecs([LATER_ULAW_LEG], PCMU, LAW_U)
        if t == RESET_AT:
            seen["refused_before_reset"] = int(rp.refused[RESET_LEG])
            rp.fresh([RESET_LEG])
        pcm, lens = rp.decode(pk[t], recv[t])
        out[t] = rp.tick(pcm, lens, LAYOUT)
    return pk, recv, out, rp, seen


def replay_sequenced(lib, pk, recv, select, codecs):
    """the replay with sequence(True, 3) and speakers(*select); codecs: the legs as START sets them, else every leg at the default
    -> (datagrams, the sequence model, per tick (speaking, env), the replay)"""
    rp, model, spk = CodecReplay(lib, G), LegsSeqModel(G), SpeakersLegsModel(G)
    if codecs:
        start(rp)
    out, sel = np.zeros((T, G, 172), np.uint8), []
    for t in range(T):
        pcm, lens = rp.decode(pk[t], recv[t])
        _, new_lens, lists = model.tick(seq_raw_of(pk[t], recv[t]), lens, 3)
        sp, mute = spk.step_legs(LAYOUT, pcm, new_lens, 320, select[0], select[1], select[2], None)
        sel.append((sp.copy(), spk.env.copy()))
        rows, rlens = repaired_rows(pcm, lists)
        out[t] = rp.tick(rows, rlens, LAYOUT, mute)
    return out, model, sel, rp
