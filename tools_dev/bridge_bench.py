"""bridge_bench.py -- what the conference bridge costs, one JSON line.

1. wmx_mix_load_minus against what a user without it has to do for the same rings: gather the P - 1 foreign sources of every ring into
   a staging tensor (torch indexing) and one wmx_mix_load(n_src = P - 1) on the same mixer.  Both results are compared on sampled
   conferences before any time is reported.  Device events around every repetition, the two sides alternating; per side the median
   and the spread of the medians of 5 consecutive blocks of repetitions (what "the same thing measured again" gives in this run).
2. The bridge tick with all four stages beside the same wmx_tick with the bridge off: the difference is the bridge's cost per tick.

Bytes of the new call, from shapes: every ring column reads P sources, reads P ring samples and writes P ring samples, 2 B each.

    python tools_dev/bridge_bench.py [--sizes 4096x8x8000,65536x8x16000] [--reps 200] [--tick 4096x8] [--out file.json]

--ragged measures the bridge over a layout (wmx_mix_load_minus_conf) instead, for the leg counts of --sizes:
a. the same legs both ways: equal consecutive conferences of P = 4 and P = 32 through the layout against wmx_mix_load_minus (the untouched
   uniform kernel of the same build) on the same rings; compared on sampled rings before any time is reported.
b. a telephony mix of 4 096 conferences (70 % of 2 legs, 20 % of 3, 8 % of 4 - 8, 2 % of 9 - 32) through the layout against what a caller
   without it has to do: every conference padded to 32 with muted legs through wmx_mix_load_minus.  The load time per tick and the rings
   (= FIFO rows = chain streams) the layout saves.
Device events around every repetition; they include the host's work between the launches (the cursor rule over every conference).

    python tools_dev/bridge_bench.py --ragged --out profiles/bridge/bridge_ragged_bench.json

--speakers N measures the talker selection (wmx_mix_select_speakers, with --ragged wmx_mix_select_speakers_conf) on the same shapes: per
tick the selection alone, the bridge load alone over every leg (the load kernels are what they were before the selection existed), and
the selection followed by the load it feeds (the load then skips the sources of the legs that are not speaking).  The mask of the first
call is compared with numpy's ranking of the rows' levels before any time is reported; the sides alternate, device events around each.

    python tools_dev/bridge_bench.py --speakers 3 --out profiles/bridge/bridge_speakers_bench.json
    python tools_dev/bridge_bench.py --speakers 3 --ragged --out profiles/bridge/bridge_speakers_ragged_bench.json

--legs measures the bridge load with a cursor per leg (wmx_mix_load_minus_legs) on the telephony mix of --ragged, beside
wmx_mix_load_minus_conf on the same layout in the same run: (a) steady arrivals, one valid packet per leg and tick, max_packets 1 -- the
rings of the first call are compared with the common-cursor load's before any time is reported; (b) a jittered script, max_packets 3
(per leg and tick 1/4 nothing, 1/8 two at once, 1/8 two with an invalid slot between them, 1/2 one; a cycle of 16 ticks).  Every
repetition moves every side's play head on by one package first (host state only, no launch), so that the legs' cursors neither run
into the overrun bound nor fall behind for good.  The sides alternate, device events around each.

    python tools_dev/bridge_bench.py --legs --out profiles/bridge/bridge_legs_bench.json

--pipe measures the bridge of RTP/G.711 legs end to end on the telephony mix of --ragged, datagrams from and to host memory, milliseconds
of wall clock per tick over blocks of ticks, three ways in one process, the sides alternating block by block: (a) the composition
examples/host_tick.c --bridge-rtp makes -- blocking copies, wmx_rtp_ingest_legs, wmx_mix_load_minus_legs on a tick's mixer, wmx_tick_play,
wmx_rtp_egress; (b) wmx_conf with 3 slots, the arrivals already in the slots' pinned rows (a host's recvfrom writes there), the datagrams
read where they land; (c) wmx_conf_step_resident alone on rows that are on the device.  The three send the same datagrams for the first
ticks before any time is reported.  Beside them the device time (events) of wmx_mix_drain + wmx_rtp_egress and of wmx_rtp_egress_rings
on twin mixers of as many rings.  And (d), (e): the handle and the resident step again with sequencing on (wmx_conf_sequence, max_gap 3).
The script is a cycle of three ticks, so a leg's sequence numbers cannot count on for ever: they count through the cycle, and (d) and
(e) forget the sequence state at the cycle's start (wmx_rtp_reset_sequence of every leg: one memset per three ticks, inside the timed
region).  Every packet is then in order -- a data call in slot order, none is silence, none is discarded, every counter stays 0 -- so
the load does the work it does with sequencing off and (d) - (b), (e) - (c) are the sequencer's launch, the call-list path of the load
and a third of that memset.

    python tools_dev/bridge_bench.py --pipe --out profiles/bridge/bridge_pipe_bench.json
And (h), (i): the handle and the resident step with sequencing and concealment on (wmx_conf_conceal): (h) - (d), (i) - (e) are the
concealment's launch and the plain load on four repaired slots in place of the call-list load.  --pipe --loss-every N takes one packet in
N out of the script on all sides alike -- the packet with sequence number s of leg g when (g + s) % N == N - 1; its number is consumed
-- so that the sequencer makes silence calls and the concealment's run path is paid for; the sides with sequencing on then send other
datagrams than those without, and only handle and resident step of a kind are compared.
    python tools_dev/bridge_bench.py --pipe --loss-every 50 --out profiles/bridge/bridge_conceal_bench.json
And (j), (k): the handle and the resident step of (b), (c) with DTMF on and suppression on (wmx_conf_dtmf): (j) - (b), (k) - (c) are the
detector's launch.  The script is noise: no block is a tone, no row is zeroed, no key is reported, the datagrams are those of (b).
    python tools_dev/bridge_bench.py --pipe --ulaw-every 2 --out file.json    (profiles/bridge/bridge_dtmf_bench.json is made of such runs)
--pipe --ulaw-every N adds (f), (g): the handle and the resident step again with a codec per leg (wmx_conf_set_codecs): every N-th leg is
WMX_CODEC_PCMU in and mu-law out and its datagrams carry payload type 0, the other legs stay at the default; the launches are the per-leg
ones for every leg.  (f) and (g) send the same datagrams, each leg in its own payload type, before any time is reported.
--pipe --denoise adds (l), (m): the handle and the resident step of (b), (c) with denoising on (wmx_conf_denoise): (l) - (b), (m) - (c)
are the launch of wmx_nsx_process_legs, every row of the script through its leg's suppressor.  --steady makes the script of every side
one packet per leg and tick in slot 0.  Beside them the new kernel alone, device time (events), on as many legs: wmx_nsx_process_legs on
one row per leg against wmx_nsx_process on a dense plane of the same rows -- the dense side twice in every repetition, so that its
own run-to-run spread stands beside the difference -- and then with one leg in eight sending against the dense call, which must
process everyone.  Every side's rows are put back in front of every call, outside the timed region: a row cleaned over and over is
silence, and silence takes the suppressor's short path.
    python tools_dev/bridge_bench.py --pipe --denoise --steady --out profiles/bridge/bridge_denoise_bench.json
--pipe --level V adds (n), (o): the handle and the resident step of (b), (c) with levelling on at compression gain V (wmx_conf_level):
(n) - (b), (o) - (c) are the launch of wmx_agc_process_legs, every row of the script through its leg's AGC.  Beside them the new kernel
alone, device time (events), on as many legs: wmx_agc_process_legs on one row per leg against wmx_agc_process (its four-wave pipeline
kernel) on a dense plane of the same rows -- the dense side twice in every repetition -- and then with one leg in eight sending; and all
of that again with three rows per leg, the most the bench's max_packets holds.  Every
side's rows are put back in front of every call, outside the timed region: a row levelled over and over ends at the limiter.
    python tools_dev/bridge_bench.py --pipe --level 20 --steady --out profiles/bridge/bridge_level_bench.json
--gate-kernel N: nothing of the above; the gate's kernel alone, device time (events), on N legs: wmx_vad_process_legs on one row per leg
against wmx_vad_process (1 x 8000, 20 ms packets, its four-wave pipeline kernel) on a dense plane of the same rows -- the dense side
twice in every repetition -- and then with one leg in eight sending.
    python tools_dev/bridge_bench.py --gate-kernel 4096 --out profiles/bridge/bridge_gate_bench.json
--echo D: nothing of the above; the resident tick of wmx_conf on --echo-legs legs (4 096) with echo control off and on at a reported delay
of D ms, and wmx_aecm_process_legs alone on one row per leg, device time (events)
    python tools_dev/bridge_bench.py --echo 20 --out profiles/bridge/bridge_echo_bench.json
--prompts N: nothing of the above; the resident tick of wmx_conf on --prompt-legs legs (4 096) without a prompt store, with a store nobody
plays from, and with N legs playing an endless clip (wmx_conf_play), device time (events).  With a library that has no prompts in
WMIX_AMD_LIB (the parent's) it measures the first of the three alone.
    python tools_dev/bridge_bench.py --prompts 4096 --out profiles/bridge/bridge_prompts_bench.json
--prompts N --duck R adds the duck (wmx_conf_play_duck): a fourth side on which the N legs play the clip with reduce = R, so that every
conference of 8 has all its rings ducked in every tick, and a fifth on which one leg of every conference does, the other seven
playing with reduce 0.  A library without wmx_conf_play_duck (the parent's) runs the first three alone.
    python tools_dev/bridge_bench.py --prompts 4096 --duck 1 --out file.json    (profiles/bridge/bridge_duck_bench.json is made of such runs)
--record N [--record-format CHN,FREQ]: nothing of the above; the tick of wmx_conf on --record-legs legs (4 096) in conferences of 8 without
a recording store, with a store of N taps of which none is running, and with the N taps running, one per conference (on the first leg
of every conference, then the second, ...): the resident step, device time (events), and the handle with 3 slots, wall clock per tick over
blocks of ticks -- the recorded rows are downloaded with the datagrams there, so the added D2H bytes are in it.  The two sides with a store
are ONE handle, its taps stopped and started between the blocks.  A library without
wmx_conf_recorders (the parent's, given in WMIX_AMD_LIB) runs the first side alone, and so does --record-alone with this one: the two
are then the same program on two libraries.
    python tools_dev/bridge_bench.py --record 512 --record-format 2,16000 --out file.json    (profiles/bridge/bridge_record_bench.json is made of such runs)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wmix_amd.mix import MixBatch  # noqa: E402
from wmix_amd.tick import TickBatch  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes / s a streaming kernel reaches on this part (MI355X: 8 TB/s spec)
BLOCKS = 5


def stats(ms):
    ms = np.asarray(ms)
    blocks = [float(np.median(b)) for b in np.array_split(ms, BLOCKS)]
    med = float(np.median(ms))
    return {"median_ms": round(med, 5), "block_medians_ms": [round(b, 5) for b in blocks], "spread": round((max(blocks) - min(blocks)) / med, 4)}


def alternate(sides, reps, warmup=20):
    """sides: callables; every repetition runs each once between its own pair of events -> per-side lists of milliseconds"""
    for _ in range(warmup):
        for f in sides:
            f()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in sides]
    for r in range(reps):
        for k, f in enumerate(sides):
            ev[k][r][0].record()
            f()
            ev[k][r][1].record()
    torch.cuda.synchronize()
    return [[a.elapsed_time(b) for a, b in side] for side in ev]


def load_minus_vs_gather(n_conf, P, freq, reps):
    per = freq // 1000 * 20  # one 20 ms package, 1 channel, the ring's own format
    n = n_conf * P
    mb = MixBatch(n, 1, freq)
    g = torch.Generator(device="cuda").manual_seed(5)
    src = torch.randint(-20000, 20000, (n_conf, P, per), dtype=torch.int16, device="cuda", generator=g)
    foreign = torch.tensor([[s for s in range(P) if s != q] for q in range(P)], device="cuda")  # [P, P - 1], index order

    def gather_and_load(head, tick):
        staging = src[:, foreign].reshape(n, P - 1, per)
        return mb.load(staging, per * 2, freq, 1, head=head, tick=tick)

    # ---- the same rings?  Both from silence, at two cursors that do not overlap, on the same mixer
    mb.set(0, 0, 1)
    mb.set_play_correct(0)
    ha, _ = mb.load_minus(src, P, per * 2, freq, 1, head=0, tick=0)
    hb, _ = gather_and_load(4 * per * 2, 4 * per * 2)
    assert ha == per * 2 and hb == 5 * per * 2
    sample = sorted({0, 1, n_conf // 2, n_conf - 1})
    for c in sample:
        for q in range(P):
            ring = mb.export(c * P + q)[0]
            assert ring[:per].any() and np.array_equal(ring[:per], ring[4 * per:5 * per]), ("rings differ", c, q)
            assert not ring[5 * per:].any() and not ring[per:4 * per].any()
    # ---- time: each side keeps its own running cursor, like a source that plays on
    cur = {"new": (NULL, 0), "old": (NULL, 0)}

    def new():
        cur["new"] = mb.load_minus(src, P, per * 2, freq, 1, head=cur["new"][0], tick=cur["new"][1])

    def old():
        cur["old"] = gather_and_load(*cur["old"])

    t_new, t_old = alternate([new, old], reps)
    mb.close()
    a, b = stats(t_new), stats(t_old)
    moved = n_conf * per * P * 6
    return {"conferences": n_conf, "parties": P, "ring": "1x%d" % freq, "package_samples": per, "rings_checked": len(sample) * P,
            "load_minus": a, "gather_then_load": b, "ratio": round(b["median_ms"] / a["median_ms"], 2),
            "faster_by_more_than_the_spread": bool(b["median_ms"] - a["median_ms"] > max(a["spread"] * a["median_ms"], b["spread"] * b["median_ms"])),
            "load_minus_bytes": moved, "load_minus_TBs": round(moved / (a["median_ms"] * 1e-3) / 1e12, 3),
            "share_of_achievable_hbm": round(moved / (a["median_ms"] * 1e-3) / HBM_ACHIEVABLE, 3)}


def bridge_tick(n_conf, P, reps):
    n = n_conf * P
    from wmix_amd import synth
    base = synth.conference_inputs(11, reps + 40, 1, 64, 8000, 1)[1]  # [T, 64, 160] talkers, repeated over the batch
    local = torch.from_numpy(np.ascontiguousarray(base)).to("cuda")
    idx = torch.arange(n, device="cuda") % 64
    ticks = [TickBatch(n, 1), TickBatch(n, 1)]  # 1 x 8000 Hz, 20 ms, NS | AEC | AGC | VAD
    ticks[0].bridge(P)
    rec = [torch.zeros((n, 160), dtype=torch.int16, device="cuda") for _ in ticks]
    step = [0, 0]

    def side(k):
        def f():
            rec[k].copy_(local[step[k] % local.shape[0]][idx])
            ticks[k].run(rec[k])
            step[k] += 1
        return f

    t_on, t_off = alternate([side(0), side(1)], reps)
    for t in ticks:
        t.close()
    a, b = stats(t_on), stats(t_off)
    return {"conferences": n_conf, "parties": P, "stages": "NS|AEC|AGC|VAD", "bridge_on": a, "bridge_off": b,
            "bridge_costs_ms_per_tick": round(a["median_ms"] - b["median_ms"], 5)}


NULL = 0xFFFFFFFF


def same_legs_both_ways(n_legs, P, freq, reps):
    per = freq // 1000 * 20
    n_conf = n_legs // P
    n = n_conf * P
    mb = MixBatch(n, 1, freq)
    g = torch.Generator(device="cuda").manual_seed(6)
    src = torch.randint(-20000, 20000, (n, per), dtype=torch.int16, device="cuda", generator=g)
    mb.set_conferences([list(range(c * P, c * P + P)) for c in range(n_conf)])
    mb.set(0, 0, 1)
    mb.set_play_correct(0)
    # ---- the same rings?  Both from silence, at two cursors that do not overlap
    ha, _ = mb.load_minus(src.view(n_conf, P, per), P, per * 2, freq, 1, head=0, tick=0)
    hb, tb = mb.load_minus_conf(src, per * 2, freq, 1, head=np.full(n_conf, 4 * per * 2, np.uint32), tick=np.full(n_conf, 4 * per * 2, np.uint32))
    assert ha == per * 2 and (hb == 5 * per * 2).all()
    sample = sorted({0, 1, n_conf // 2, n_conf - 1})
    for c in sample:
        for q in range(P):
            ring = mb.export(c * P + q)[0]
            assert ring[:per].any() and np.array_equal(ring[:per], ring[4 * per:5 * per]), ("rings differ", c, q)
    cur = {"old": (NULL, 0), "new": (hb, tb)}

    def new():
        cur["new"] = mb.load_minus_conf(src, per * 2, freq, 1, head=cur["new"][0], tick=cur["new"][1])

    def old():
        cur["old"] = mb.load_minus(src.view(n_conf, P, per), P, per * 2, freq, 1, head=cur["old"][0], tick=cur["old"][1])

    t_new, t_old = alternate([new, old], reps)
    mb.close()
    a, b = stats(t_new), stats(t_old)
    moved = n_conf * per * P * 6
    return {"legs": n, "conferences": n_conf, "parties": P, "ring": "1x%d" % freq, "rings_checked": len(sample) * P, "load_minus_conf": a,
            "load_minus": b, "ratio_conf_over_uniform": round(a["median_ms"] / b["median_ms"], 3),
            "load_minus_conf_TBs": round(moved / (a["median_ms"] * 1e-3) / 1e12, 3), "load_minus_TBs": round(moved / (b["median_ms"] * 1e-3) / 1e12, 3)}


def telephony_sizes(n_conf=4096):
    """70 % of 2 legs, 20 % of 3, 8 % of 4 - 8, 2 % of 9 - 32, in a shuffled order"""
    n3, n48, n932 = round(0.20 * n_conf), round(0.08 * n_conf), round(0.02 * n_conf)
    sizes = [2] * (n_conf - n3 - n48 - n932) + [3] * n3 + [4 + k % 5 for k in range(n48)] + [9 + k % 24 for k in range(n932)]
    np.random.default_rng(8).shuffle(sizes)
    return [int(v) for v in sizes]


def telephony_against_padding(reps, freq=8000):
    per = freq // 1000 * 20
    sizes = telephony_sizes()
    n_conf, legs, padded = len(sizes), sum(sizes), len(sizes) * 32
    off = np.concatenate([[0], np.cumsum(sizes)])
    ragged, pad = MixBatch(legs, 1, freq), MixBatch(padded, 1, freq)
    ragged.set_conferences([list(range(off[c], off[c + 1])) for c in range(n_conf)])
    g = torch.Generator(device="cuda").manual_seed(7)
    src = torch.randint(-20000, 20000, (legs, per), dtype=torch.int16, device="cuda", generator=g)
    # the padded form: conference c owns rings 32 c .. 32 c + 31, the legs in front, the rest muted filler
    slot = np.concatenate([32 * c + np.arange(sizes[c]) for c in range(n_conf)])
    src_pad = torch.zeros((padded, per), dtype=torch.int16, device="cuda")
    src_pad[torch.from_numpy(slot).to("cuda")] = src
    mute = np.ones(padded, np.uint8)
    mute[slot] = 0
    mute = torch.from_numpy(mute).to("cuda")
    for m in (ragged, pad):
        m.set(0, 0, 1)
        m.set_play_correct(0)
    cur = {"new": ragged.load_minus_conf(src, per * 2, freq, 1), "old": pad.load_minus(src_pad.view(n_conf, 32, per), 32, per * 2, freq, 1, mute=mute)}
    for c in sorted({0, 1, n_conf // 2, n_conf - 1}):  # the same rings?
        for q in range(sizes[c]):
            a, b = ragged.export(int(off[c]) + q)[0], pad.export(32 * c + q)[0]
            assert a.any() and np.array_equal(a, b), ("rings differ", c, q)

    def new():
        cur["new"] = ragged.load_minus_conf(src, per * 2, freq, 1, head=cur["new"][0], tick=cur["new"][1])

    def old():
        cur["old"] = pad.load_minus(src_pad.view(n_conf, 32, per), 32, per * 2, freq, 1, mute=mute, head=cur["old"][0], tick=cur["old"][1])

    t_new, t_old = alternate([new, old], reps)
    ragged.close()
    pad.close()
    a, b = stats(t_new), stats(t_old)
    hist = {str(k): sizes.count(k) for k in sorted(set(sizes))}
    return {"conferences": n_conf, "sizes": hist, "ring": "1x%d" % freq, "legs": legs, "padded_legs": padded, "layout_load": a, "padded_to_32_load": b,
            "ratio_padded_over_layout": round(b["median_ms"] / a["median_ms"], 2),
            "rings_fifo_rows_and_chain_streams_saved": padded - legs, "ring_bytes_saved": (padded - legs) * 2 * freq}


def legs_against_conf(reps, freq=8000):
    per = freq // 1000 * 20
    sizes = telephony_sizes()
    n_conf, legs = len(sizes), sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    layout = [list(range(off[c], off[c + 1])) for c in range(n_conf)]
    g = torch.Generator(device="cuda").manual_seed(12)
    src = torch.randint(-20000, 20000, (legs, 3, per), dtype=torch.int16, device="cuda", generator=g)
    one = torch.full((legs, 1), per * 2, dtype=torch.int32, device="cuda")
    u = torch.randint(0, 8, (16, legs), device="cuda", generator=g)
    script = torch.zeros((16, legs, 3), dtype=torch.int32, device="cuda")
    script[:, :, 0] = torch.where(u >= 2, per * 2, 0)
    script[:, :, 1] = torch.where(u == 2, per * 2, torch.where(u == 3, per * 2 - 2, 0))
    script[:, :, 2] = torch.where(u == 3, per * 2, 0)
    mixers = {k: MixBatch(legs, 1, freq) for k in ("conf", "steady", "jitter")}
    for m in mixers.values():
        m.set_conferences(layout)
        m.set(0, 0, 1)
    # ---- steady arrivals from fresh cursors: the same rings as the common-cursor load?
    cur = {"conf": mixers["conf"].load_minus_conf(src[:, 0], per * 2, freq, 1)}
    mixers["steady"].load_minus_legs(src[:, :1], per * 2, freq, 1, one)
    for c in sorted({0, 1, n_conf // 2, n_conf - 1}):
        for q in range(sizes[c]):
            a, b = mixers["conf"].export(int(off[c]) + q)[0], mixers["steady"].export(int(off[c]) + q)[0]
            assert a.any() and np.array_equal(a, b), ("rings differ", c, q)
    step = {k: 0 for k in mixers}

    def play_on(k):  # the play thread's bookkeeping of one package, without its launch
        step[k] += 1
        mixers[k].set(step[k] * per * 2 % (2 * freq), step[k] * per * 2, 1)

    def conf():
        play_on("conf")
        cur["conf"] = mixers["conf"].load_minus_conf(src[:, 0], per * 2, freq, 1, head=cur["conf"][0], tick=cur["conf"][1])

    def steady():
        play_on("steady")
        mixers["steady"].load_minus_legs(src[:, :1], per * 2, freq, 1, one)

    def jitter():
        play_on("jitter")
        mixers["jitter"].load_minus_legs(src, per * 2, freq, 1, script[step["jitter"] % 16])

    t_conf, t_steady, t_jitter = alternate([conf, steady, jitter], reps)
    dropped = {k: int(mixers[k].export_leg_cursors()[2].sum()) for k in ("steady", "jitter")}
    for m in mixers.values():
        m.close()
    a, b, c = stats(t_conf), stats(t_steady), stats(t_jitter)
    return {"conferences": n_conf, "sizes": {str(k): sizes.count(k) for k in sorted(set(sizes))}, "ring": "1x%d" % freq, "legs": legs,
            "load_minus_conf": a, "legs_steady_max_packets_1": b, "legs_jitter_max_packets_3": c,
            "packets_per_leg_and_tick_jitter": round(float((script == per * 2).sum()) / (16 * legs), 3), "calls_dropped": dropped,
            "ratio_steady_over_conf": round(b["median_ms"] / a["median_ms"], 3), "ratio_jitter_over_conf": round(c["median_ms"] / a["median_ms"], 3)}


def stage_kernel(stage, legs, reps, value=None, rows=1):
    """A per-leg stage's ragged entry point beside its dense one on the same rows, `rows` (1 .. 3) per leg: device milliseconds per launch.
    stage "denoise": wmx_nsx_process_legs beside wmx_nsx_process, on noise; "level": wmx_agc_process_legs beside wmx_agc_process with the
    compression gain `value`, on voiced rows; "gate": wmx_vad_process_legs beside wmx_vad_process (1 x 8000, 20 ms, one call of one packet:
    its four-wave pipeline kernel), on voiced rows.  The dense side twice in every repetition, so that its own run-to-run spread stands
    beside the difference; then with one leg in eight sending.  Every side's rows are put back in front of every call, outside the timed
    region: a row gated over and over is silence."""
    from wmix_amd.agc import AgcBatch
    from wmix_amd.nsx import NsxBatch
    from wmix_amd.vad import VadBatch
    # the batch, the dense plane's [packets, samples] of a leg, the seed, what stands between "legs" and the timings, what process_legs takes more
    make, dense_shape, seed, head, extras = {
        "denoise": (lambda: NsxBatch(legs, 1, 8000), (2 * rows, 80), 17, {"rows_per_leg": rows, "blocks_per_row": 2}, ()),
        "level": (lambda: AgcBatch(legs, 1, 8000, value), (2 * rows, 80), 17, {"value": value, "rows_per_leg": rows, "packets_per_row": 2}, ()),
        "gate": (lambda: VadBatch(legs, 1, 8000, 20), (rows, 160), 19, {"rows_per_leg": rows},
                 (None, torch.zeros((2, legs), dtype=torch.int32, device="cuda"))),
    }[stage]
    name = {"denoise": "wmx_nsx_process", "level": "wmx_agc_process", "gate": "wmx_vad_process"}[stage]
    rng = np.random.default_rng(seed)
    if stage == "denoise":
        x = rng.normal(0, 400, (legs, 160 * rows))
    else:
        t = np.arange(160 * rows)
        x = rng.integers(300, 12000, (legs, 1)) * np.sin(2 * np.pi * rng.integers(150, 1500, (legs, 1)) * t / 8000) + rng.normal(0, 100, (legs, 160 * rows))
    src = torch.from_numpy(np.clip(np.round(x), -32768, 32767).astype(np.int16)).cuda()
    every, sparse_of = torch.zeros((legs, 3), dtype=torch.int32, device="cuda"), torch.zeros((legs, 3), dtype=torch.int32, device="cuda")
    every[:, :rows] = 320
    sparse_of[::8, :rows] = 320
    handles = [make() for _ in range(4)]
    dense_rows = [torch.zeros((legs,) + dense_shape, dtype=torch.int16, device="cuda") for _ in range(2)]
    leg_rows = [torch.zeros((legs, 3, 160), dtype=torch.int16, device="cuda") for _ in range(2)]

    def dense(k):
        return (lambda: dense_rows[k].view(legs, 160 * rows).copy_(src)), (lambda: handles[k].process(dense_rows[k]))

    def ragged(k, lens):
        return (lambda: leg_rows[k][:, :rows].copy_(src.view(legs, rows, 160))), (lambda: handles[2 + k].process_legs(leg_rows[k], lens, *extras))

    sides = [dense(0), ragged(0, every), dense(1), ragged(1, sparse_of)]
    for prepare, f in sides * 20:
        prepare()
        f()
    assert torch.equal(dense_rows[0].view(legs, rows, 160), leg_rows[0][:, :rows]), "the ragged call and the dense call differ"
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in sides]
    for r in range(reps):
        for k, (prepare, f) in enumerate(sides):
            prepare()
            ev[k][r][0].record()
            f()
            ev[k][r][1].record()
    torch.cuda.synchronize()
    assert torch.equal(dense_rows[0].view(legs, rows, 160), leg_rows[0][:, :rows]), "the ragged call and the dense call differ"
    d0, full, d1, sparse = (stats([a.elapsed_time(b) for a, b in side]) for side in ev)
    for h in handles:
        h.close()
    return {"legs": legs, **head, name + "_dense": d0, name + "_dense_again": d1, name + "_legs_every_leg": full,
            name + "_legs_one_leg_in_eight": sparse, "dense_again_over_dense": round(d1["median_ms"] / d0["median_ms"], 4),
            "legs_over_dense": round(full["median_ms"] / d0["median_ms"], 4), "one_in_eight_over_dense": round(sparse["median_ms"] / d0["median_ms"], 4)}


def echo_tick(legs, reps, delay_ms):
    """--echo D: the resident step of wmx_conf on `legs` legs in conferences of 8, every leg one packet per tick, with echo control off and
    on (wmx_conf_echo, reported delay D), two handles, the sides alternating tick by tick, device time per tick (events) behind 40 ticks
    of warm-up -- every canceller is past its start-up --; and wmx_aecm_process_legs alone, rows and far row in one call, one row per leg."""
    from wmix_amd.aecm import AecmBatch
    from wmix_amd.conf import ConfBridge
    layout = [list(range(c, min(c + 8, legs))) for c in range(0, legs, 8)]
    rng = np.random.default_rng(13)
    CYC = 3
    pk = rng.integers(0, 256, (CYC, legs, 3, 176), dtype=np.uint8)
    pk[..., :12] = 0
    pk[..., 0], pk[..., 1] = 0x80, 0x88
    recv = np.zeros((CYC, legs, 3), np.int32)
    recv[:, :, 0] = 172
    r_in, r_recv = torch.from_numpy(pk).cuda(), torch.from_numpy(recv).cuda()
    r_out = torch.zeros((legs, 172), dtype=torch.uint8, device="cuda")
    sides = {}
    for name in ("off", "on"):
        cb = ConfBridge(legs, 1, 3)
        cb.set_conferences(layout)
        cb.set_play_correct(0)
        if name == "on":
            cb.echo(True, delay_ms)
        sides[name] = cb
    ms = {"off": [], "on": []}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(40 + reps):
        for name, cb in sides.items():
            a.record()
            cb.step_resident(r_in[i % CYC], r_recv[i % CYC], r_out)
            b.record()
            b.synchronize()
            if i >= 40:
                ms[name].append(a.elapsed_time(b))
    running = int((sides["on"].export_echo()["startup"] == 0).sum())
    for cb in sides.values():
        cb.close()
    ab = AecmBatch.create_legs(legs)
    ab.set_delay_legs(delay_ms)
    rows = torch.from_numpy(rng.integers(-3000, 3000, (legs, 1, 160)).astype(np.int16)).cuda()
    far = torch.from_numpy(rng.integers(-3000, 3000, (legs, 160)).astype(np.int16)).cuda()
    lens = torch.full((legs, 1), 320, dtype=torch.int32, device="cuda")
    alone = []
    for i in range(40 + reps):
        work = rows.clone()
        a.record()
        ab.process_legs(work, lens, None, far)
        b.record()
        b.synchronize()
        if i >= 40:
            alone.append(a.elapsed_time(b))
    state_bytes = int(ab.export_stream(0).size)
    ab.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"legs": legs, "conferences": len(layout), "delay_ms": delay_ms, "legs_past_startup": running, "ms_per_tick_echo_off": med["off"],
            "ms_per_tick_echo_on": med["on"], "ms_per_tick_added": med["on"] - med["off"], "aecm_process_legs_one_row_ms": float(np.median(alone)),
            "bytes_per_leg_blob": state_bytes}


def prompts_tick(legs, reps, playing, duck=0):
    """--prompts N: the resident step of wmx_conf on `legs` legs in conferences of 8, every leg one packet per tick, on up to three
    handles, the sides alternating tick by tick, device time per tick (events) behind 40 ticks of warm-up: a handle without a prompt
    store; one with a store nobody plays from; one on which the first N legs play an endless clip of 1 000 samples.  A library that
    has no prompts (the parent's, given in WMIX_AMD_LIB) runs the first side alone: the parent's own figure, by the same tool.
    duck = R > 0: two more handles, the N legs playing with reduce = R, and one leg of every conference with reduce = R beside seven with
    reduce 0; a library without wmx_conf_play_duck leaves them out."""
    from wmix_amd._lib import lib
    from wmix_amd.conf import ConfBridge
    layout = [list(range(c, min(c + 8, legs))) for c in range(0, legs, 8)]
    rng = np.random.default_rng(13)
    CYC = 3
    pk = rng.integers(0, 256, (CYC, legs, 3, 176), dtype=np.uint8)
    pk[..., :12] = 0
    pk[..., 0], pk[..., 1] = 0x80, 0x88
    recv = np.zeros((CYC, legs, 3), np.int32)
    recv[:, :, 0] = 172
    r_in, r_recv = torch.from_numpy(pk).cuda(), torch.from_numpy(recv).cuda()
    r_out = torch.zeros((legs, 172), dtype=torch.uint8, device="cuda")
    has = getattr(lib(), "wmx_conf_prompts", None) is not None
    has_duck = duck > 0 and playing > 0 and getattr(lib(), "wmx_conf_play_duck", None) is not None
    sides = {}
    names = ("no_store", "store_idle", "playing") if has else ("no_store",)
    for name in names + (("duck_all", "duck_one_per_conference") if has_duck else ()):
        cb = ConfBridge(legs, 1, 3)
        cb.set_conferences(layout)
        if name != "no_store":
            cb.prompts(4, 4000)
            clip = cb.add_clip(rng.integers(-8000, 8000, 1000).astype(np.int16))
            who = list(range(min(playing, legs)))
            if name == "playing" and playing > 0:
                cb.play(who, clip, 0, 0)
            if name == "duck_all":
                cb.play(who, clip, 0, 0, reduce=duck)
            if name == "duck_one_per_conference":
                cb.play([g for g in who if g % 8], clip, 0, 0)
                cb.play([g for g in who if g % 8 == 0], clip, 0, 0, reduce=duck)
        sides[name] = cb
    ms = {name: [] for name in sides}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(40 + reps):
        for name, cb in sides.items():
            a.record()
            cb.step_resident(r_in[i % CYC], r_recv[i % CYC], r_out)
            b.record()
            b.synchronize()
            if i >= 40:
                ms[name].append(a.elapsed_time(b))
    still = int((sides["playing"].export_prompts()["clip"] >= 0).sum()) if has else 0
    ducked = {name: int((sides[name].export_duck() > 1).sum()) for name in ("duck_all", "duck_one_per_conference")} if has_duck else {}
    for cb in sides.values():
        cb.close()
    out = {"legs": legs, "conferences": len(layout), "legs_asked_to_play": playing if has else 0, "legs_playing_at_the_end": still,
           "library_has_prompts": bool(has), "library_ducks": bool(has_duck)}
    if has_duck:
        out["reduce"] = duck
        out["rings_ducked_at_the_end"] = ducked
    out.update({"ms_per_tick_" + name: stats(v) for name, v in ms.items()})
    # per playing leg and tick: 320 bytes of clip read, 320 of ring read and 320 written, the 32-byte state entry read and written, 8 of table
    out["hbm_bytes_per_playing_leg_and_tick"] = 320 * 3 + 32 * 2 + 8
    return out


def record_tick(legs, reps, taps, chn, freq, alone=False):
    """--record N: see the head of this file.  Two handles per clock: one without a store, and one with a store that is measured in both
    states, its taps stopped and its taps running, block by block in turn -- so that what is compared is one handle with itself, not two
    handles whose streams the runtime happened to place on other hardware queues.  The order of the sides rotates from block to block."""
    import time
    from wmix_amd._lib import check, lib
    from wmix_amd.conf import ConfBridge
    L = lib()
    layout = [list(range(c, min(c + 8, legs))) for c in range(0, legs, 8)]
    rng = np.random.default_rng(13)
    CYC = 3
    pk = rng.integers(0, 256, (CYC, legs, 3, 176), dtype=np.uint8)
    pk[..., :12] = 0
    pk[..., 0], pk[..., 1] = 0x80, 0x88
    recv = np.zeros((CYC, legs, 3), np.int32)
    recv[:, :, 0] = 172
    r_in, r_recv = torch.from_numpy(pk).cuda(), torch.from_numpy(recv).cuda()
    r_out = torch.zeros((legs, 172), dtype=torch.uint8, device="cuda")
    has = getattr(L, "wmx_conf_recorders", None) is not None and not alone
    tapped = [(k % len(layout)) * 8 + k // len(layout) for k in range(taps)]  # one per conference, then a second one, ...
    assert max(tapped, default=0) < legs and len(set(tapped)) == taps
    made = {}
    for slots in (1, 3):
        for store in ((False, True) if has else (False,)):
            cb = ConfBridge(legs, slots, 3)
            cb.set_conferences(layout)
            cb.set_play_correct(0)
            if store:
                cb.recorders(taps, chn, freq)
            for k in range(slots if slots == 3 else 0):
                cb.rows_in[k][:] = pk[k]
                cb.recv[k][:] = recv[k]
            made[(slots, store)] = cb
    names = ("no_store", "store_idle", "recording") if has else ("no_store",)
    row = made[(1, True)].rec_row_bytes if has else 0
    d_rows = torch.zeros((max(taps, 1), max(row // 2, 1)), dtype=torch.int16, device="cuda")
    d_legs = torch.full((max(taps, 1),), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    tick = {1: 0, 3: 0}

    def enter(slots, name):  # the state of the side, outside every timed region
        cb = made[(slots, name != "no_store")]
        if name == "store_idle":
            cb.record_stop()
        if name == "recording":
            cb.record(tapped, ticks=0)
        cb.wait(-1)
        torch.cuda.synchronize()
        return cb

    def step(cb, name):
        i = tick[1] % CYC
        tick[1] += 1
        if name == "recording":
            check(L.wmx_conf_step_resident_rec(cb._h, r_in[i].data_ptr(), r_recv[i].data_ptr(), r_out.data_ptr(), d_rows.data_ptr(), d_rows.stride(0),
                                               d_legs.data_ptr(), stream), "wmx_conf_step_resident_rec")
        else:  # the C call, as on the recording side: the tick is a handful of launches, and a wrapper's checks would be in its time
            check(L.wmx_conf_step_resident(cb._h, r_in[i].data_ptr(), r_recv[i].data_ptr(), r_out.data_ptr(), stream), "wmx_conf_step_resident")

    per_block = max(reps // BLOCKS, 8)
    ms, wall = {name: [] for name in names}, {name: [] for name in names}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for blk in range(2 * BLOCKS + 1):  # the first block warms up
        for name in names[blk % len(names):] + names[:blk % len(names)]:
            cb = enter(1, name)
            for _ in range(per_block):
                a.record()
                step(cb, name)
                b.record()
                b.synchronize()
                if blk:
                    ms[name].append(a.elapsed_time(b))
            if name == "recording":  # the rows are the rings' heads as the egress encoded them: every tapped leg's row is there
                assert d_legs.cpu().tolist() == tapped and bool(d_rows.any())
            cb = enter(3, name)
            t0 = time.perf_counter()
            for _ in range(per_block):
                cb.submit()
            cb.wait(-1)
            if blk:
                wall[name].append((time.perf_counter() - t0) * 1e3 / per_block)
    written = int(made[(3, True)].export_record()["written"].sum()) if has else 0
    for cb in made.values():
        cb.close()
    out = {"legs": legs, "conferences": len(layout), "taps": taps if has else 0, "format": [chn, freq], "row_bytes": row,
           "library_records": bool(has), "rows_written_by_the_handle_since_its_last_start": written, "ticks_per_block": per_block,
           "d2h_bytes_per_tick_datagrams": legs * 172, "d2h_bytes_per_tick_added_while_recording": taps * (row + 4) if has else 0}
    out.update({"resident_ms_per_tick_" + name: stats(v) for name, v in ms.items()})
    for name, v in wall.items():
        out["handle_wall_ms_per_tick_" + name] = {"median_ms": round(float(np.median(v)), 5), "blocks_ms": [round(x, 5) for x in v],
                                                   "spread": round((max(v) - min(v)) / float(np.median(v)), 4)}
    return out


def conf_pipe(reps, ulaw_every=0, loss_every=0, denoise=False, steady=False, level=-1):
    import ctypes as C
    import time
    from wmix_amd._lib import check, lib
    from wmix_amd.conf import ConfBridge
    from wmix_amd.rtp import RtpSenders
    L = lib()
    sizes = telephony_sizes()
    n_conf, legs = len(sizes), sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    layout = [list(range(off[c], off[c + 1])) for c in range(n_conf)]
    CYC = 3  # the script is a cycle of as many ticks as the handle has slots: every slot keeps its tick's rows
    rng = np.random.default_rng(13)
    u = np.full((CYC, legs), 4) if steady else rng.integers(0, 8, (CYC, legs))
    recv = np.zeros((CYC, legs, 3), np.int32)
    recv[:, :, 0] = np.where(u >= 2, 172, 0)
    recv[:, :, 1] = np.where(u == 2, 172, np.where(u == 3, -1, 0))
    recv[:, :, 2] = np.where(u == 3, 172, 0)
    pk = rng.integers(0, 256, (CYC, legs, 3, 176), dtype=np.uint8)
    pk[..., :12] = 0
    pk[..., 0], pk[..., 1] = 0x80, 0x88
    there = recv > 0
    before = np.cumsum(there.sum(axis=2), axis=0) - there.sum(axis=2)  # datagrams of the leg in the cycle's earlier ticks
    number = np.where(there, before[:, :, None] + np.cumsum(there, axis=2) - 1, 0)  # sequence numbers that count through the cycle
    pk[..., 2], pk[..., 3] = number >> 8, number & 255
    if loss_every > 0:  # the packet with sequence number s of leg g never arrives when (g + s) % N == N - 1: its number is consumed
        gone = there & ((np.arange(legs)[None, :, None] + number) % loss_every == loss_every - 1)
        recv = np.where(gone, 0, recv).astype(np.int32)
    stream = torch.cuda.current_stream().cuda_stream
    # (a) the parent's composition
    tk, snd = TickBatch(legs, 1, stages=0), RtpSenders(legs)
    tk.bridge_conferences(layout)
    check(L.wmx_tick_set_play_correct(tk._h, 0), "wmx_tick_set_play_correct")  # every side: what is loaded is played in the same tick
    mix_a = L.wmx_tick_mix(tk._h)
    h_in, h_recv = [torch.from_numpy(pk[i]) for i in range(CYC)], [torch.from_numpy(recv[i]) for i in range(CYC)]
    d_in, d_recv = torch.zeros((legs, 3, 176), dtype=torch.uint8, device="cuda"), torch.zeros((legs, 3), dtype=torch.int32, device="cuda")
    d_pcm, d_len = torch.zeros((legs, 3, 164), dtype=torch.int16, device="cuda"), torch.zeros((legs, 3), dtype=torch.int32, device="cuda")
    d_play, d_out = torch.zeros((legs, 160), dtype=torch.int16, device="cuda"), torch.zeros((legs, 172), dtype=torch.uint8, device="cuda")
    out_a = torch.zeros((legs, 172), dtype=torch.uint8)
    step = {"a": 0, "b": 0, "c": 0}

    def parent():
        i = step["a"] % CYC
        step["a"] += 1
        d_in.copy_(h_in[i])      # pageable host memory: blocking
        d_recv.copy_(h_recv[i])
        check(L.wmx_rtp_ingest_legs(legs, 3, d_in.data_ptr(), 3 * 176, 176, d_recv.data_ptr(), d_pcm.data_ptr(), 3 * 164, 164, d_len.data_ptr(), None,
                                    stream), "wmx_rtp_ingest_legs")
        check(L.wmx_mix_load_minus_legs(mix_a, d_pcm.data_ptr(), 320, 8000, 1, 16, 3 * 164, 164, 3, d_len.data_ptr(), None, 1, stream),
              "wmx_mix_load_minus_legs")
        tk.play(d_play)
        snd.egress(d_play, 1, 8000, 1, 8000, packets=d_out)
        out_a.copy_(d_out)       # blocking
        return out_a

    # (b) the handle, 3 slots
    cb = ConfBridge(legs, 3, 3)
    cb.set_conferences(layout)
    cb.set_play_correct(0)
    for k in range(3):
        cb.rows_in[k][:] = pk[k]
        cb.recv[k][:] = recv[k]

    def handle():
        step["b"] += 1
        return cb.submit()

    # (c) the launches alone
    cr = ConfBridge(legs, 1, 3)
    cr.set_conferences(layout)
    cr.set_play_correct(0)
    r_in, r_recv = torch.from_numpy(pk).cuda(), torch.from_numpy(recv).cuda()
    r_out = torch.zeros((legs, 172), dtype=torch.uint8, device="cuda")

    def resident():
        i = step["c"] % CYC
        step["c"] += 1
        cr.step_resident(r_in[i], r_recv[i], r_out)

    # (d), (e) the same two with sequencing on
    cs = ConfBridge(legs, 3, 3)
    ce = ConfBridge(legs, 1, 3)
    for x in (cs, ce):
        x.set_conferences(layout)
        x.set_play_correct(0)
        x.sequence(True, 3)
    for k in range(3):
        cs.rows_in[k][:] = pk[k]
        cs.recv[k][:] = recv[k]
    e_out = torch.zeros((legs, 172), dtype=torch.uint8, device="cuda")
    step["d"] = step["e"] = 0

    def new_cycle(bridge, i):
        if i == 0:
            check(L.wmx_rtp_reset_sequence(L.wmx_conf_senders(bridge._h), None, 0, stream), "wmx_rtp_reset_sequence")

    def handle_seq():
        new_cycle(cs, step["d"] % CYC)
        step["d"] += 1
        return cs.submit()

    def resident_seq():
        i = step["e"] % CYC
        step["e"] += 1
        new_cycle(ce, i)
        ce.step_resident(r_in[i], r_recv[i], e_out)

    # (h), (i) the same two with sequencing and concealment on; the histories live on through the cycles
    ch = ConfBridge(legs, 3, 3)
    ci = ConfBridge(legs, 1, 3)
    for x in (ch, ci):
        x.set_conferences(layout)
        x.set_play_correct(0)
        x.sequence(True, 3)
        x.conceal(True)
    for k in range(3):
        ch.rows_in[k][:] = pk[k]
        ch.recv[k][:] = recv[k]
    i_out = torch.zeros((legs, 172), dtype=torch.uint8, device="cuda")
    step["h"] = step["i"] = 0

    def handle_plc():
        new_cycle(ch, step["h"] % CYC)
        step["h"] += 1
        return ch.submit()

    def resident_plc():
        i = step["i"] % CYC
        step["i"] += 1
        new_cycle(ci, i)
        ci.step_resident(r_in[i], r_recv[i], i_out)

    # (j), (k) the handle and the resident step of (b), (c) with DTMF on and suppression on: the script is noise, so no block is a tone, no
    # row is zeroed and nothing is reported -- what a bridge pays per tick while nobody presses a key
    cj = ConfBridge(legs, 3, 3)
    ck = ConfBridge(legs, 1, 3)
    for x in (cj, ck):
        x.set_conferences(layout)
        x.set_play_correct(0)
        x.dtmf(True, suppress=True)
    for k in range(3):
        cj.rows_in[k][:] = pk[k]
        cj.recv[k][:] = recv[k]
    k_out = torch.zeros((legs, 172), dtype=torch.uint8, device="cuda")
    step["k"] = 0

    def handle_dtmf():
        return cj.submit()

    def resident_dtmf():
        i = step["k"] % CYC
        step["k"] += 1
        ck.step_resident(r_in[i], r_recv[i], k_out)

    # (l), (m) the handle and the resident step of (b), (c) with denoising on: every row of the script through its leg's suppressor
    if denoise:
        cl, cm = ConfBridge(legs, 3, 3), ConfBridge(legs, 1, 3)
        for x in (cl, cm):
            x.set_conferences(layout)
            x.set_play_correct(0)
            x.denoise(True)
        for k in range(3):
            cl.rows_in[k][:] = pk[k]
            cl.recv[k][:] = recv[k]
        m_out = torch.zeros((legs, 172), dtype=torch.uint8, device="cuda")
        step["m"] = 0

        def handle_dn():
            return cl.submit()

        def resident_dn():
            i = step["m"] % CYC
            step["m"] += 1
            cm.step_resident(r_in[i], r_recv[i], m_out)

        for t in range(2 * CYC):
            k = handle_dn()
            cl.wait(k)
            resident_dn()
            assert np.array_equal(cl.rows_out[k], m_out.cpu().numpy()), ("handle and resident step differ with denoising on, tick", t)

    # (n), (o) the handle and the resident step of (b), (c) with levelling on: every row of the script through its leg's AGC
    if level >= 0:
        cn, co = ConfBridge(legs, 3, 3), ConfBridge(legs, 1, 3)
        for x in (cn, co):
            x.set_conferences(layout)
            x.set_play_correct(0)
            x.level(True, level)
        for k in range(3):
            cn.rows_in[k][:] = pk[k]
            cn.recv[k][:] = recv[k]
        o_out = torch.zeros((legs, 172), dtype=torch.uint8, device="cuda")
        step["o"] = 0

        def handle_lv():
            return cn.submit()

        def resident_lv():
            i = step["o"] % CYC
            step["o"] += 1
            co.step_resident(r_in[i], r_recv[i], o_out)

        for t in range(2 * CYC):
            k = handle_lv()
            cn.wait(k)
            resident_lv()
            assert np.array_equal(cn.rows_out[k], o_out.cpu().numpy()), ("handle and resident step differ with levelling on, tick", t)

    # (f), (g) the same two with a codec per leg: every ulaw_every-th leg on PCMU both ways, the others at the default
    mixed = ulaw_every > 0
    if mixed:
        ulaw = np.arange(legs) % ulaw_every == ulaw_every - 1
        pk_u = pk.copy()
        pk_u[:, ulaw, :, 1] = 0x80
        cf, cg = ConfBridge(legs, 3, 3), ConfBridge(legs, 1, 3)
        for x in (cf, cg):
            x.set_conferences(layout)
            x.set_play_correct(0)
            x.set_codecs(np.flatnonzero(ulaw), "pcmu", "u")  # one call of many legs: set-up, outside the timed blocks
        for k in range(3):
            cf.rows_in[k][:] = pk_u[k]
            cf.recv[k][:] = recv[k]
        u_in, g_out = torch.from_numpy(pk_u).cuda(), torch.zeros((legs, 172), dtype=torch.uint8, device="cuda")
        step["g"] = 0

        def handle_mixed():
            return cf.submit()

        def resident_mixed():
            i = step["g"] % CYC
            step["g"] += 1
            cg.step_resident(u_in[i], r_recv[i], g_out)

        for t in range(2 * CYC):
            k = handle_mixed()
            cf.wait(k)
            resident_mixed()
            f_rows = cf.rows_out[k].copy()
            assert np.array_equal(f_rows, g_out.cpu().numpy()), ("datagrams differ with mixed codecs, tick", t)
            assert (f_rows[ulaw, 1] == 0x80).all() and (f_rows[~ulaw, 1] == 0x88).all() and (f_rows[ulaw, 12:] != 0xFF).any()

    # ---- the same datagrams?
    for t in range(2 * CYC):
        a = parent().numpy().copy()
        k = handle()
        cb.wait(k)
        resident()
        assert np.array_equal(a, cb.rows_out[k]) and np.array_equal(a, r_out.cpu().numpy()), ("datagrams differ, tick", t)
        k = handle_seq()
        cs.wait(k)
        resident_seq()
        d_rows = cs.rows_out[k].copy()
        assert np.array_equal(d_rows, e_out.cpu().numpy()), ("handle and resident step differ with sequencing on, tick", t)
        k = handle_plc()
        ch.wait(k)
        resident_plc()
        h_rows = ch.rows_out[k].copy()
        assert np.array_equal(h_rows, i_out.cpu().numpy()), ("handle and resident step differ with concealment on, tick", t)
        if loss_every == 0:  # in order and complete: neither stage changes a datagram
            assert np.array_equal(a, d_rows), ("datagrams differ with sequencing on, tick", t)
            assert np.array_equal(a, h_rows), ("datagrams differ with concealment on, tick", t)
        assert (a[:, 12:] != 0xD5).any()
        k = handle_dtmf()
        cj.wait(k)
        resident_dtmf()
        assert np.array_equal(a, cj.rows_out[k]) and np.array_equal(a, k_out.cpu().numpy()), ("datagrams differ with DTMF on, tick", t)

    def wall(f, n, end):
        t0 = time.perf_counter()
        for _ in range(n):
            f()
        end()
        return (time.perf_counter() - t0) * 1e3 / n

    per_block = max(reps // BLOCKS, 8)
    ms = {"a": [], "b": [], "c": [], "d": [], "e": [], "f": [], "g": [], "h": [], "i": [], "j": [], "k": [], "l": [], "m": [], "n": [], "o": []}
    for _ in range(BLOCKS + 1):  # the first block warms up
        ms["a"].append(wall(parent, per_block, torch.cuda.synchronize))
        ms["b"].append(wall(handle, per_block, lambda: cb.wait(-1)))
        ms["c"].append(wall(resident, per_block, torch.cuda.synchronize))
        ms["d"].append(wall(handle_seq, per_block, lambda: cs.wait(-1)))
        ms["e"].append(wall(resident_seq, per_block, torch.cuda.synchronize))
        ms["h"].append(wall(handle_plc, per_block, lambda: ch.wait(-1)))
        ms["i"].append(wall(resident_plc, per_block, torch.cuda.synchronize))
        ms["j"].append(wall(handle_dtmf, per_block, lambda: cj.wait(-1)))
        ms["k"].append(wall(resident_dtmf, per_block, torch.cuda.synchronize))
        if denoise:
            ms["l"].append(wall(handle_dn, per_block, lambda: cl.wait(-1)))
            ms["m"].append(wall(resident_dn, per_block, torch.cuda.synchronize))
        if level >= 0:
            ms["n"].append(wall(handle_lv, per_block, lambda: cn.wait(-1)))
            ms["o"].append(wall(resident_lv, per_block, torch.cuda.synchronize))
        if mixed:
            ms["f"].append(wall(handle_mixed, per_block, lambda: cf.wait(-1)))
            ms["g"].append(wall(resident_mixed, per_block, torch.cuda.synchronize))
    side = lambda v: {"median_ms_per_tick": round(float(np.median(v[1:])), 5), "block_ms_per_tick": [round(x, 5) for x in v[1:]]}  # noqa: E731
    a, b, c, d, e = side(ms["a"]), side(ms["b"]), side(ms["c"]), side(ms["d"]), side(ms["e"])
    sq = cs.export_sequence()
    seq_counters = {name: int(sq[name].sum()) for name in ("lost", "late", "dup", "resync", "overflow")}
    assert loss_every > 0 or not any(seq_counters.values()), seq_counters  # the script is in order
    h, i = side(ms["h"]), side(ms["i"])
    concealed_h = int(ch.export_conceal().sum())
    assert (concealed_h > 0) == (seq_counters["lost"] > 0)
    dropped = {"conf": int(cb.export_legs()["dropped"].sum()), "resident": int(cr.export_legs()["dropped"].sum())}
    # ---- the fused play-and-send kernel beside the pair it replaces
    pair, fused, s2, s3 = MixBatch(legs, 1, 8000), MixBatch(legs, 1, 8000), RtpSenders(legs), RtpSenders(legs)
    p_play, p_out, f_out = torch.zeros_like(d_play), torch.zeros_like(d_out), torch.zeros_like(d_out)

    def drain_then_egress():
        check(L.wmx_mix_drain(pair._h, p_play.data_ptr(), 320, 160, stream), "wmx_mix_drain")
        check(L.wmx_rtp_egress(s2._h, 1, 8000, p_play.data_ptr(), 320, 160, 1, 8000, p_out.data_ptr(), 172, None, stream), "wmx_rtp_egress")

    def egress_rings():
        check(L.wmx_rtp_egress_rings(s3._h, fused._h, f_out.data_ptr(), 172, None, stream), "wmx_rtp_egress_rings")

    t_pair, t_fused = alternate([drain_then_egress, egress_rings], reps)
    assert torch.equal(p_out, f_out)
    kp, kf = stats(t_pair), stats(t_fused)
    more = {}
    if mixed:
        f, g = side(ms["f"]), side(ms["g"])
        more = {"ulaw_every": ulaw_every, "ulaw_legs": int(ulaw.sum()), "f_wmx_conf_3_slots_mixed_codecs": f, "g_step_resident_mixed_codecs": g,
                "f_minus_b_ms": round(f["median_ms_per_tick"] - b["median_ms_per_tick"], 5),
                "g_minus_c_ms": round(g["median_ms_per_tick"] - c["median_ms_per_tick"], 5),
                "refused_of_f": int(cf.export_codecs()["refused"].sum())}
        cf.close()
        cg.close()
    more.update({"loss_every": loss_every, "packets_lost_from_the_script_per_cycle": int((there & (recv <= 0)).sum()),
                 "h_wmx_conf_3_slots_sequencing_and_concealment_on": h, "i_step_resident_sequencing_and_concealment_on": i,
                 "h_minus_d_ms": round(h["median_ms_per_tick"] - d["median_ms_per_tick"], 5),
                 "i_minus_e_ms": round(i["median_ms_per_tick"] - e["median_ms_per_tick"], 5), "concealed_of_h": concealed_h})
    if denoise:
        l_side, m_side = side(ms["l"]), side(ms["m"])
        more.update({"steady": bool(steady), "l_wmx_conf_3_slots_denoise_on": l_side, "m_step_resident_denoise_on": m_side,
                     "l_minus_b_ms": round(l_side["median_ms_per_tick"] - b["median_ms_per_tick"], 5),
                     "m_minus_c_ms": round(m_side["median_ms_per_tick"] - c["median_ms_per_tick"], 5)})
        cl.close()
        cm.close()
    if level >= 0:
        n_side, o_side = side(ms["n"]), side(ms["o"])
        more.update({"steady": bool(steady), "level": level, "n_wmx_conf_3_slots_level_on": n_side, "o_step_resident_level_on": o_side,
                     "n_minus_b_ms": round(n_side["median_ms_per_tick"] - b["median_ms_per_tick"], 5),
                     "o_minus_c_ms": round(o_side["median_ms_per_tick"] - c["median_ms_per_tick"], 5)})
        cn.close()
        co.close()
    j, k = side(ms["j"]), side(ms["k"])
    keys_of_j = int(cj.export_dtmf()["count"].sum())
    assert keys_of_j == 0, keys_of_j  # the script is noise
    more.update({"j_wmx_conf_3_slots_dtmf_on": j, "k_step_resident_dtmf_on": k,
                 "j_minus_b_ms": round(j["median_ms_per_tick"] - b["median_ms_per_tick"], 5),
                 "k_minus_c_ms": round(k["median_ms_per_tick"] - c["median_ms_per_tick"], 5), "keys_reported_of_j": keys_of_j})
    for x in (tk, snd, cb, cr, cs, ce, ch, ci, cj, ck, pair, fused, s2, s3):
        x.close()
    return {**more, "conferences": n_conf, "sizes": {str(k): sizes.count(k) for k in sorted(set(sizes))}, "legs": legs, "max_packets": 3,
            "packets_per_leg_and_tick": round(float((recv > 0).sum()) / (CYC * legs), 3), "ticks_per_block": per_block, "datagram_ticks_checked": 2 * CYC,
            "a_host_tick_bridge_rtp_composition": a, "b_wmx_conf_3_slots": b, "c_step_resident": c,
            "d_wmx_conf_3_slots_sequencing_on": d, "e_step_resident_sequencing_on": e,
            "d_minus_b_ms": round(d["median_ms_per_tick"] - b["median_ms_per_tick"], 5),
            "e_minus_c_ms": round(e["median_ms_per_tick"] - c["median_ms_per_tick"], 5), "sequence_counters_of_d": seq_counters,
            "b_over_c": round(b["median_ms_per_tick"] / c["median_ms_per_tick"], 3), "a_over_b": round(a["median_ms_per_tick"] / b["median_ms_per_tick"], 3),
            "b_nearer_to_c_than_to_a": bool(b["median_ms_per_tick"] - c["median_ms_per_tick"] < a["median_ms_per_tick"] - b["median_ms_per_tick"]),
            "calls_dropped": dropped, "drain_then_egress": kp, "egress_rings": kf,
            "fused_over_pair": round(kf["median_ms"] / kp["median_ms"], 3)}


def speakers_against_load(layout, P, n, freq, max_speakers, reps, what):
    """layout: None = the uniform form with P consecutive legs per conference; else the list of conferences of the layout form"""
    per = freq // 1000 * 20
    mb = MixBatch(n, 1, freq)
    g = torch.Generator(device="cuda").manual_seed(9)
    src = torch.randint(-20000, 20000, (n, per), dtype=torch.int16, device="cuda", generator=g)
    if layout is not None:
        mb.set_conferences(layout)
    confs = layout if layout is not None else [list(range(c * P, c * P + P)) for c in range(n // P)]
    mb.set(0, 0, 1)
    mb.set_play_correct(0)
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    shaped = src.view(n // P, P, per) if layout is None else src

    def select():
        if layout is None:
            mb.select_speakers(shaped, P, per * 2, max_speakers, 0, 3, out=mask)
        else:
            mb.select_speakers_conf(shaped, per * 2, max_speakers, 0, 3, out=mask)

    # ---- the same speakers?  The first call finds every envelope at zero: env' is the row's level, floor 0
    select()
    got, level = mask.cpu().numpy(), src.to(torch.int64).abs().sum(1).cpu().numpy()
    sample = sorted({0, 1, len(confs) // 2, len(confs) - 1})
    for c in sample:
        mem = confs[c]
        order = sorted(range(len(mem)), key=lambda p: (-level[mem[p]], p))[:max_speakers]
        want = [0 if p in order else 1 for p in range(len(mem))]
        assert len(mem) < 2 or got[mem].tolist() == want, ("speakers differ", c)
    assert np.array_equal(mb.export_speakers()[1][confs[sample[-1]]], level[confs[sample[-1]]]) or len(confs[sample[-1]]) < 2
    cur = {}

    def load(key, mute):
        def f():
            if layout is None:
                h, t = cur.get(key, (NULL, 0))
                cur[key] = mb.load_minus(shaped, P, per * 2, freq, 1, mute=mute, head=h, tick=t)
            else:
                h, t = cur.get(key, (None, None))
                cur[key] = mb.load_minus_conf(shaped, per * 2, freq, 1, mute=mute, head=h, tick=t)
        return f

    load_all, load_sel = load("all", None), load("sel", mask)

    def select_then_load():
        select()
        load_sel()

    t_sel, t_all, t_both = alternate([select, load_all, select_then_load], reps)
    mb.close()
    a, b, c = stats(t_sel), stats(t_all), stats(t_both)
    live = sum(len(m) for m in confs if len(m) >= 2)
    read = live * per * 2
    return {"what": what, "legs": n, "conferences": len(confs), "legs_in_conferences": live, "ring": "1x%d" % freq, "package_samples": per,
            "max_speakers": max_speakers, "conferences_checked": len(sample), "select": a, "load_every_leg": b, "select_then_load": c,
            "select_over_load": round(a["median_ms"] / b["median_ms"], 3),
            "select_then_load_over_load": round(c["median_ms"] / b["median_ms"], 3),
            "select_source_bytes": read, "select_TBs": round(read / (a["median_ms"] * 1e-3) / 1e12, 3)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096x8x8000,65536x8x16000", help="conferences x parties x ring rate, comma separated")
    ap.add_argument("--tick", default="4096x8", help="conferences x parties of the tick measurement; empty = skip")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--ragged", action="store_true", help="the bridge over a layout: same legs both ways, a telephony mix against padding")
    ap.add_argument("--speakers", type=int, default=0, help="measure the talker selection with this max_speakers instead (uniform shapes, or --ragged)")
    ap.add_argument("--legs", action="store_true", help="the bridge load with a cursor per leg beside wmx_mix_load_minus_conf, same layout")
    ap.add_argument("--pipe", action="store_true", help="the bridge of RTP/G.711 legs end to end: the parent's composition, wmx_conf, the launches alone")
    ap.add_argument("--ulaw-every", type=int, default=0, help="with --pipe: two more sides, every N-th leg on PCMU both ways (a codec per leg)")
    ap.add_argument("--loss-every", type=int, default=0, help="with --pipe: one packet in N never arrives, on all sides alike: the run path of the concealment")
    ap.add_argument("--denoise", action="store_true", help="with --pipe: two more sides with denoising on, and the new kernel alone beside the dense call")
    ap.add_argument("--level", type=int, default=-1, help="with --pipe: two more sides with levelling on at this compression gain, and the new kernel alone beside the dense call")
    ap.add_argument("--gate-kernel", type=int, default=0, help="wmx_vad_process_legs alone on this many legs beside wmx_vad_process on the same rows; nothing else")
    ap.add_argument("--echo", type=int, default=-1, help="the resident tick on --echo-legs legs with echo control off and on at this reported delay (ms), and the kernel alone; nothing else")
    ap.add_argument("--echo-legs", type=int, default=4096)
    ap.add_argument("--duck", type=int, default=0, help="with --prompts N: two more sides, the N legs playing with this reduce (1 .. 15), and one leg of every conference of 8")
    ap.add_argument("--prompts", type=int, default=-1, help="the resident tick on --prompt-legs legs without a prompt store, with one nobody plays from, and with this many legs playing an endless clip; nothing else")
    ap.add_argument("--prompt-legs", type=int, default=4096)
    ap.add_argument("--record", type=int, default=-1, help="the tick on --record-legs legs without a recording store, with an idle one of this many taps, and with the taps running, one per conference of 8; nothing else")
    ap.add_argument("--record-format", default="1,8000", help="with --record: CHN,FREQ of the store")
    ap.add_argument("--record-legs", type=int, default=4096)
    ap.add_argument("--record-alone", action="store_true", help="with --record: the side without a store alone, as a library without recording runs it")
    ap.add_argument("--steady", action="store_true", help="with --pipe: every leg sends one packet per tick, on all sides alike")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bridge_bench.py measures on the GPU; there is nothing to report without one"
    res = {"tool": "bridge_bench", "device": torch.cuda.get_device_name(0), "reps": args.reps, "load": [], "tick": None}
    if args.legs:
        res = {"tool": "bridge_bench --legs", "device": torch.cuda.get_device_name(0), "reps": args.reps,
               "runs": "the builder's own, one process, the sides alternating", "legs": legs_against_conf(args.reps)}
        args.sizes = args.tick = ""
        args.ragged, args.speakers = False, 0
    if args.gate_kernel > 0:
        res = {"tool": "bridge_bench --gate-kernel", "device": torch.cuda.get_device_name(0), "reps": args.reps,
               "runs": "the builder's own, one process, the sides alternating", "gate_kernel": stage_kernel("gate", args.gate_kernel, args.reps), "load": [], "tick": None}
        args.sizes = args.tick = ""
        args.ragged, args.speakers, args.pipe = False, 0, False
    if args.echo >= 0:
        res = {"tool": "bridge_bench --echo", "device": torch.cuda.get_device_name(0), "reps": args.reps,
               "runs": "the builder's own, one process, the sides alternating", "echo": echo_tick(args.echo_legs, args.reps, args.echo), "load": [], "tick": None}
        args.sizes = args.tick = ""
        args.ragged, args.speakers, args.pipe = False, 0, False
    if args.prompts >= 0:
        res = {"tool": "bridge_bench --prompts", "device": torch.cuda.get_device_name(0), "reps": args.reps,
               "runs": "the builder's own, one process, the sides alternating",
               "prompts": prompts_tick(args.prompt_legs, args.reps, args.prompts, args.duck), "load": [], "tick": None}
        args.sizes = args.tick = ""
        args.ragged, args.speakers, args.pipe = False, 0, False
    if args.record >= 0:
        chn, freq = (int(v) for v in args.record_format.split(","))
        res = {"tool": "bridge_bench --record", "device": torch.cuda.get_device_name(0), "reps": args.reps,
               "runs": "the builder's own, one process, the sides alternating",
               "record": record_tick(args.record_legs, args.reps, args.record, chn, freq, args.record_alone), "load": [], "tick": None}
        args.sizes = args.tick = ""
        args.ragged, args.speakers, args.pipe = False, 0, False
    if args.pipe:
        res = {"tool": "bridge_bench --pipe", "device": torch.cuda.get_device_name(0), "reps": args.reps,
               "runs": "the builder's own, one process, the sides alternating", "pipe": conf_pipe(args.reps, args.ulaw_every, args.loss_every, args.denoise, args.steady, args.level)}
        if args.denoise:
            res["denoise_kernel"] = stage_kernel("denoise", res["pipe"]["legs"], args.reps)
        if args.level >= 0:
            res["level_kernel"] = stage_kernel("level", res["pipe"]["legs"], args.reps, args.level)
            res["level_kernel_three_rows"] = stage_kernel("level", res["pipe"]["legs"], args.reps, args.level, rows=3)
        args.sizes = args.tick = ""
        args.ragged, args.speakers = False, 0
    if args.speakers:
        res = {"tool": "bridge_bench --speakers %d%s" % (args.speakers, " --ragged" if args.ragged else ""), "device": torch.cuda.get_device_name(0),
               "reps": args.reps, "runs": "the builder's own, one process, the sides alternating", "speakers": []}
        for s in [x for x in args.sizes.split(",") if x]:
            n_conf, P, freq = (int(v) for v in s.split("x"))
            if not args.ragged:
                res["speakers"].append(speakers_against_load(None, P, n_conf * P, freq, args.speakers, args.reps, "uniform %dx%d" % (n_conf, P)))
                continue
            for parties in (4, 32):  # the same legs as equal consecutive conferences through the layout
                lay = [list(range(c * parties, c * parties + parties)) for c in range(n_conf * P // parties)]
                res["speakers"].append(speakers_against_load(lay, parties, n_conf * P, freq, args.speakers, args.reps, "layout %dx%d" % (len(lay), parties)))
        if args.ragged:
            sizes = telephony_sizes()
            off = np.concatenate([[0], np.cumsum(sizes)])
            lay = [list(range(off[c], off[c + 1])) for c in range(len(sizes))]
            res["speakers"].append(speakers_against_load(lay, 0, int(off[-1]), 8000, args.speakers, args.reps, "telephony mix of %d conferences" % len(sizes)))
        args.sizes = args.tick = ""
        args.ragged = False
    if args.ragged:
        res = {"tool": "bridge_bench --ragged", "device": torch.cuda.get_device_name(0), "reps": args.reps, "same_legs": [], "telephony": None}
        for s in [x for x in args.sizes.split(",") if x]:
            n_conf, P, freq = (int(v) for v in s.split("x"))
            for parties in (4, 32):
                res["same_legs"].append(same_legs_both_ways(n_conf * P, parties, freq, args.reps))
        res["telephony"] = telephony_against_padding(args.reps)
        args.sizes = args.tick = ""
    for s in [x for x in args.sizes.split(",") if x]:
        n_conf, P, freq = (int(v) for v in s.split("x"))
        res["load"].append(load_minus_vs_gather(n_conf, P, freq, args.reps))
    if args.tick:
        n_conf, P = (int(v) for v in args.tick.split("x"))
        res["tick"] = bridge_tick(n_conf, P, args.reps)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
