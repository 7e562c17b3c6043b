// leg_prompt.h -- the prompt of one call leg of the bridge (wmx_mix_load_prompts, mix.hip): an announcement, a beep or hold music
// played into the leg's own ring.
//
// The reference is a mixer daemon, and playing a file is the first thing it does: wmix_task_play_wav (src/wmixTask.c:1353-1595) reads
// a chunk and hands it to wmix_load_data with a cursor of its own, and at the end of the file it stops, or sleeps `interval` and
// starts over, `repeat` times.  The bridge is one reference daemon per leg, so a prompt to leg g is one more task on daemon g, with its
// own cursor, loading ring g beside the receive threads of the other legs.  This rule is that task for one leg and one 20 ms tick.
//
// A CLIP is PCM in the ring's own format (1 x 8000, int16), `samples` long, at sample `off` of the store's arena.
// Per leg: clip (-1: idle), pos (the samples of the current pass that have been loaded), left (the passes left, the current one
// included; 0: endless), done (the prompts that ran to their end since the leg's reset), wait (the ticks of pause still to pass),
// gap (the pause between two passes in ticks, the reference's `interval`; its upper half: reduce, see REDUCE) and the task's cursor
// (head, tick; mix_cursor.h).
//   play(clip, repeat, gap):  clip, pos = 0, left = repeat, wait = 0, gap, a FRESH cursor -- the reference's NULL head: a new task; done
//                             stays.  A play over a playing leg is the same assignment: what the old task loaded plays out.
//   stop:                     idle: clip = -1, pos = left = wait = gap = 0, a fresh cursor; done stays.  A reset is a stop with done = 0.
// One tick (leg_prompt_tick), behind the tick's load of the legs and in front of its drain:
//   idle                      nothing happens.
//   pos >= samples            (a state the clip table does not bear out; no play makes one) the leg goes idle, no call, done stays.
//   wait > 0                  wait--, no call.
//   otherwise                 ONE wmix_load_data call of n = min(160, samples - pos) samples (2 n bytes of 8000 / 1 / 16, reduce 1)
//                             from clip sample pos, by mix_cursor.h's begin / end rule; pos += n.
//     pos == samples, left == 1:  the leg goes idle and done++.
//     pos == samples, else:       left-- unless endless, pos = 0, wait = gap, and the cursor is FRESH again: behind its sleep the
//                                 reference resets the task's cursor (`head.U8 = wmix->head.U8; tick = 0`, src/wmixTask.c:1580-1581),
//                                 so the first call of EVERY pass jumps to head + VIEW_PLAY_CORRECT, whatever lead the pass before
//                                 had left.  The pause heard between two passes is therefore gap ticks, plus the 320 - 2 n bytes the
//                                 short last call of a pass that is no whole number of ticks leaves unwritten.
// Inside a pass the cursor is kept from call to call.  A pass's calls are all whole ticks but the last, so the cursor keeps its lead
// over the play head throughout the pass and no call inside a pass jumps (but where the mixer's tick counter wraps: the reference's
// comparison is plain uint32).  A repeated play also inherits the reference's rule for the ring's end: a pass that begins where
// head + play_correct lies behind it starts at the ring's START (mix_cursor_begin), so with play_correct 3 200 the passes that begin in
// the last 200 ms of a lap of the ring land on top of one another there.
// ORDER.  Within a tick ring g receives the calls of the other legs of its conference first and the prompt's call last: volumeAdd
// saturates, so the order is part of the result.  A prompt passes none of the per-leg stages: it is not sequenced, concealed, denoised,
// levelled, gated or ranked by talker selection, and neither env nor speaking see it.  A leg in no conference, or alone in one, receives
// no legs and still plays its prompt: hold music.
// THE LAP RULE of leg_cursor.h (a call that would end more than one ring ahead of the mixer's tick is not made) cannot fire here.  A
// call starts where the cursor is or, if it jumps, play_correct bytes ahead of the mixer's tick, and adds at most 320 bytes; the drain
// behind every tick moves the mixer's tick by 320.  So by induction the cursor is at most play_correct (the largest in force since the
// play) ahead when a call starts and at most play_correct + 320 ahead when it ends: inside one ring for every play_correct up to
// ring_bytes - 320, the platform's 200 ms (3 200 of 16 000 bytes) included.  And one call covers at most 160 of the ring's 8 000
// samples, so it touches no sample twice whatever the cursor holds.
// REDUCE, the duck.  Every play call of the reference carries `reduce` (0 .. 15; wmix.h:48-98, wmixConf.h:72): while the file plays,
// everything else loaded into the daemon's ring is divided by D = reduce + 1 and the prompt itself is not.  wmix_load_data
// (src/wmix.c:1653, 1675-1676, 1685) sets rdce = (reduce == wmix->reduceMode) ? 1 : wmix->reduceMode and adds every sample as
// volumeAdd(ring, src / rdce): C integer division, which truncates toward zero, BEFORE the saturating add.  The play task holds
// reduceMode = D: it takes it when it starts (src/wmixTask.c:1416-1423), releases it in front of its sleep between two passes
// (:1525-1527), takes it again behind the sleep (:1555-1557) and releases it at its end (:1592-1594).  In the tick model:
//   LEG g IS DUCKED IN A TICK EXACTLY WHEN ITS PROMPT MAKES A CALL IN THAT TICK AND WAS STARTED WITH reduce > 0
// -- on the state as the tick finds it: clip >= 0, wait == 0, pos < samples of a clip the table bears out, and a divisor D = reduce + 1
// in 2 .. 16 (leg_prompt_ducks; 1: not ducked).  The load of the legs runs in front of the prompts' step, so it evaluates this on the
// state before the step.  In a ducked tick every call another leg makes into ring g adds c / D per sample (a silence call or a muted
// source adds 0, as ever); the prompt's own call is reduce == reduceMode, hence undivided, and still last in the ring.  The gap
// between two passes is not ducked, the first tick of the next pass is.  stop, reset and the end of the last pass release the duck; a
// play over a playing leg replaces the divisor as it replaces everything else.  The task takes the mode only if reduceMode == 1, so
// the duck is in force only while the mixer's own reduce_mode is 1 (the conference handle's); on any other mixer a ducking play is an
// ordinary play.  For a ducked ring the load's line rdce = (reduce == reduce_mode) ? 1 : reduce_mode reads (reduce == D) ? 1 : D, with
// `reduce` the load's argument.  A ducked leg in no conference, or alone in one, has nothing to duck and plays as ever.
// The divisor travels as reduce = D - 1 in the upper half of `gap`, which kPromptMaxGap leaves free: the entry stays one 32-byte load,
// and with reduce 0 every field is what it was without it.  leg_prompt_gap gives the pause.
// LEFT OUT: resampling inside the tick, for the reason clips are stored in the ring's format: the caller converts once
// (wmx_pcm_zoom), not every tick.
//
// Plain C++ without HIP types: mix.hip includes it for the device, tests/test_leg_prompt_host.py compiles it with g++ and runs it beside
// a model written from the text above (tests/leg_prompt_model.py).
#pragma once
#include <cstdint>
#include "leg_calls.h"
#include "mix_cursor.h"

#define WMX_PROMPT_FN WMX_CURSOR_FN

namespace wmx {

constexpr uint32_t kPromptMaxGap = 65535u;    // ticks of pause between two passes
constexpr uint32_t kPromptMaxReduce = 15u;    // the reference's `reduce`, 0 .. 15: the others are divided by reduce + 1

struct PromptClip {
    uint32_t off, samples;  // in the arena, in samples
};

struct LegPrompt {  // 32 bytes: one wave-uniform load
    int32_t clip;
    uint32_t pos, left, done, wait, gap;  // gap: the pause in bits 0 .. 15, reduce in bits 16 .. 19
    uint32_t head, tick;  // the task's cursor; head == UINT32_MAX: none yet
};

static_assert(sizeof(LegPrompt) == 32 && sizeof(PromptClip) == 8, "the kernel loads an entry of each with one scalar load");

WMX_PROMPT_FN LegPrompt leg_prompt_idle(uint32_t done) { return LegPrompt{-1, 0u, 0u, done, 0u, 0u, UINT32_MAX, 0u}; }

WMX_PROMPT_FN LegPrompt leg_prompt_play(int32_t clip, uint32_t repeat, uint32_t gap, uint32_t done, uint32_t reduce = 0u) {
    return LegPrompt{clip, 0u, repeat, done, 0u, (gap & kPromptMaxGap) | ((reduce & kPromptMaxReduce) << 16), UINT32_MAX, 0u};
}

WMX_PROMPT_FN uint32_t leg_prompt_gap(const LegPrompt &p) { return p.gap & kPromptMaxGap; }

// the divisor the play was started with, 1 .. 16, whatever the entry holds
WMX_PROMPT_FN uint32_t leg_prompt_divisor(const LegPrompt &p) { return ((p.gap >> 16) & kPromptMaxReduce) + 1u; }

// The divisor in force for this tick's load of the legs into this leg's ring (1: none), on the state as the tick finds it, in front of
// leg_prompt_tick: the prompt makes a call in this tick and was started with reduce > 0.  samples: the clip's length, 0 for a clip the
// table does not bear out.
WMX_PROMPT_FN uint32_t leg_prompt_ducks(const LegPrompt &p, uint32_t samples) {
    return (p.clip >= 0 && p.wait == 0u && p.pos < samples) ? leg_prompt_divisor(p) : 1u;
}

struct PromptCall {
    uint32_t n;      // ring samples the tick's call loads; 0: no call
    uint32_t start;  // byte offset in the ring of its first sample
    uint32_t from;   // the clip sample it starts at
};

// one tick of one leg whose clip is `samples` long
WMX_PROMPT_FN PromptCall leg_prompt_tick(const BridgeMixState &m, uint32_t samples, LegPrompt &p) {
    PromptCall c{0u, 0u, 0u};
    if (p.clip < 0) return c;
    if (p.pos >= samples) {
        p = leg_prompt_idle(p.done);
        return c;
    }
    if (p.wait > 0) {
        p.wait--;
        return c;
    }
    const uint32_t rest = samples - p.pos;
    c.n = rest < (uint32_t)kLegRow ? rest : (uint32_t)kLegRow;
    c.from = p.pos;
    mix_cursor_begin(m, p.head, p.tick);
    c.start = p.head;
    mix_cursor_end(m, c.n, p.head, p.tick);
    p.pos += c.n;
    if (p.pos == samples) {
        if (p.left == 1u) {
            p = leg_prompt_idle(p.done + 1u);
        } else {  // the next pass is a task that starts over: the reference's reset of head and tick behind its sleep
            if (p.left) p.left--;
            p.pos = 0u;
            p.wait = leg_prompt_gap(p);
            p.head = UINT32_MAX;
            p.tick = 0u;
        }
    }
    return c;
}

}  // namespace wmx
