// leg_cursor.h -- the cursor of one call leg of the bridge (wmx_mix_load_minus_legs, mix.hip): legs whose packets come early, late
// or not at all.
//
// Every wmix_thread_rtp_recv_pcma keeps a cursor of its own (head, tick; src/wmixTask.c:1266-1268) and calls wmix_load_data once per
// datagram that arrived (:1278-1316), so a leg's cursor moves by the packets IT delivered.  wmix_load_data's cursor rule is the jitter
// buffer: a sender that fell behind the play head (tick < wmix->tick), or has no cursor yet, jumps to head + VIEW_PLAY_CORRECT -- or
// to the START of the ring when that lies behind its end (src/wmix.c:1666-1673); one that runs ahead writes further ahead, and the
// bookkeeping behind the samples moves head and tick by what was written (:1942-1956).  leg_cursor_call applies both (mix_cursor.h)
// for one leg and one packet, as load_begin / load_end of mix.hip do for a host cursor.
//
// The one rule that is not the reference's: a call whose end cursor would lie more than one ring ahead of the mixer's tick is not
// made (`drop`; the cursor stays).  The reference laps the play head there and adds to samples that are still queued.  A leg's
// calls of one launch are contiguous in tick and end at most one ring past the mixer's tick, so together they cover no ring sample
// twice: the load kernel relies on that.
//
// Plain C++ without HIP types: mix.hip includes it for the device, tests/test_leg_cursor_host.py compiles it with g++ and runs it
// beside the oracle's orc_load_data.
#pragma once
#include <cstdint>
#include "leg_calls.h"
#include "mix_cursor.h"

#define WMX_LEG_FN WMX_CURSOR_FN

namespace wmx {

using LegMixState = BridgeMixState;

struct LegCursor {
    uint32_t head, tick;  // head == UINT32_MAX: no cursor yet (the reference's NULL head)
};

WMX_LEG_FN LegCursor leg_cursor_fresh() { return LegCursor{UINT32_MAX, 0u}; }

struct LegCall {
    uint32_t start;   // byte offset in the ring where the call writes its first sample (not meaningful when drop)
    LegCursor after;  // the cursor the call ends with; the cursor it was handed when drop
    bool drop;        // the call is not made
};

// one wmix_load_data call of n_out ring samples handed the cursor c
WMX_LEG_FN LegCall leg_cursor_call(const LegMixState &m, uint32_t n_out, LegCursor c) {
    LegCall r;
    r.after = c;
    mix_cursor_begin(m, r.after.head, r.after.tick);
    r.start = r.after.head;
    mix_cursor_end(m, n_out, r.after.head, r.after.tick);
    r.drop = (uint32_t)(r.after.tick - m.tick) > m.ring_bytes;
    if (r.drop) r.after = c;
    return r;
}

// The calls of one leg in one launch: slot k is a call when valid bit k is set.  Only the first call can jump and only the tail can
// drop (a drop ends the leg's calls of this launch), so the calls made are contiguous in the ring from `start`.
struct LegSpan {
    uint32_t start;    // byte offset of the first call made
    uint32_t count;    // calls made
    uint32_t slots;    // 2 bits per call made: the slot it came from
    uint32_t dropped;  // calls left out
    LegCursor after;
};

WMX_LEG_FN LegSpan leg_cursor_span(const LegMixState &m, uint32_t n_out, LegCursor c, uint32_t valid, int max_packets) {
    LegSpan s{0u, 0u, 0u, 0u, c};
    bool stopped = false;
    for (int k = 0; k < kLegMaxCalls; k++) {
        if (k >= max_packets || !((valid >> k) & 1u)) continue;
        if (stopped) {
            s.dropped++;
            continue;
        }
        const LegCall call = leg_cursor_call(m, n_out, s.after);
        if (call.drop) {
            stopped = true;
            s.dropped++;
            continue;
        }
        if (s.count == 0) s.start = call.start;
        s.slots |= (uint32_t)k << (2u * s.count);
        s.count++;
        s.after = call.after;
    }
    return s;
}

// The same for a call list (leg_calls.h), in list order.  A silence call is a call with zeros (WCT_SILENCE,
// src/wmixTask.c:1307-1309): it moves the cursor by n_out like a data call and can jump or drop like one.  `silence`: bit j set when the j-th call MADE adds nothing.
struct LegSpanCalls {
    LegSpan span;
    uint32_t silence;
};

WMX_LEG_FN LegSpanCalls leg_cursor_span_calls(const LegMixState &m, uint32_t n_out, LegCursor c, uint32_t calls) {
    LegSpanCalls s{LegSpan{0u, 0u, 0u, 0u, c}, 0u};
    const uint32_t n = leg_calls_walked(calls);
    for (uint32_t j = 0; j < n; j++) {
        const LegCall call = leg_cursor_call(m, n_out, s.span.after);
        if (call.drop) {  // the lap rule: this call and the list's tail are left out
            s.span.dropped = n - j;
            break;
        }
        if (s.span.count == 0) s.span.start = call.start;
        s.span.slots |= leg_calls_slot(calls, j) << (2u * s.span.count);
        s.silence |= leg_calls_silence(calls, j) << s.span.count;
        s.span.count++;
        s.span.after = call.after;
    }
    return s;
}

}  // namespace wmx
