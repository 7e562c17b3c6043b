// leg_seq.h -- the sequence rule of one RTP leg of the bridge (wmx_rtp_sequence_legs, rtp.hip): which wmix_load_data calls a leg makes
// in a tick, and in which order, decided by the one field of the RTP header that says where a packet belongs.
//
// The reference's receive thread makes one call per datagram in arrival order (src/wmixTask.c:1266-1316) and never looks at the
// sequence number, so a lost packet moves every later one 20 ms early, a duplicate is mixed twice and two packets swapped on the wire
// are mixed swapped.  The rule keeps the parity's shape -- one reference mixer per leg, fed calls -- and repairs the list of calls: the
// slots of a tick are put in sequence order, a packet already passed (late) or seen twice (dup) makes no call, and a gap of up to
// max_gap packets becomes that many calls with zeros (WCT_SILENCE, src/wmixTask.c:1307-1309: the cursor moves, no ring changes).  A
// larger jump is a sender that restarted: the leg resyncs to it without silence.
//
// Per leg: synced (0 / 1) and next, the sequence number of the next call position; the counters lost, late, dup, resync, overflow.
// Per tick and slot k: ok_k (the slot is a call after ingest) and s_k, the sequence number in host order.
//   1. no slot ok: no calls, state unchanged.
//   2. not synced: synced = 1, next = s of the first ok slot in slot order.
//   3. an ok slot with (uint16)(next - s_k) in 1 .. WMX_RTP_SEQ_MISORDER is late: discarded, late++.
//   4. every other ok slot is a candidate with forward distance u_k = (uint16)(s_k - next); candidates ascending by u, ties by slot; a
//      candidate with its predecessor's u is a duplicate: discarded, dup++.
//   5. walk with pos = 0: gap = u - pos.  gap > max_gap: resync++, the candidate continues with gap 0.  The candidate needs gap silence
//      calls and one data call; if they do not fit in what is left of kLegMaxCalls calls, it and every later candidate are discarded
//      (overflow counts them) and the walk ends; else they are emitted, lost += gap, pos = u + 1.  A packet more than
//      WMX_RTP_SEQ_MISORDER back is a far-ahead candidate by the uint16 arithmetic and resyncs.
//   6. next += pos.  No trailing silence: a packet that has not come yet may come next tick.
//   7. every discarded slot is named in `discard`: the caller zeroes its d_len.
//
// Plain C++ without HIP types: rtp.hip includes it for the device, tests/test_leg_seq_host.py compiles it with g++ beside a model
// written from the text above.
#pragma once
#include <cstdint>
#include "leg_calls.h"

#define WMX_SEQ_FN WMX_CALLS_FN

namespace wmx {

constexpr uint32_t kSeqMisorder = 16;  // WMX_RTP_SEQ_MISORDER (include/wmix_amd.h)

struct LegSeqState {
    uint32_t synced, next;  // next: low 16 bits significant
    uint32_t lost, late, dup, resync, overflow;
};

struct LegSeqTick {
    uint32_t calls;    // the call list (leg_calls.h)
    uint32_t discard;  // bit k: slot k was ok and makes no call
};

WMX_SEQ_FN void leg_seq_cswap(uint32_t &a, uint32_t &b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo, b = hi;
}

// One tick of one leg.  seq[k]: the sequence number of slot k in host order; ok: bit k set when slot k is a call; max_gap 0 .. 3.
WMX_SEQ_FN LegSeqTick leg_seq_tick(LegSeqState &st, const uint32_t seq[kLegMaxCalls], uint32_t ok, uint32_t max_gap) {
    LegSeqTick r{0u, 0u};
    ok &= (1u << kLegMaxCalls) - 1u;
    if (!ok) return r;
    if (!st.synced) {
        st.synced = 1u;
        for (int k = kLegMaxCalls - 1; k >= 0; k--)
            if ((ok >> k) & 1u) st.next = seq[k] & 0xFFFFu;
    }
    const uint32_t next = st.next & 0xFFFFu;
    // the candidates' keys u << 2 | k (18 bits); a slot that is none sorts behind them
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    uint32_t key[kLegMaxCalls];
    for (int k = 0; k < kLegMaxCalls; k++) {
        key[k] = kNone;
        if (!((ok >> k) & 1u)) continue;
        const uint32_t back = (next - seq[k]) & 0xFFFFu;
        if (back >= 1u && back <= kSeqMisorder) {
            st.late++;
            r.discard |= 1u << k;
            continue;
        }
        key[k] = (((seq[k] - next) & 0xFFFFu) << 2) | (uint32_t)k;
    }
    leg_seq_cswap(key[0], key[1]);  // the fixed network of four: five compare-exchanges
    leg_seq_cswap(key[2], key[3]);
    leg_seq_cswap(key[0], key[2]);
    leg_seq_cswap(key[1], key[3]);
    leg_seq_cswap(key[1], key[2]);
    uint32_t pos = 0, prev_u = kNone;
    bool full = false;
    for (int i = 0; i < kLegMaxCalls; i++) {
        if (key[i] == kNone) continue;
        const uint32_t u = key[i] >> 2, k = key[i] & 3u;
        if (u == prev_u) {
            st.dup++;
            r.discard |= 1u << k;
            continue;
        }
        prev_u = u;
        if (full) {
            st.overflow++;
            r.discard |= 1u << k;
            continue;
        }
        uint32_t gap = u - pos;
        if (gap > max_gap) {
            st.resync++;
            gap = 0;
        }
        if (leg_calls_count(r.calls) + gap + 1u > (uint32_t)kLegMaxCalls) {
            full = true;
            st.overflow++;
            r.discard |= 1u << k;
            continue;
        }
        for (uint32_t g = 0; g < gap; g++) r.calls = leg_calls_push(r.calls, 0u, 1u);
        r.calls = leg_calls_push(r.calls, k, 0u);
        st.lost += gap;
        pos = u + 1u;
    }
    st.next = (next + pos) & 0xFFFFu;
    return r;
}

}  // namespace wmx
