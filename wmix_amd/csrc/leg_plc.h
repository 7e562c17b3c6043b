// leg_plc.h -- the concealment rule of one RTP leg of the bridge (wmx_rtp_conceal_legs, rtp.hip): what a leg emits for the calls the
// sequence rule (leg_seq.h) made out of lost packets.
//
// The sequence rule turns a gap of 1 .. 3 lost packets into that many WCT_SILENCE calls: the cursor stays right, and every other leg
// of the conference hears 20 .. 60 ms of hard zero cut into speech.  The reference has no counterpart (its receive thread never reads
// the sequence number).  This rule fills a gap from the leg's own history: the last pitch period, found by an integer correlation,
// repeated under a gain that runs out in 60 ms, and the first 4 ms of the packet behind the gap cross-faded out of that repetition.
// Integers only; >> is an arithmetic shift on int32.
//
// Per leg: hist[320], the last 320 samples the leg emitted, newest at 319, zero when fresh; concealed, a counter.
// Per tick: the leg's PCM rows, d_len and the call list as wmx_rtp_sequence_legs leaves them, walked in list order by the one walk
// of leg_calls.h: a data call that names a row that is not readable is a silence call here, as the load treats it.
//   A RUN is a maximal sequence of consecutive silence calls of the list.  At its start h0 = hist is frozen, q[i] = h0[i] >> 4
//   (|q| <= 2048) and for every lag L in 40 .. 120: c(L) = sum over i = 160 .. 319 of q[i] * q[i - L] (i - L >= 40; |c| <= 160 * 2^22
//   < 2^31).  L* = the smallest L with the largest c(L): no normalisation, no threshold; an all-zero history gives 40 and zeros out.
//   Sample i of the n-th silence call of the run (n = 1, 2, ..): k = (n - 1) * 160 + i, s = h0[320 - L* + k mod L*],
//   g = max(0, 32768 - 68 k), y = (s * g) >> 15 (|s * g| <= 2^30); concealed++ per call.
//   A data call that directly follows a run of n_s calls, x its row: for i in 0 .. 31 cont = the formula above at k = n_s * 160 + i and
//   y[i] = (x[i] * i + cont * (32 - i)) >> 5; for i in 32 .. 159 y[i] = x[i].  Any other data call is emitted as it is.
//   After each call its 160 emitted samples are appended to hist.  The history follows the list, not the load's lap rule or the mute.
// Out: the emitted rows [4][160] in call order and len_out[4]: 320 for j < count, else 0 -- every call has become a data call, for
// wmx_mix_load_minus_legs with max_packets = 4.  A leg with no calls keeps its state.
//
// Plain C++ without HIP types: rtp.hip includes it for the device, tests/test_leg_plc_host.py compiles it with g++ beside a model
// written from the text above.
#pragma once
#include <cstdint>
#include "leg_calls.h"

#define WMX_PLC_FN WMX_CALLS_FN

namespace wmx {

constexpr int kPlcHist = 2 * kLegRow;  // samples of history per leg
constexpr int kPlcLagMin = 40;         // 200 Hz
constexpr int kPlcLagMax = 120;        // 66 Hz
constexpr int kPlcBlend = 32;          // samples of cross-fade behind a run

struct LegPlcState {
    int16_t hist[kPlcHist];
    uint32_t concealed;
};

WMX_PLC_FN int32_t leg_plc_q(int32_t h) { return h >> 4; }

// c(L) over q[0 .. 319]
WMX_PLC_FN int32_t leg_plc_score(const int16_t *q, int32_t L) {
    int32_t c = 0;
    for (int i = kPlcHist - kLegRow; i < kPlcHist; i++) c += (int32_t)q[i] * (int32_t)q[i - L];
    return c;
}

// (c, L) beats (best_c, best_L): the larger score, ties to the smaller lag
WMX_PLC_FN bool leg_plc_better(int32_t c, int32_t L, int32_t best_c, int32_t best_L) { return c > best_c || (c == best_c && L < best_L); }

WMX_PLC_FN int32_t leg_plc_gain(int32_t k) {
    const int32_t g = 32768 - 68 * k;
    return g < 0 ? 0 : g;
}

// where in h0 sample k of a run comes from
WMX_PLC_FN int32_t leg_plc_index(int32_t k, int32_t L) { return kPlcHist - L + k % L; }

WMX_PLC_FN int32_t leg_plc_synth(int32_t s, int32_t k) { return (s * leg_plc_gain(k)) >> 15; }

// sample i < kPlcBlend of the data call behind a run: x from the packet, cont the run continued
WMX_PLC_FN int32_t leg_plc_blend(int32_t x, int32_t cont, int32_t i) { return (x * i + cont * (kPlcBlend - i)) >> 5; }

// One tick of one leg.  pcm: the leg's rows, slot k at pcm + k * packet_stride; len: its max_packets entries of d_len; out:
// kLegMaxCalls rows of kLegRow, of which the first `count` are written; len_out: kLegMaxCalls entries.
WMX_PLC_FN void leg_plc_tick(LegPlcState &st, const int16_t *pcm, long packet_stride, const uint32_t *len, int max_packets, uint32_t calls,
                             int16_t *out, uint32_t *len_out) {
    const LegWalk w = leg_calls_walk(len, true, calls, max_packets);
    const uint32_t count = w.count;
    for (uint32_t j = 0; j < (uint32_t)kLegMaxCalls; j++) len_out[j] = j < count ? kLegRowBytes : 0u;
    int16_t h0[kPlcHist] = {0}, q[kPlcHist];
    int32_t lag = kPlcLagMin, run = 0;  // run: silence calls of the run so far
    for (uint32_t j = 0; j < count; j++) {
        int16_t *y = out + (size_t)j * kLegRow;
        if (!((w.data >> j) & 1u)) {
            if (run == 0) {
                for (int i = 0; i < kPlcHist; i++) h0[i] = st.hist[i], q[i] = (int16_t)leg_plc_q(st.hist[i]);
                int32_t best = leg_plc_score(q, kPlcLagMin);
                for (int32_t L = kPlcLagMin + 1; L <= kPlcLagMax; L++) {
                    const int32_t c = leg_plc_score(q, L);
                    if (leg_plc_better(c, L, best, lag)) best = c, lag = L;
                }
            }
            for (int i = 0; i < kLegRow; i++) {
                const int32_t k = run * kLegRow + i;
                y[i] = (int16_t)leg_plc_synth(h0[leg_plc_index(k, lag)], k);
            }
            run++;
            st.concealed++;
        } else {
            const int16_t *x = pcm + (size_t)leg_calls_slot(calls, j) * packet_stride;
            for (int i = 0; i < kLegRow; i++) {
                if (run > 0 && i < kPlcBlend) {
                    const int32_t k = run * kLegRow + i;
                    y[i] = (int16_t)leg_plc_blend(x[i], leg_plc_synth(h0[leg_plc_index(k, lag)], k), i);
                } else {
                    y[i] = x[i];
                }
            }
            run = 0;
            lag = kPlcLagMin;
        }
        for (int i = 0; i < kPlcHist - kLegRow; i++) st.hist[i] = st.hist[i + kLegRow];
        for (int i = 0; i < kLegRow; i++) st.hist[kPlcHist - kLegRow + i] = y[i];
    }
}

}  // namespace wmx
