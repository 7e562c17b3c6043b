// leg_dtmf.h -- the DTMF rule of one RTP leg of the bridge (wmx_rtp_detect_dtmf_legs, rtp.hip): which keys of the telephone keypad a
// leg pressed, heard in band in its decoded PCM or read from RFC 4733 telephone-event packets.
//
// The reference has no counterpart: its receive thread decodes whatever arrives and mixes it (src/wmixTask.c:1266-1316), so a key
// pressed in band is voice -- loud voice, which wins a talker slot -- and an event packet is a payload type nobody knows.  Integers
// only; >> is an arithmetic shift.
//
// DIGIT CODES are the RFC 4733 event numbers 0 .. 15: 0 .. 9 the keys `0` .. `9`, 10 `*`, 11 `#`, 12 .. 15 `A` .. `D`.  Keypad position
// (row r, column c) is code {1,2,3,12, 4,5,6,13, 7,8,9,14, 10,0,11,15}[4 r + c].
//
// ONE BLOCK is the 160 samples x[0 .. 159] of one data call (20 ms of 1 x 8000, a row with d_len == 320).  Everything is int64.
//   Frequencies f = 697, 770, 852, 941 (rows), 1209, 1336, 1477, 1633 (columns); coef = 27980, 26956, 25701, 24219, 19073, 16325,
//   13085, 9315 = round(2 cos(2 pi f / 8000) 2^14), literals, never computed.
//   Per frequency, from s1 = s2 = 0, for n = 0 .. 159: s0 = x[n] + ((coef * s1) >> 14) - s2; s2 = s1; s1 = s0.
//   P = s1 * s1 + s2 * s2 - ((coef * s1) >> 14) * s2.
//   |s| stays below 2^24 for any int16 input (a full-scale square wave at 697 Hz reaches 6.2e6: the sum over 160 samples of the
//   resonator's impulse response sin((n + 1) w) / sin w, times 32768), so s1 and s2 are held as int32 here and every product is
//   formed in int64: the values are those of the all-int64 text.
//   E = the sum of x[n]^2.  r* = the row with the largest P, c* = the column with the largest P, ties to the lower index.
//   The block is a TONE of digit table[4 r* + c*] when all of
//     P_r* >= 400000000 and P_c* >= 400000000
//     P_c* <= 4 P_r* and P_r* <= 8 P_c*                                   (the twist limits)
//     8 P_i <= P_r* for every other row i, 8 P_i <= P_c* for every other column i
//     P_r* + P_c* >= 32 E
//   hold.  The numbers are part of the rule.
//
// PER LEG AND TICK the leg's blocks are its calls in the order of leg_calls.h's walk; a call that adds nothing there is a block that is
// not a tone.  A leg with no block this tick keeps its state.  Every block is judged on its row as the tick brought it.
//
// DEBOUNCE.  cand = the previous block's digit or none; cur = the digit that is down or none.  A block that is a tone of d with
// cand == d and cur != d reports d once and sets cur = d.  A block that is not a tone after a block that was not a tone either sets
// cur = none.  Then cand = this block's digit or none.  So a key fills two consecutive packets before it is reported, and two packets
// without a tone pass before the same key is reported again.
//
// RFC 4733 reads the raw datagram rows, not the PCM, whatever the call list says.  For every slot in slot order with recv >= 16,
// (byte 1 & 0x7F) == event_pt and event = byte 12 <= 15: the packet reports `event` once when the leg has no last event timestamp or
// bytes 4 .. 7 differ from it as four raw bytes, and stores those four bytes.  Retransmissions and end packets of one key press share a
// timestamp and report nothing more; event > 15 (flash, fax tones) is ignored, and leaves the stored timestamp alone.  The packet
// stays refused for the audio path (leg_codec.h).
//
// REPORT.  count (uint32, every digit reported) and ring[8] (uint8): report number n (from 0) is ring[n & 7] = code | 0x80 from a
// packet, code heard in band.  A tick's packet reports are stored before its in-band reports.
//
// SUPPRESSION.  With suppress on every block that is a tone -- the block's own decision, not the debounced one -- is zeroed in the
// leg's PCM row in place, once every block of the tick has been judged; d_len stays, so it is a data call of zeros.
//
// Plain C++ without HIP types: rtp.hip includes it for the device, tests/test_leg_dtmf_host.py compiles it with g++ beside a model
// written from the text above.
#pragma once
#include <cstdint>
#include "leg_calls.h"

#define WMX_DTMF_FN WMX_CALLS_FN

namespace wmx {

constexpr int kDtmfFreqs = 8;
constexpr int32_t kDtmfNone = -1;
constexpr int64_t kDtmfMinPower = 400000000;
constexpr uint32_t kDtmfMinEventBytes = 16;  // the 12-byte header and the four bytes of an event payload
constexpr uint32_t kDtmfFromPacket = 0x80u;

struct LegDtmfState {
    uint32_t count;   // digits reported
    uint64_t ring;    // ring[i] is bits 8 i .. 8 i + 7: in memory the eight bytes of uint8 ring[8] on a little-endian machine
    uint32_t ts;      // header bytes 4 .. 7 of the last event packet, as stored
    uint32_t flags;   // has_ts | (cand + 1) << 8 | (cur + 1) << 16: all zero is the fresh state
};

WMX_DTMF_FN uint32_t leg_dtmf_has_ts(const LegDtmfState &st) { return st.flags & 1u; }
WMX_DTMF_FN int32_t leg_dtmf_cand(const LegDtmfState &st) { return (int32_t)((st.flags >> 8) & 0xFFu) - 1; }
WMX_DTMF_FN int32_t leg_dtmf_cur(const LegDtmfState &st) { return (int32_t)((st.flags >> 16) & 0xFFu) - 1; }
WMX_DTMF_FN void leg_dtmf_set(LegDtmfState &st, uint32_t has_ts, int32_t cand, int32_t cur) {
    st.flags = (has_ts & 1u) | ((uint32_t)(cand + 1) << 8) | ((uint32_t)(cur + 1) << 16);
}

WMX_DTMF_FN int32_t leg_dtmf_coef(int f) {
    switch (f) {
    case 0: return 27980;
    case 1: return 26956;
    case 2: return 25701;
    case 3: return 24219;
    case 4: return 19073;
    case 5: return 16325;
    case 6: return 13085;
    default: return 9315;
    }
}

WMX_DTMF_FN int32_t leg_dtmf_code(int r, int c) {
    switch (4 * r + c) {
    case 0: return 1;
    case 1: return 2;
    case 2: return 3;
    case 3: return 12;
    case 4: return 4;
    case 5: return 5;
    case 6: return 6;
    case 7: return 13;
    case 8: return 7;
    case 9: return 8;
    case 10: return 9;
    case 11: return 14;
    case 12: return 10;
    case 13: return 0;
    case 14: return 11;
    default: return 15;
    }
}

// (coef * s1) >> 14: |coef| < 2^15 and |s1| < 2^24, so it fits int32
WMX_DTMF_FN int32_t leg_dtmf_turn(int32_t coef, int32_t s1) { return (int32_t)(((int64_t)coef * (int64_t)s1) >> 14); }

WMX_DTMF_FN void leg_dtmf_step(int32_t &s1, int32_t &s2, int32_t coef, int32_t x) {
    const int32_t s0 = x + leg_dtmf_turn(coef, s1) - s2;
    s2 = s1;
    s1 = s0;
}

WMX_DTMF_FN int64_t leg_dtmf_power(int32_t s1, int32_t s2, int32_t coef) {
    return (int64_t)s1 * s1 + (int64_t)s2 * s2 - (int64_t)leg_dtmf_turn(coef, s1) * s2;
}

WMX_DTMF_FN int64_t leg_dtmf_energy(int64_t e, int32_t x) { return e + (int64_t)x * x; }

// the block's digit, or kDtmfNone.  p: the eight powers, rows then columns
WMX_DTMF_FN int32_t leg_dtmf_decide(const int64_t p[kDtmfFreqs], int64_t e) {
    int r = 0, c = 0;
    int64_t pr = p[0], pc = p[4];
    for (int i = 1; i < 4; i++) {
        if (p[i] > pr) pr = p[i], r = i;
        if (p[4 + i] > pc) pc = p[4 + i], c = i;
    }
    bool tone = pr >= kDtmfMinPower && pc >= kDtmfMinPower && pc <= 4 * pr && pr <= 8 * pc && pr + pc >= 32 * e;
    for (int i = 0; i < 4; i++) {
        if (i != r && 8 * p[i] > pr) tone = false;
        if (i != c && 8 * p[4 + i] > pc) tone = false;
    }
    return tone ? leg_dtmf_code(r, c) : kDtmfNone;
}

// one frequency of one block
WMX_DTMF_FN int64_t leg_dtmf_goertzel(const int16_t *x, int f) {
    const int32_t coef = leg_dtmf_coef(f);
    int32_t s1 = 0, s2 = 0;
    for (int n = 0; n < kLegRow; n++) leg_dtmf_step(s1, s2, coef, x[n]);
    return leg_dtmf_power(s1, s2, coef);
}

// one block on the host: powers and energy out (either may be NULL)
WMX_DTMF_FN int32_t leg_dtmf_block_digit(const int16_t *x, int64_t *p_out, int64_t *e_out) {
    int64_t p[kDtmfFreqs], e = 0;
    for (int f = 0; f < kDtmfFreqs; f++) p[f] = leg_dtmf_goertzel(x, f);
    for (int n = 0; n < kLegRow; n++) e = leg_dtmf_energy(e, x[n]);
    for (int f = 0; p_out && f < kDtmfFreqs; f++) p_out[f] = p[f];
    if (e_out) *e_out = e;
    return leg_dtmf_decide(p, e);
}

WMX_DTMF_FN void leg_dtmf_report(LegDtmfState &st, uint32_t byte) {
    const uint32_t sh = 8u * (st.count & 7u);
    st.ring = (st.ring & ~((uint64_t)0xFFu << sh)) | ((uint64_t)(byte & 0xFFu) << sh);
    st.count++;
}

// one datagram slot: recv what recvfrom returned, b1 header byte 1, event byte 12, ts bytes 4 .. 7 as one word as stored (b1, event and
// ts are read only where recv >= kDtmfMinEventBytes)
WMX_DTMF_FN void leg_dtmf_packet(LegDtmfState &st, int32_t recv, uint32_t b1, uint32_t event, uint32_t ts, uint32_t event_pt) {
    if (recv < (int32_t)kDtmfMinEventBytes || (b1 & 0x7Fu) != event_pt || event > 15u) return;
    if (!leg_dtmf_has_ts(st) || ts != st.ts) leg_dtmf_report(st, event | kDtmfFromPacket);
    st.ts = ts;
    st.flags |= 1u;
}

// the debounce: one block, digit or kDtmfNone
WMX_DTMF_FN void leg_dtmf_debounce(LegDtmfState &st, int32_t digit) {
    int32_t cur = leg_dtmf_cur(st);
    const int32_t cand = leg_dtmf_cand(st);
    if (digit != kDtmfNone) {
        if (cand == digit && cur != digit) {
            leg_dtmf_report(st, (uint32_t)digit);
            cur = digit;
        }
    } else if (cand == kDtmfNone) {
        cur = kDtmfNone;
    }
    leg_dtmf_set(st, leg_dtmf_has_ts(st), digit, cur);
}

WMX_DTMF_FN uint32_t leg_dtmf_word(const uint8_t *p) {  // four raw bytes as a little-endian machine loads them
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// One tick of one leg on the host.  packets: slot k at packets + k * packet_stride; recv, len: max_packets entries; pcm: slot k at
// pcm + k * pcm_packet_stride, zeroed in place where suppress says so; digits (kLegMaxCalls entries, may be NULL): the per-block
// decisions in block order, kDtmfNone behind the last.  -> the number of blocks
WMX_DTMF_FN uint32_t leg_dtmf_tick(LegDtmfState &st, const uint8_t *packets, long packet_stride, const int32_t *recv, int16_t *pcm,
                                   long pcm_packet_stride, const uint32_t *len, int max_packets, bool have_calls, uint32_t calls,
                                   uint32_t event_pt, bool suppress, int32_t *digits) {
    for (int k = 0; k < kLegMaxCalls && k < max_packets; k++) {
        const uint8_t *pkt = packets + (size_t)k * packet_stride;
        if (recv[k] >= (int32_t)kDtmfMinEventBytes) leg_dtmf_packet(st, recv[k], pkt[1], pkt[12], leg_dtmf_word(pkt + 4), event_pt);
    }
    const LegWalk w = leg_calls_walk(len, have_calls, calls, max_packets);
    const uint32_t list = w.list, count = w.count;
    int32_t d[kLegMaxCalls] = {kDtmfNone, kDtmfNone, kDtmfNone, kDtmfNone};
    for (uint32_t j = 0; j < count; j++) {
        if ((w.data >> j) & 1u) d[j] = leg_dtmf_block_digit(pcm + (size_t)leg_calls_slot(list, j) * pcm_packet_stride, nullptr, nullptr);
        leg_dtmf_debounce(st, d[j]);
    }
    for (uint32_t j = 0; suppress && j < count; j++) {
        if (d[j] == kDtmfNone) continue;
        int16_t *row = pcm + (size_t)leg_calls_slot(list, j) * pcm_packet_stride;
        for (int i = 0; i < kLegRow; i++) row[i] = 0;
    }
    for (int j = 0; digits && j < kLegMaxCalls; j++) digits[j] = d[j];
    return count;
}

}  // namespace wmx
