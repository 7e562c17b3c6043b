// leg_calls.h -- the call list of one RTP leg of the bridge and the one walk over a leg's rows of a tick: which of its 0 .. 4 rows a
// per-leg stage takes, and in which order.  What the sequence rule (leg_seq.h) writes and the cursor rule (leg_cursor.h), the
// concealment rule (leg_plc.h), the DTMF rule (leg_dtmf.h), the denoiser of the legs (nsx_legs_kernel, nsx.hip), their AGC
// (agc_legs_kernel, agc.hip) and their voice-activity gate (vad_legs_kernel, vad.hip) read.
//
// A ROW is the 160 samples of one datagram, 20 ms of 1 x 8000; it is readable when its d_len says 320 bytes.
//
// THE CALL WORD (WMX_RTP_CALLS_* of include/wmix_amd.h): count in bits 0 .. 2, call j in bits 4 + 4 j ..: two bits of source slot, one
// bit "silence" (a call with zeros, WCT_SILENCE, src/wmixTask.c:1307-1309).  A count above four is four.
//
// PER LEG AND TICK the leg's rows are taken in the order the load makes its calls: without a call list the slots k = 0 ..
// max_packets - 1 with d_len == 320 in slot order; with one, the list wmx_rtp_sequence_legs leaves (leg_seq.h), in list order, where a
// silence call or a data call naming a row that is not readable adds nothing: the load makes it with zeros, concealment fills it, it
// is a block that is not a tone, and neither the noise estimator nor the level detector nor the gate's noise model is fed.  A leg with no call this tick keeps
// its state.  Every row is taken as the tick brought it.
//
// Plain C++ without HIP types: mix.hip, rtp.hip, nsx.hip, agc.hip and vad.hip include it for the device (the four kernels that walk a
// batch's legs -- DTMF in rtp.hip, nsx_legs_kernel, agc_legs_kernel, vad_legs_kernel -- through leg_calls_walk_leg), wmx_internal.h for
// the argument check the three stages' entry points share (legs_rows_check), tools_dev/san/leg_calls_san.cpp compiles it with g++ and
// tests/test_leg_calls_host.py compares every case with a model written from the text above; the stage models of the tests take the
// same rows through rows_taken of tests/leg_rows_model.py.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define WMX_CALLS_FN __host__ __device__ inline
#else
#define WMX_CALLS_FN inline
#endif
#if defined(__clang__)
#define WMX_CALLS_UNROLL _Pragma("unroll")
#else
#define WMX_CALLS_UNROLL
#endif

namespace wmx {

constexpr int kLegMaxCalls = 4;  // calls, and slots, per leg and tick: WMX_MIX_MAX_LEG_PACKETS (include/wmix_amd.h)
constexpr int kLegRow = 160;     // samples of one row
constexpr uint32_t kLegRowBytes = 2u * kLegRow;

// the call word's layout
WMX_CALLS_FN uint32_t leg_calls_count(uint32_t calls) { return calls & 7u; }
WMX_CALLS_FN uint32_t leg_calls_slot(uint32_t calls, uint32_t j) { return (calls >> (4u + 4u * j)) & 3u; }
WMX_CALLS_FN uint32_t leg_calls_silence(uint32_t calls, uint32_t j) { return (calls >> (6u + 4u * j)) & 1u; }
WMX_CALLS_FN uint32_t leg_calls_set_silence(uint32_t calls, uint32_t j) { return calls | (1u << (6u + 4u * j)); }
WMX_CALLS_FN uint32_t leg_calls_push(uint32_t calls, uint32_t slot, uint32_t silence) {
    const uint32_t j = calls & 7u;
    return ((calls & ~7u) | (j + 1u)) | ((slot | (silence << 2)) << (4u + 4u * j));
}
// the calls a reader walks: the count, at most kLegMaxCalls
WMX_CALLS_FN uint32_t leg_calls_walked(uint32_t calls) {
    const uint32_t n = leg_calls_count(calls);
    return n > (uint32_t)kLegMaxCalls ? (uint32_t)kLegMaxCalls : n;
}

// a slot's row is readable: bit k of the mask a leg's tick is walked with (slots k >= max_packets: 0)
WMX_CALLS_FN uint32_t leg_row_readable(uint32_t len) { return len == kLegRowBytes ? 1u : 0u; }

// call j of the list adds nothing: marked silence, or it names a row that is not readable
WMX_CALLS_FN bool leg_calls_adds_nothing(uint32_t calls, uint32_t j, uint32_t readable) {
    return leg_calls_silence(calls, j) || !((readable >> leg_calls_slot(calls, j)) & 1u);
}

// the leg's rows of the tick as a call list: the list given, or the readable slots in slot order
WMX_CALLS_FN uint32_t leg_calls_list(bool have_calls, uint32_t calls, uint32_t readable, int max_packets) {
    if (have_calls) return calls;
    uint32_t list = 0;
    for (int k = 0; k < kLegMaxCalls && k < max_packets; k++)
        if ((readable >> k) & 1u) list = leg_calls_push(list, (uint32_t)k, 0u);
    return list;
}

// The walk.  len: the leg's max_packets entries of d_len; calls is read only with have_calls.
struct LegWalk {
    uint32_t list;      // the calls in the order they are taken, as a call word
    uint32_t count;     // how many: 0 .. kLegMaxCalls
    uint32_t readable;  // bit k: slot k's row is readable
    uint32_t data;      // bit j, j < count: call j is a data call on a readable row -- the row at slot leg_calls_slot(list, j) is taken
};

WMX_CALLS_FN LegWalk leg_calls_walk(const uint32_t *len, bool have_calls, uint32_t calls, int max_packets) {
    LegWalk w{0u, 0u, 0u, 0u};
    WMX_CALLS_UNROLL
    for (int k = 0; k < kLegMaxCalls; k++)
        if (k < max_packets) w.readable |= leg_row_readable(len[k]) << k;
    w.list = leg_calls_list(have_calls, calls, w.readable, max_packets);
    w.count = leg_calls_walked(w.list);
    WMX_CALLS_UNROLL
    for (uint32_t j = 0; j < (uint32_t)kLegMaxCalls; j++)
        if (j < w.count && !leg_calls_adds_nothing(w.list, j, w.readable)) w.data |= 1u << j;
    return w;
}

// The walk of leg `leg` of a batch.  len: [n_legs][max_packets]; calls_in: NULL, or one call word per leg.
WMX_CALLS_FN LegWalk leg_calls_walk_leg(const uint32_t *len, const uint32_t *calls_in, size_t leg, int max_packets) {
    return leg_calls_walk(len + leg * (size_t)max_packets, calls_in != nullptr, calls_in ? calls_in[leg] : 0u, max_packets);
}

}  // namespace wmx
