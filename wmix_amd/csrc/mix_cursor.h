// mix_cursor.h -- wmix_load_data's cursor rule, once.
//
// A source of the reference keeps a cursor (head, tick) into the mixer's ring and hands it to every wmix_load_data call.  The call
// starts at that cursor unless the source has none yet (the reference's NULL head) or fell behind the play head (tick < wmix->tick):
// then it jumps to head + VIEW_PLAY_CORRECT, or to the START of the ring when that lies behind its end (src/wmix.c:1666-1673).  The
// bookkeeping behind the samples moves head and tick by what was written (:1942-1956).  Both in the reference's uint32 arithmetic.
// Every form of the load applies the rule through these two functions: load_begin / load_end and the legacy wmix_load_data adapter
// (mix.hip), bridge_cursor_step (bridge_layout.h) and leg_cursor_call (leg_cursor.h, host and device).
//
// Plain C++ without HIP types: the host tests compile it with g++ through the headers that include it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define WMX_CURSOR_FN __host__ __device__ inline
#else
#define WMX_CURSOR_FN inline
#endif

namespace wmx {

// What the rule reads of the mixer (wmx_mix: head_off, tick, play_correct, ring_bytes).  The one type of every caller; it keeps the
// name the bridge gave it because the library's symbol of bridge_plan_load (bridge_layout.h) carries it.
struct BridgeMixState {
    uint32_t head_off, tick, play_correct, ring_bytes;
};

// where a call that is handed (head, tick) starts (head == UINT32_MAX: no cursor yet): both are rewritten to the cursor the call
// works from; head is the byte offset of its first sample
WMX_CURSOR_FN void mix_cursor_begin(const BridgeMixState &m, uint32_t &head, uint32_t &tick) {
    if (head == UINT32_MAX || tick < m.tick) {  // src/wmix.c:1666-1673
        head = m.head_off + m.play_correct;
        tick = m.tick + m.play_correct;
        if (head >= m.ring_bytes) head = 0;
    }
}

// the cursor a call that started at (head, tick) ends with after n_out ring samples
WMX_CURSOR_FN void mix_cursor_end(const BridgeMixState &m, uint32_t n_out, uint32_t &head, uint32_t &tick) {
    uint32_t tickAdd = n_out * 2, new_head = head + tickAdd;  // src/wmix.c:1942-1956
    new_head %= m.ring_bytes;
    if (tick < m.tick) {
        new_head = m.head_off + tickAdd;
        tickAdd += m.tick;
        if (new_head >= m.ring_bytes) new_head -= m.ring_bytes;
    } else {
        tickAdd += tick;
    }
    tick = tickAdd;
    head = new_head;
}

}  // namespace wmx
