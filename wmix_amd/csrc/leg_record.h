// leg_record.h -- the recording tap of one call leg of the bridge (wmx_rtp_record_rings, rtp.hip): what the leg's play thread hands its
// speaker, as PCM, in front of the G.711 encoder.
//
// The reference is a mixer daemon, and recording is one of its verbs: wmix_thread_record_wav (src/wmixTask.c:410-505) takes the daemon's
// audio a package at a time, passes it through wmix_pcm_zoom to the chn x freq the caller asked for, writes it out, and stops after
// `time` seconds or when the daemon is reset (loopWordRecord, :466).  The bridge is one reference daemon per leg, so a recording of leg
// g is one more task on daemon g: it takes the 160 samples the play thread is about to take from ring g -- everybody of the leg's
// conference but the leg itself, its prompt on top, ducked if it is ducked; NOT the leg's own voice -- and converts them.  A RECORDER of
// a conference is the same tap on one more leg of it that is muted, never fed, and whose datagram nobody transmits: it hears everybody.
//
// ONE PACKAGE PER ZOOM CALL.  The reference's recorder reads 1 .. 5 packages per call depending on thread timing (:451, :468), and
// wmix_pcm_zoom starts its phase at zero in every call, so the bytes it writes depend on how the thread happened to be scheduled.  This
// tap is the reader that keeps up: one zoom call per package of 320 bytes in, 1 x 8000 -> chn x freq.  The zoom is stateless and every
// call has the same length in, so every row has the same length out: the number the zoom writes, not wmix_len_of_out's bound.
//
// A STORE has max_taps taps and one format.  Per tap: leg (-1: the tap is free), left (the ticks still to record, this one included;
// 0: until stopped), written (the rows written since the tap was started).
//   start(leg, ticks)   leg, left = ticks, written = 0.  A leg that has a tap is restarted in place; otherwise it takes the LOWEST free
//                       tap.  A list of legs is all or nothing: with fewer free taps than legs that need one nothing starts
//                       (leg_record_assign).  Why ticks and not seconds: the reference counts seconds by the bytes of the source
//                       format and breaks behind the write that completes second `time` -- 50 x time packages of 20 ms, and one package
//                       for time == 0.
//   stop                the tap is free: leg = -1, left = 0; written stays, for the export.
//   reset of its leg    a stop with written = 0: the reference's wmix_reset ends its record threads.
// One tick (leg_record_tick), behind the tick's load of the legs and of the prompts and in front of its drain:
//   free                nothing happens: no row, and the slot's entry of the tap says -1.
//   running             ONE row -- ring `leg` from the play head on, 160 samples, NOT zeroed: the drain still has to play them -- and the
//                       slot's entry of the tap says `leg`; written++.  left == 1: the tap frees itself behind that row.  left > 1:
//                       left--.  left == 0 stays 0.
// The rule reads nothing the device computes, so the host steps a copy of it beside every launch and knows, without a download,
// whether the coming tick has any tap running: a tick without one launches and copies what it did before there were taps.
//
// Plain C++ without HIP types: rtp.hip includes it for host and device, tests/test_leg_record_host.py compiles it with g++ and runs it
// beside a model written from the text above (tests/leg_record_model.py).
#pragma once
#include <cstdint>
#include "mix_cursor.h"

#define WMX_RECORD_FN WMX_CURSOR_FN

namespace wmx {

constexpr int kRecordMaxFreq = 48000;  // what a store's format may ask of the zoom: 1 or 2 channels, 1 .. 48 000 Hz
constexpr int kRecordRowIn = 160;      // the package: 320 bytes of 1 x 8000

struct LegRecord {  // 16 bytes: one wave-uniform load
    int32_t leg;
    uint32_t left, written, pad;
};

static_assert(sizeof(LegRecord) == 16, "the kernel loads an entry with one scalar load");

WMX_RECORD_FN LegRecord leg_record_free(uint32_t written) { return LegRecord{-1, 0u, written, 0u}; }

WMX_RECORD_FN LegRecord leg_record_start(int32_t leg, uint32_t ticks) { return LegRecord{leg, ticks, 0u, 0u}; }

WMX_RECORD_FN LegRecord leg_record_stop(const LegRecord &r) { return leg_record_free(r.written); }

WMX_RECORD_FN LegRecord leg_record_reset() { return leg_record_free(0u); }

// one tick of one tap -> the leg whose row the tick writes, -1 for none
WMX_RECORD_FN int32_t leg_record_tick(LegRecord &r) {
    if (r.leg < 0) return -1;
    const int32_t leg = r.leg;
    r.written++;
    if (r.left == 1u)
        r = leg_record_free(r.written);
    else if (r.left)
        r.left--;
    return leg;
}

// The taps a start of `n` legs takes, into out[i]: the tap legs[i] has already (the lowest, should two hold it), else the lowest free
// tap nobody earlier in the list was given.  A leg listed twice gets one tap.  false: fewer free taps than legs that need one, and
// out is not to be used -- nothing starts.
inline bool leg_record_assign(const LegRecord *taps, int n_taps, const int32_t *legs, int n, int32_t *out) {
    int next_free = 0;
    for (int i = 0; i < n; i++) {
        int at = -1;
        for (int k = 0; k < n_taps && at < 0; k++)
            if (taps[k].leg == legs[i]) at = k;
        for (int j = 0; j < i && at < 0; j++)
            if (legs[j] == legs[i]) at = out[j];
        while (at < 0 && next_free < n_taps) {  // next_free only moves up: a free tap is given once
            const int k = next_free++;
            if (taps[k].leg < 0) at = k;
        }
        if (at < 0) return false;
        out[i] = at;
    }
    return true;
}

// whether the coming tick has a tap that writes a row
inline bool leg_record_any(const LegRecord *taps, int n_taps) {
    for (int k = 0; k < n_taps; k++)
        if (taps[k].leg >= 0) return true;
    return false;
}

}  // namespace wmx
