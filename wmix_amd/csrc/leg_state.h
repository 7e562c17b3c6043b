// leg_state.h -- the state a rule of the bridge keeps per leg: one table, four functions.
//
// A rule's state is ONE device block of columns: column c holds one entry of col[c].bytes per leg, its fresh value the byte col[c].fill
// repeated, and the columns lie behind one another in table order.  THE LAYOUT RULE: every column starts on its entry's alignment
// whatever the number of legs -- the bytes per leg of the columns in front of it are a multiple of min(bytes, 16) rounded down to a
// power of two --, so a table lists its widest column first.  A table that breaks it is never made (make: WMX_EINVAL).
//
// A state is made by the first call that needs it (make), put back to fresh for a list of legs or for all, every column or a range of
// them (reset), given a chosen byte in one column (set) and read out (export_to).
//
// The arithmetic (LegLayout) is plain C++ without HIP: tools_dev/san/leg_state_san.cpp compiles it with g++ and
// tests/test_leg_state_host.py compares every line with its model.  rtp.hip, mix.hip and conf.hip include the whole for LegState.
#pragma once
#include <cstddef>
#include <cstdint>
#include "leg_codec.h"
#include "leg_plc.h"

namespace wmx {

struct LegColumn {
    size_t bytes;
    int fill;
};

constexpr int kLegMaxColumns = 7;
struct LegColumns {  // a table's columns in order; a column of 0 bytes ends a shorter list
    LegColumn col[kLegMaxColumns];
};

// ---- the bridge's eight tables and their columns
// the senders (rtp.hip): sequence number (low 16 bits significant) and timestamp -- rtp_header(..., seq 0, timestamp 0, ssrc 0)
enum { kSendSeq, kSendTs };
constexpr LegColumns kLegSendColumns{{{4, 0}, {4, 0}}};
// the sequence rule (leg_seq.h): unsynced, counters 0
enum { kSeqSynced, kSeqNext, kSeqLost, kSeqLate, kSeqDup, kSeqResync, kSeqOverflow, kSeqWords };
constexpr LegColumns kLegSeqColumns{{{4, 0}, {4, 0}, {4, 0}, {4, 0}, {4, 0}, {4, 0}, {4, 0}}};
// the codec rule (leg_codec.h): refused (uint32), in_codec and out_law (uint8) -- the one table with a fresh value that is not zero
enum { kCodecRefused, kCodecIn, kCodecOutLaw };
constexpr LegColumns leg_codec_columns(int law) { return LegColumns{{{4, 0}, {1, (int)kCodecReference}, {1, law}}}; }
// the concealment rule (leg_plc.h): hist (kPlcHist int16), concealed (uint32)
enum { kPlcColHist, kPlcColConcealed };
constexpr LegColumns kLegPlcColumns{{{kPlcHist * sizeof(int16_t), 0}, {4, 0}}};
// the DTMF rule (leg_dtmf.h): ring (uint64), count, ts and flags (uint32 each); no key down
enum { kDtmfRing, kDtmfCount, kDtmfTs, kDtmfFlags };
constexpr LegColumns kLegDtmfColumns{{{8, 0}, {4, 0}, {4, 0}, {4, 0}}};
// the mixer's cursor per leg (leg_cursor.h): head (UINT32_MAX: no cursor yet), tick and the drop count
enum { kCursorHead, kCursorTick, kCursorDropped };
constexpr LegColumns kLegCursorColumns{{{4, 0xFF}, {4, 0}, {4, 0}}};
// the mixer's talker selection (speakers.h): the envelope (uint32) and the speaking flag (uint8), which no reset touches
enum { kTalkerEnv, kTalkerSpeaking };
constexpr LegColumns kLegTalkerColumns{{{4, 0}, {1, 0}}};
// the conference handle's gate (conf.hip): rows judged voice / not voice, the [2][n_legs] wmx_vad_process_legs counts into
enum { kGateVoiced, kGateUnvoiced };
constexpr LegColumns kLegGateColumns{{{4, 0}, {4, 0}}};

// ---- where the columns lie
struct LegLayout {
    size_t n_legs = 0;
    int n_cols = 0;
    LegColumn col[kLegMaxColumns] = {};
    bool aligned = true;  // the layout rule holds

    LegLayout() = default;
    LegLayout(int n_legs_, const LegColumns &cols) : n_legs((size_t)n_legs_) {
        while (n_cols < kLegMaxColumns && cols.col[n_cols].bytes) {
            col[n_cols] = cols.col[n_cols];
            n_cols++;
        }
        size_t per_leg = 0;
        for (int c = 0; c < n_cols; per_leg += col[c++].bytes) aligned = aligned && per_leg % alignment(col[c].bytes) == 0;
    }
    // what an entry of `bytes` must start on: min(bytes, 16) rounded down to a power of two
    static size_t alignment(size_t bytes) {
        size_t a = 1;
        while (a < 16 && 2 * a <= bytes) a *= 2;
        return a;
    }
    size_t offset(int c) const {  // of column c in the block; c = n_cols: the block's size
        size_t per_leg = 0;
        for (int i = 0; i < c; i++) per_leg += col[i].bytes;
        return per_leg * n_legs;
    }
    // the columns c .. run_end - 1 of those in front of `end` hold one fill byte (same_width: and one width): one memset sets them
    int run_end(int c, bool same_width, int end) const {
        int e = c + 1;
        while (e < end && col[e].fill == col[c].fill && (!same_width || col[e].bytes == col[c].bytes)) e++;
        return e;
    }
};

}  // namespace wmx

#if defined(__HIPCC__)
#include <initializer_list>
#include "wmx_internal.h"

namespace wmx {

struct LegState : LegLayout {
    const char *what = "";   // names the state in an error text
    const char *whose = "";  // whose legs they are in the index error: "handle", "mixer"
    uint8_t *p = nullptr;    // NULL: not made, every leg is fresh

    LegState() = default;
    LegState(const char *what_, const char *whose_, int n_legs_, const LegColumns &cols) : LegLayout(n_legs_, cols), what(what_), whose(whose_) {}
    template <class T>
    T *at(int c) const {
        return p ? reinterpret_cast<T *>(p + offset(c)) : nullptr;
    }

    // the block, fresh and complete on the device when this returns
    int make() {
        if (p) return 0;
        if (!aligned) {
            set_error("%s: a column of the table does not start on its entry's alignment", what);
            return WMX_EINVAL;
        }
        void *q = nullptr;
        WMX_HIP(hipMalloc(&q, offset(n_cols)));
        hipError_t e = hipSuccess;
        for (int c = 0; c < n_cols && e == hipSuccess; c = run_end(c, false, n_cols))
            e = hipMemset(static_cast<uint8_t *>(q) + offset(c), col[c].fill, offset(run_end(c, false, n_cols)) - offset(c));
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            (void)hipFree(q);
            return hip_fail(e, what, __FILE__, __LINE__);
        }
        p = static_cast<uint8_t *>(q);
        return 0;
    }

    // A bad list: WMX_EINVAL and nothing touched.  `who` opens the error text.
    int check(const char *who, const int32_t *host_idx, int n) const {
        return (host_idx && n < 0) || idx_check(host_idx, n, (int)n_legs, who, whose) ? WMX_EINVAL : 0;
    }

    // the byte `value` into column c of the listed legs (NULL = all), on `s`; a state not made yet is made first
    int set(const char *who, int c, int value, const int32_t *host_idx, int n, hipStream_t s) {
        if (check(who, host_idx, n)) return WMX_EINVAL;
        const int rc = make();
        return rc ? rc : write(c, c + 1, value, host_idx, n, s);
    }

    // the columns c0 .. c1 - 1 (default: every column) of the listed legs (NULL = all) fresh again, on `s`: set with each column's fill
    int reset(const char *who, const int32_t *host_idx, int n, hipStream_t s, int c0 = 0, int c1 = -1) {
        if (check(who, host_idx, n)) return WMX_EINVAL;
        if (!p) return make();  // made just now: fresh already
        return write(c0, c1 < 0 ? n_cols : c1, -1, host_idx, n, s);
    }

    // dst[c], where not NULL, takes column c of every leg as the work queued on `s` leaves it; blocking
    int export_to(std::initializer_list<void *> dst, hipStream_t s) const {
        if (p) WMX_HIP(hipStreamSynchronize(s));
        int c = 0;
        for (void *d : dst) {
            const size_t bytes = n_legs * col[c].bytes;
            if (d && p)
                WMX_HIP(hipMemcpy(d, p + offset(c), bytes, hipMemcpyDeviceToHost));
            else if (d)
                memset(d, col[c].fill, bytes);  // never made: fresh
            c++;
        }
        return 0;
    }

    void destroy() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }

private:
    // `value`, or below 0 each column's own fill, into the columns c0 .. c1 - 1 of a list that check() has passed
    int write(int c0, int c1, int value, const int32_t *host_idx, int n, hipStream_t s) {
        if (!host_idx) {
            for (int c = c0; c < c1; c = run_end(c, false, c1))
                WMX_HIP(hipMemsetAsync(p + offset(c), value < 0 ? col[c].fill : value, offset(run_end(c, false, c1)) - offset(c), s));
            return 0;
        }
        // a handful of legs at a time: nothing of the list goes to the device.  The leg's entry in each column; columns of one width
        // are the rows of one 2-D memset
        for (int i = 0; i < n; i++)
            for (int c = c0; c < c1; c = run_end(c, true, c1)) {
                uint8_t *entry = p + offset(c) + (size_t)host_idx[i] * col[c].bytes;
                const int rows = run_end(c, true, c1) - c, byte = value < 0 ? col[c].fill : value;
                if (rows == 1)
                    WMX_HIP(hipMemsetAsync(entry, byte, col[c].bytes, s));
                else
                    WMX_HIP(hipMemset2DAsync(entry, n_legs * col[c].bytes, byte, col[c].bytes, (size_t)rows, s));
            }
        return 0;
    }
};

}  // namespace wmx
#endif
