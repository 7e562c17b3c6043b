// slot_ring.h -- the rotating slots that move host rows through the device, once for wmx_pipe (pipe.hip), the sub-batches of a wmx_rt
// (rt.hip) and wmx_conf (conf.hip).  Host code only: it sequences copies and events.
//
// A ring has `n` slots.  A slot holds a short table of buffers -- pinned host memory (hipHostMalloc: the copies run on the DMA engines,
// no staging; zeroed when made) and a device twin each, `up` buffers going to the device and `down` buffers coming back -- the events
// ev_in, ev_done, ev_gate, ev_out and the flag in_flight.  The ring has a copy-in and a copy-out stream (its own, or borrowed: the
// sub-batches of a wmx_rt share the rt's two, one FIFO of uploads and one of downloads), the rotation `next` and `pending`, the slot
// whose download is not queued yet.  One step over slot k is
//
//     retire(k) -> upload(k) on the copy-in stream -> (ev_in) -> the owner's launches on its compute stream -> done(k) (ev_done)
//               -> download(k) on the copy-out stream -> (ev_out) -> commit(k)
//
// and returns at once: while step k computes, the rows of step k + 1 arrive and those of step k - 1 leave.
//
// FAILING CLEAN.  Nothing of the bookkeeping -- `next`, `pending`, a slot's in_flight (and, in the pipe, the gate armed in the chain) --
// moves before the last fallible call has succeeded: commit() is the only place they move.  A step that fails
//   * BEFORE its first launch (taking the slot, the uploads and their event) has advanced nothing at all: upload() has drained the copy-in
//     stream, the same rows may be submitted again and the results are those of a run that never failed;
//   * AFTER its first launch has lost the step: the stages that ran have consumed the step's input -- as the reference's heartbeat has
//     when aec_process2 fails behind ns_process, which worked in place (src/wmix.c:613-709: no rollback there either) -- the slot's
//     down rows are undefined, the owner counts or reports it (wmx_pipe_failed_steps; "the tick is lost"), drain() empties the streams,
//     and the download still owed for the PREVIOUS step is queued by the next submit or wait as if nothing had happened.  A host that
//     cannot lose a step restores the streams from wmx_chain_export_stream / _export_cohort blobs taken at a checkpoint
//     (tests/test_pipe_faults_gpu.py does).
#pragma once
#include <vector>
#include "wmx_internal.h"

namespace wmx {

constexpr int kMaxSlots = 16;  // what wmx_pipe_create*, wmx_rt_create* and wmx_conf_create accept: 1 .. kMaxSlots
inline bool slots_ok(int slots) { return slots >= 1 && slots <= kMaxSlots; }

struct SlotRing {
    static constexpr int kMaxBufs = 5;
    struct Buf {
        size_t bytes;
        bool up;    // host -> device in upload(); otherwise device -> host in download()
        int alias;  // >= 0: the device twin IS that (earlier) buffer's, e.g. rows worked on in place; -1: its own
    };
    struct Slot {
        void *h[kMaxBufs], *d[kMaxBufs];
        hipEvent_t ev_in, ev_done, ev_gate, ev_out;
        bool in_flight;
    };
    std::vector<Buf> buf;
    std::vector<Slot> slot;
    hipStream_t s_in = nullptr, s_out = nullptr;
    bool own_streams = false;
    int next = 0;
    int pending = -1;  // the slot whose download is not queued yet (commit(k, true)), or -1

    // shared_in / shared_out: the copy streams of somebody else, who outlives the ring; NULL: the ring makes (and destroys) its own
    hipError_t make(int n_slots, std::initializer_list<Buf> bufs, hipStream_t shared_in = nullptr, hipStream_t shared_out = nullptr) {
        buf.assign(bufs);
        slot.assign((size_t)n_slots, Slot{});
        own_streams = !shared_in;
        s_in = shared_in, s_out = shared_out;
        hipError_t e = hipSuccess;
        if (own_streams) {
            e = hipStreamCreateWithFlags(&s_in, hipStreamNonBlocking);
            if (e == hipSuccess) e = hipStreamCreateWithFlags(&s_out, hipStreamNonBlocking);
        }
        for (Slot &s : slot) {
            for (size_t b = 0; b < buf.size(); b++) {
                if (e == hipSuccess) e = hipHostMalloc(&s.h[b], buf[b].bytes, hipHostMallocDefault);
                if (e == hipSuccess) memset(s.h[b], 0, buf[b].bytes);
                if (buf[b].alias >= 0)
                    s.d[b] = s.d[buf[b].alias];
                else if (e == hipSuccess)
                    e = hipMalloc(&s.d[b], buf[b].bytes);
            }
            for (hipEvent_t *ev : {&s.ev_in, &s.ev_done, &s.ev_gate, &s.ev_out})
                if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
        }
        return e;
    }
    // One more buffer in every slot of a ring that is IDLE (no slot in flight, nothing pending: the owner has waited for every slot),
    // for an owner that learns of a buffer behind make() -- the conference handle's recording rows.  Its index is buf.size() - 1
    // afterwards; on a failure the ring is what it was.
    hipError_t add(Buf b) {
        if ((int)buf.size() >= kMaxBufs || b.alias >= 0) return hipErrorInvalidValue;
        const size_t at = buf.size();
        hipError_t e = hipSuccess;
        for (Slot &s : slot) {
            s.h[at] = s.d[at] = nullptr;
            if (e == hipSuccess) e = hipHostMalloc(&s.h[at], b.bytes, hipHostMallocDefault);
            if (e == hipSuccess) memset(s.h[at], 0, b.bytes);
            if (e == hipSuccess) e = hipMalloc(&s.d[at], b.bytes);
            if (e == hipSuccess) e = hipMemset(s.d[at], 0, b.bytes);
        }
        if (e != hipSuccess) {
            for (Slot &s : slot) {
                if (s.h[at]) (void)hipHostFree(s.h[at]);
                if (s.d[at]) (void)hipFree(s.d[at]);
                s.h[at] = s.d[at] = nullptr;
            }
            return e;
        }
        buf.push_back(b);
        return hipSuccess;
    }
    // safe on a ring that make() left half made; the caller has waited for the device
    void destroy() {
        for (Slot &s : slot) {
            for (size_t b = 0; b < buf.size(); b++) {
                if (s.h[b]) (void)hipHostFree(s.h[b]);
                if (s.d[b] && buf[b].alias < 0) (void)hipFree(s.d[b]);
            }
            for (hipEvent_t ev : {s.ev_in, s.ev_done, s.ev_gate, s.ev_out})
                if (ev) (void)hipEventDestroy(ev);
        }
        slot.clear();
        if (own_streams) {
            if (s_in) (void)hipStreamDestroy(s_in);
            if (s_out) (void)hipStreamDestroy(s_out);
        }
        s_in = s_out = nullptr;
    }

    int n() const { return (int)slot.size(); }
    bool ok(int k) const { return k >= 0 && k < n(); }
    void *host(int k, int b) const { return ok(k) ? slot[(size_t)k].h[b] : nullptr; }  // the accessors' answer, NULL for a bad slot
    void *dev(int k, int b) const { return slot[(size_t)k].d[b]; }
    hipEvent_t gate_event(int k) const { return slot[(size_t)k].ev_gate; }
    void set_next(int k) { next = k; }  // a wmx_rt rotates its sub-batches in lockstep, also past a failed one

    // Slot k's previous step has left the device (its download queued if it was still owed, then waited for): the slot's buffers are
    // free.  Completes only what earlier steps promised; a slot not in flight costs nothing.
    int retire(int k) {
        Slot &s = slot[(size_t)k];
        if (!s.in_flight) return 0;
        if (pending == k) {  // one slot only: its download cannot wait for the next step
            const int rc = flush();
            if (rc != 0) return rc;
        }
        WMX_HIP(hipEventSynchronize(s.ev_out));
        s.in_flight = false;
        return 0;
    }
    // the up buffers whose bit is set in `which`, on the copy-in stream; `main` waits for them
    int upload(int k, hipStream_t main, unsigned which = ~0u) {
        const int rc = upload_queue(slot[(size_t)k], main, which);
        if (rc != 0) {
            (void)hipStreamSynchronize(s_in);  // whatever was queued has read the rows: they may be rewritten and submitted again
            (void)hipGetLastError();
        }
        return rc;
    }
    int done(int k, hipStream_t main) {
        WMX_HIP(hipEventRecord(slot[(size_t)k].ev_done, main));
        return 0;
    }
    // The down buffers of slot k, behind `gate` (an event of the compute stream, or NULL) AND the slot's own ev_done: a gate is recorded on
    // whatever stream the gating step was given, and nothing but the caller's habit of using one stream orders that behind slot k's
    // last launch (the second wait costs nothing when the stream is the same).  `which`: the down buffers whose bit is set, as in upload().
    int download(int k, hipEvent_t gate = nullptr, unsigned which = ~0u) {
        Slot &s = slot[(size_t)k];
        if (gate && gate != s.ev_done) WMX_HIP(hipStreamWaitEvent(s_out, gate, 0));
        WMX_HIP(hipStreamWaitEvent(s_out, s.ev_done, 0));
        for (size_t b = 0; b < buf.size(); b++)
            if (!buf[b].up && (which >> b & 1u)) WMX_HIP(hipMemcpyAsync(s.h[b], s.d[b], buf[b].bytes, hipMemcpyDeviceToHost, s_out));
        WMX_HIP(hipEventRecord(s.ev_out, s_out));
        return 0;
    }
    // The download of the pending slot.  WHERE the download of a step is queued matters: the runtime copies device-to-host with a blit
    // kernel (11 - 21 MB of posted writes over PCIe, 0.2 - 0.4 ms), and a memory-bound kernel beside it starves -- the next step's ingest
    // kernel, 15 us alone, took the blit's whole 210 us when the download was queued right behind the egress (rocprofv3 kernel trace,
    // profiles/r05), and the noise suppressor (24 KB of state per stream at 70 % of the HBM peak) is the next most sensitive.  So the pipe
    // commits step k deferred, and its download is queued by submit(k + 1), gated on an event the chain records BEHIND step k + 1's
    // noise suppressor: it runs beside the echo canceller, which is bound by arithmetic.  The last step's download is queued by wait /
    // poll.  (A conference tick's rows are a few KB: wmx_conf downloads at once.)  `pending` is given up only once everything is queued:
    // a flush that fails half-way is simply made again (a second copy of the same rows, then the event).
    int flush(hipEvent_t gate = nullptr) {
        if (pending < 0) return 0;
        const int rc = download(pending, gate);
        if (rc == 0) pending = -1;
        return rc;
    }
    // the step over slot k is queued whole: the only place `next`, `pending` and in_flight move
    void commit(int k, bool deferred) {
        next = (k + 1) % n();
        if (deferred) pending = k;
        slot[(size_t)k].in_flight = true;
    }
    // the failure path behind the first launch: whatever was queued has run, no error is left behind, nothing has moved
    void drain(hipStream_t main, bool with_out) {
        (void)hipStreamSynchronize(s_in);
        (void)hipStreamSynchronize(main);
        if (with_out) (void)hipStreamSynchronize(s_out);
        (void)hipGetLastError();
    }
    // Blocks until the slot's down rows are in host memory (at once for a slot that is not in flight); k < 0: every slot.
    int wait(int k) {
        if (k >= n()) return WMX_EINVAL;
        if (pending >= 0 && (k < 0 || k == pending)) {
            const int rc = flush();
            if (rc != 0) return rc;
        }
        for (int i = 0; i < n(); i++)
            if ((k < 0 || i == k) && slot[(size_t)i].in_flight) {
                WMX_HIP(hipEventSynchronize(slot[(size_t)i].ev_out));
                slot[(size_t)i].in_flight = false;
            }
        return 0;
    }
    // Non-blocking wait: queues the download still owed for k (< 0: any) and returns 1 when the rows of the slot (every slot) are in
    // host memory, 0 when they are still on their way.
    int poll(int k) {
        if (k >= n()) return WMX_EINVAL;
        if (pending >= 0 && (k < 0 || k == pending)) {
            const int rc = flush();
            if (rc != 0) return rc;
        }
        int all = 1;
        for (int i = 0; i < n(); i++) {
            if ((k >= 0 && i != k) || !slot[(size_t)i].in_flight) continue;
            const int r = query(slot[(size_t)i]);
            if (r < 0) return r;
            if (r) slot[(size_t)i].in_flight = false;
            all &= r;
        }
        return all;
    }
    // 1 when slot k's step has landed in host memory, 0 when it has not, < 0 on an error.  The event is queried, never waited for, and
    // nothing is queued or moved: a download still owed has not landed.
    int landed(int k) const {
        if (pending >= 0) return 0;
        return slot[(size_t)k].in_flight ? query(slot[(size_t)k]) : 1;
    }

   private:
    int upload_queue(Slot &s, hipStream_t main, unsigned which) {
        for (size_t b = 0; b < buf.size(); b++)
            if (buf[b].up && (which >> b & 1u)) WMX_HIP(hipMemcpyAsync(s.d[b], s.h[b], buf[b].bytes, hipMemcpyHostToDevice, s_in));
        WMX_HIP(hipEventRecord(s.ev_in, s_in));
        WMX_HIP(hipStreamWaitEvent(main, s.ev_in, 0));
        return 0;
    }
    static int query(const Slot &s) {
        const hipError_t q = hipEventQuery(s.ev_out);
        if (q == hipSuccess) return 1;
        if (q != hipErrorNotReady) return hip_fail(q, "hipEventQuery(ev_out)", __FILE__, __LINE__);
        (void)hipGetLastError();
        return 0;
    }
};

}  // namespace wmx
