// pipe.hip -- the packet edge end to end as a C pipeline (host code only: it sequences copies and launches).
//
// What wmix_thread_rtp_recv_pcma / the record heartbeat / wmix_thread_rtp_send_pcma do for ONE stream per 20 ms
// (src/wmixTask.c:1278-1316: rtp_recv -> G711a2PCM; src/wmix.c:613-709: ns -> aec -> agc -> vad; src/wmixTask.c:1124-1143:
// wmix_pcm_zoom -> PCM2G711a -> timestamp / seq -> rtp_send), for n streams per step with only the 172-byte datagrams crossing PCIe:
//
//     host datagrams --H2D--> wmx_rtp_ingest -> wmx_chain_process (two 10 ms packets, 8 kHz mono, in place) -> wmx_rtp_egress --D2H--> host
//
// A wmx_pipe owns a ring of `slots` slots (slot_ring.h: pinned host rows in and out, their device twins, the copy streams and the
// events, all made once).  wmx_pipe_submit(slot k) queues   H2D on the copy-in stream -> (event) -> ingest, chain, egress on the
// caller's stream -> (event) -> D2H on the copy-out stream -> (event)   and returns at once: while step k computes, the datagrams of
// step k + 1 arrive and those of step k - 1 leave.  wmx_pipe_wait(slot) blocks until that slot's datagrams are in host memory.  The
// host thread waits only when it takes a slot that is still in flight.
//
// wmx_pipe_create_pcm makes the same pipeline for a host that holds PCM -- the heartbeat's own boundary: buffSrc is host memory
// (wmix_ai_read, src/wmix.c:609-612) and the chain works on it in place (:613-709).  A row is then one WMIX_PKG_SIZE package of one
// stream (chn x freq x interval_ms), there is no ingest / egress, and the chain runs in place on the uploaded rows.
#include <vector>
#include "wmx_internal.h"

#include "pipe_internal.h"

using wmx::kDatagram;
using wmx::kPkt10;
constexpr int kFreq = wmx::kPipeFreq;

extern "C" {

int wmx_pipe_destroy(wmx_pipe *h) {
    WMX_ON_DEVICE(h);
    if (!h) return 0;
    (void)hipDeviceSynchronize();
    h->ring.destroy();
    if (h->d_pcm) (void)hipFree(h->d_pcm);
    if (h->d_nbytes) (void)hipFree(h->d_nbytes);
    if (h->d_seq) (void)hipFree(h->d_seq);
    if (h->chain) wmx_chain_destroy(h->chain);
    if (h->snd) wmx_rtp_destroy(h->snd);
    delete h;
    return 0;
}

}  // extern "C"

int wmx::pipe_make(wmx_pipe **out, int n_streams, int slots, bool pcm, int law, int chn, int freq, int interval_ms, int agc_value,
                   unsigned stages, hipStream_t shared_in, hipStream_t shared_out, bool far_rows) {
    wmx_pipe *h = new wmx_pipe();
    if ((h->device = wmx::current_device()) < 0) {
        delete h;
        return WMX_ENODEV;
    }
    h->n_streams = n_streams;
    h->pcm = pcm;
    h->far_rows = far_rows && pcm;
    h->pkt10 = freq / 100 * chn;
    h->ppc = interval_ms / 10;
    h->row_bytes = pcm ? h->pkt10 * h->ppc * 2 : kDatagram;
    h->far_samples = h->pkt10 * h->ppc;
    h->failed_steps = 0;
    // the RTP edge hands the heartbeat 10 ms packets (two per datagram); a PCM host hands it whole packages like the daemon does
    int rc;
    if (h->far_rows) {
        // aec_process2(fp, far, near, ..) takes the far-end per handle (src/webrtc.c:410-483): every stream a control cohort and a far-end
        // history of its own (122 KB each); cohorts made together share one host control plane (aec_ctl.h classes)
        std::vector<int32_t> own((size_t)n_streams);
        for (int i = 0; i < n_streams; i++) own[(size_t)i] = i;
        rc = wmx_chain_create_groups(&h->chain, n_streams, chn, freq, interval_ms, agc_value, stages, n_streams, own.data());
    } else {
        rc = wmx_chain_create(&h->chain, n_streams, chn, freq, pcm ? interval_ms : 10, agc_value, stages, 1);
    }
    if (rc == 0 && !pcm) rc = wmx_rtp_create(&h->snd, n_streams, law);
    hipError_t e = hipSuccess;
    const size_t bytes = (size_t)n_streams * (size_t)h->row_bytes;
    const size_t far_bytes = (size_t)h->far_samples * sizeof(int16_t) * (h->far_rows ? (size_t)n_streams : 1);
    if (rc == 0) {
        if (!pcm) {
            e = hipMalloc(&h->d_pcm, (size_t)n_streams * 2 * kPkt10 * sizeof(int16_t));
            if (e == hipSuccess) e = hipMalloc(&h->d_nbytes, (size_t)n_streams * sizeof(uint32_t));
            if (e == hipSuccess) e = hipMalloc(&h->d_seq, (size_t)n_streams * sizeof(uint16_t));
        }
        // kIn, kOut (the heartbeat works in place on PCM), kFar
        if (e == hipSuccess) e = h->ring.make(slots, {{bytes, true, -1}, {bytes, false, pcm ? 0 : -1}, {far_bytes, true, -1}}, shared_in, shared_out);
        if (e != hipSuccess) rc = wmx::hip_fail(e, "wmx_pipe_create: buffers / streams / events", __FILE__, __LINE__);
    }
    if (rc != 0) {
        wmx_pipe_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" {

// law: WMX_LAW_A (payload type 8, the reference's wmix_thread_rtp_*_pcma) or WMX_LAW_U; stages: WMX_CHAIN_* bits of the heartbeat
int wmx_pipe_create(wmx_pipe **out, int n_streams, int slots, int law, int agc_value, unsigned stages) {
    if (!out) return WMX_EINVAL;
    *out = nullptr;
    if (n_streams < 1 || !wmx::slots_ok(slots) || law != WMX_LAW_A) {
        // (the ingest side decodes A-law as wmix_thread_rtp_recv_pcma does, src/wmixTask.c:1282; a mu-law receiver does not exist in the
        // reference)
        wmx::set_error("wmx_pipe_create: n_streams=%d slots=%d law=%d", n_streams, slots, law);
        return WMX_EINVAL;
    }
    return wmx::pipe_make(out, n_streams, slots, false, law, 1, kFreq, 20, agc_value, stages, nullptr, nullptr);
}

// The heartbeat over PCM in host memory (src/wmix.c:609-709): a row = one package of chn x freq x interval_ms (WMIX_PKG_SIZE bytes),
// processed in place by the chain made with (chn, freq, interval_ms, agc_value, stages); the step's far-end is one package of the
// same format.  Whatever the chain refuses (a rate the enabled stages do not take, ...) is refused here with its error.
int wmx_pipe_create_pcm(wmx_pipe **out, int n_streams, int slots, int chn, int freq, int interval_ms, int agc_value, unsigned stages) {
    if (!out) return WMX_EINVAL;
    *out = nullptr;
    if (n_streams < 1 || !wmx::slots_ok(slots) || (chn != 1 && chn != 2) || freq < 8000 || freq % 100 || interval_ms < 10 || interval_ms % 10 ||
        interval_ms > 100) {
        wmx::set_error("wmx_pipe_create_pcm: n_streams=%d slots=%d chn=%d freq=%d interval_ms=%d", n_streams, slots, chn, freq, interval_ms);
        return WMX_EINVAL;
    }
    return wmx::pipe_make(out, n_streams, slots, true, 0, chn, freq, interval_ms, agc_value, stages, nullptr, nullptr);
}

// The same for CALLS: every stream hears a far-end of its own, as every handle of the reference does (aec_process2(fp, far, near, ..),
// src/webrtc.c:410-483; in a telephony server the far-end of a call is the other party).  wmx_pipe_far(h, slot) then is n_streams rows of
// one package each (stream-major like the near rows), d_far of wmx_pipe_submit / _step_resident likewise.
int wmx_pipe_create_pcm_calls(wmx_pipe **out, int n_streams, int slots, int chn, int freq, int interval_ms, int agc_value, unsigned stages) {
    if (!out) return WMX_EINVAL;
    *out = nullptr;
    if (n_streams < 1 || !wmx::slots_ok(slots) || (chn != 1 && chn != 2) || freq < 8000 || freq % 100 || interval_ms < 10 || interval_ms % 10 ||
        interval_ms > 100 || !(stages & WMX_CHAIN_AEC) || (stages & WMX_CHAIN_AECM)) {
        wmx::set_error("wmx_pipe_create_pcm_calls: n_streams=%d slots=%d chn=%d freq=%d interval_ms=%d stages=0x%x (the float canceller must be on)", n_streams,
                       slots, chn, freq, interval_ms, stages);
        return WMX_EINVAL;
    }
    return wmx::pipe_make(out, n_streams, slots, true, 0, chn, freq, interval_ms, agc_value, stages, nullptr, nullptr, true);
}

int wmx_pipe_slots(const wmx_pipe *h) { return h ? h->ring.n() : WMX_EINVAL; }
int wmx_pipe_datagram_bytes(const wmx_pipe *h) { return h ? h->row_bytes : WMX_EINVAL; }  // 172, or the package bytes of a PCM pipe
long wmx_pipe_failed_steps(const wmx_pipe *h) { return h ? h->failed_steps : WMX_EINVAL; }
// the pinned host rows of a slot: n_streams rows of wmx_pipe_datagram_bytes in / out, and the far-end samples of the slot's step
uint8_t *wmx_pipe_in(wmx_pipe *h, int slot) { return h ? static_cast<uint8_t *>(h->ring.host(slot, wmx_pipe::kIn)) : nullptr; }
const uint8_t *wmx_pipe_out(wmx_pipe *h, int slot) { return h ? static_cast<uint8_t *>(h->ring.host(slot, wmx_pipe::kOut)) : nullptr; }
int16_t *wmx_pipe_far(wmx_pipe *h, int slot) { return h ? static_cast<int16_t *>(h->ring.host(slot, wmx_pipe::kFar)) : nullptr; }
wmx_chain *wmx_pipe_chain(wmx_pipe *h) { return h ? h->chain : nullptr; }
wmx_rtp *wmx_pipe_senders(wmx_pipe *h) { return h ? h->snd : nullptr; }

static int pipe_ingest(wmx_pipe *h, const uint8_t *d_in, long in_stride, void *stream) {
    if (h->pcm) return 0;
    return wmx_rtp_ingest(h->n_streams, d_in, in_stride, h->d_pcm, 2 * kPkt10, h->d_nbytes, h->d_seq, stream);
}
static int pipe_chain_egress(wmx_pipe *h, const int16_t *d_far, const uint8_t *d_in, long in_stride, uint8_t *d_out, long out_stride,
                             void *stream) {
    if (h->pcm && h->far_rows)  // far rows like near rows: stream s hears the package at d_far + s * far_samples
        return wmx_chain_process_groups(h->chain, d_far, h->pkt10, h->far_samples, reinterpret_cast<const int16_t *>(d_in),
                                        reinterpret_cast<int16_t *>(d_out), h->ppc, out_stride / 2, h->pkt10, nullptr, nullptr, nullptr, stream);
    if (h->pcm)  // rows are packages: ppc packets of pkt10 samples, stream rows in_stride / out_stride BYTES apart
        return wmx_chain_process(h->chain, d_far, h->pkt10, reinterpret_cast<const int16_t *>(d_in), reinterpret_cast<int16_t *>(d_out), h->ppc,
                                 out_stride / 2, h->pkt10, nullptr, nullptr, nullptr, stream);
    int rc = wmx_chain_process(h->chain, d_far, kPkt10, h->d_pcm, h->d_pcm, 2, 2 * kPkt10, kPkt10, nullptr, nullptr, nullptr, stream);
    if (rc != 0) return rc;
    uint32_t bytes = 0;
    rc = wmx_rtp_egress(h->snd, 1, kFreq, h->d_pcm, 2 * kPkt10 * 2, 2 * kPkt10, 1, kFreq, d_out, out_stride, &bytes, stream);
    if (rc == 0 && bytes != (uint32_t)kDatagram) {
        wmx::set_error("wmx_pipe: egress made %u-byte datagrams", bytes);
        return WMX_ESTATE;
    }
    return rc;
}

// One step on datagrams that are ALREADY on the device: ingest -> chain -> egress, three launches' worth of calls on `stream`.
// d_in / d_out: n_streams rows of 172 bytes, in_stride / out_stride bytes apart; d_far: the shared far-end's two 10 ms packets.
int wmx_pipe_step_resident(wmx_pipe *h, const uint8_t *d_in, long in_stride, const int16_t *d_far, uint8_t *d_out, long out_stride,
                           void *stream) {
    WMX_ON_DEVICE(h);
    if (!h || !d_in || !d_out || !d_far || in_stride < h->row_bytes || out_stride < h->row_bytes || (h->pcm && (in_stride != out_stride || in_stride % 2))) {
        wmx::set_error("wmx_pipe_step_resident: bad argument");
        return WMX_EINVAL;
    }
    const int rc = pipe_ingest(h, d_in, in_stride, stream);
    return rc ? rc : pipe_chain_egress(h, d_far, d_in, in_stride, d_out, out_stride, stream);
}

}  // extern "C"

// wmx_pipe_submit (and the sub-batch form of rt.hip): one step of the slot ring (slot_ring.h; FAILING CLEAN there), its download
// deferred to the next submit's gate behind the noise suppressor.
int wmx::pipe_submit(wmx_pipe *h, const int16_t *d_far, int *slot, void *stream, wmx_pipe *flush_for, const wmx_pipe *far_of) {
    wmx::SlotRing &ring = h->ring, &fl = flush_for ? flush_for->ring : h->ring;
    const int k = ring.next;
    hipStream_t main = wmx::as_stream(stream);
    // taking the slot: these calls only complete what earlier submits promised (the slot's previous download, and for a sub-batch its
    // own download of an earlier tick nobody waited for)
    int rc = ring.retire(k);
    if (rc == 0 && &fl != &ring) rc = ring.flush();
    if (rc != 0) return rc;
    uint8_t *d_in = static_cast<uint8_t *>(ring.dev(k, wmx_pipe::kIn)), *d_out = static_cast<uint8_t *>(ring.dev(k, wmx_pipe::kOut));
    const int16_t *far = d_far ? d_far : static_cast<const int16_t *>((far_of ? far_of->ring : ring).dev(k, wmx_pipe::kFar));
    rc = ring.upload(k, main, (!d_far && !far_of) ? ~0u : ~(1u << wmx_pipe::kFar));
    if (rc != 0) return rc;
    const bool gated = fl.pending >= 0;
    auto launches = [&]() -> int {
        int r = pipe_ingest(h, d_in, h->row_bytes, stream);
        if (r != 0) return r;
        if (gated) wmx::chain_gate_after_ns(h->chain, ring.gate_event(k));  // recorded by the chain call below, behind its noise suppressor
        r = pipe_chain_egress(h, far, d_in, h->row_bytes, d_out, h->row_bytes, stream);
        if (r != 0) return r;
        if (gated && (r = fl.flush(ring.gate_event(k))) != 0) return r;  // the wait is queued after the record was: the event is this step's
        return ring.done(k, main);
    };
    rc = launches();
    if (rc != 0) {
        char why[512];
        snprintf(why, sizeof(why), "%s", wmx_last_error());
        wmx::chain_gate_after_ns(h->chain, nullptr);  // a gate the chain never reached must not fire in a later call
        ring.drain(main, false);
        h->failed_steps++;
        wmx::set_error("wmx_pipe_submit: the step is lost (%s)", why);
        return rc;
    }
    ring.commit(k, true);
    if (slot) *slot = k;
    return 0;
}

extern "C" {

// Queue the next slot: its h_in rows (and, when d_far is NULL, its h_far samples) must hold this step's input.  *slot receives the
// slot index; its h_out rows are valid after wmx_pipe_wait(h, *slot).  Blocks only if that slot is still in flight from `slots`
// steps ago.  d_far != NULL: the far-end is on the device already (its two 10 ms packets, contiguous).
int wmx_pipe_submit(wmx_pipe *h, const int16_t *d_far, int *slot, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    return wmx::pipe_submit(h, d_far, slot, stream, nullptr, nullptr);
}

// Blocks until the slot's datagrams are in its h_out rows (returns at once for a slot that is not in flight); slot < 0: every slot.
int wmx_pipe_wait(wmx_pipe *h, int slot) {
    WMX_ON_DEVICE(h);
    return h ? h->ring.wait(slot) : WMX_EINVAL;
}

// Non-blocking wmx_pipe_wait: queues the download still owed for `slot` (< 0: any) and returns 1 when the rows of the slot (every
// slot) are in host memory, 0 when they are still on their way.
int wmx_pipe_poll(wmx_pipe *h, int slot) {
    WMX_ON_DEVICE(h);
    return h ? h->ring.poll(slot) : WMX_EINVAL;
}

}  // extern "C"

