// conf.hip -- a conference bridge of RTP/G.711 legs in one handle, datagram in, datagram out (host code only: it sequences copies and
// launches, like pipe.hip).
//
// What the daemon runs as one wmix_thread_rtp_recv_pcma per leg (src/wmixTask.c:1266-1316: rtp_recv -> G711a2PCM -> wmix_load_data with
// the thread's own cursor), the play thread (src/wmix.c:1347-1366) and one wmix_thread_rtp_send_pcma per leg (src/wmixTask.c:1058-1143),
// for n_legs legs per 20 ms tick with only datagrams crossing PCIe:
//
//     host rows --H2D--> wmx_rtp_ingest_legs_codecs -> [wmx_mix_select_speakers_legs] -> wmx_mix_load_minus_legs -> wmx_rtp_egress_rings --D2H--> host
//
// With sequencing on (wmx_conf_sequence) the ingest also leaves the sequence numbers, wmx_rtp_sequence_legs turns them into a call list
// per leg and rewrites d_len in front of the selection, and the load is wmx_mix_load_minus_legs_calls.  The ingest and the egress
// apply each leg's own G.711 codec (wmx_conf_set_codecs; wmix_amd/csrc/leg_codec.h); a handle that never sets one runs the
// reference's A-law-whatever-arrives and one law out.  With concealment on as well (wmx_conf_conceal) wmx_rtp_conceal_legs stands
// between the selection and the load: it turns every leg's list into rows that are all data -- a lost packet synthesised from the
// leg's own history (wmix_amd/csrc/leg_plc.h) -- and the load is wmx_mix_load_minus_legs on those.  With denoising on
// (wmx_conf_denoise) wmx_nsx_process_legs stands behind the sequencer and the DTMF detection and in front of the selection: each leg's
// rows of the tick go through the leg's own fixed-point noise suppressor in place, in the order the load will consume them.  With
// levelling on (wmx_conf_level) wmx_agc_process_legs stands directly behind it: the same rows, in the same order, through the leg's own
// AGC with the leg's own compression gain.  With the gate on (wmx_conf_gate) wmx_vad_process_legs stands directly behind that: the same
// rows, in the same order, each one vad_process of the leg's own voice-activity gate, which shifts the row right by the leg's `reduce`.
// With echo control on (wmx_conf_echo) wmx_aecm_process_legs stands between the denoiser and the leveller -- the heartbeat's order --
// with the rows alone, and a second time behind the egress with the far row alone: what wmx_rtp_decode_sent_legs makes of the
// datagram the tick has just sent to the leg.  With a prompt store (wmx_conf_prompts) wmx_mix_load_prompts stands behind the load and in
// front of the egress: every leg that plays a clip loads its next 20 ms into its own ring (wmix_amd/csrc/leg_prompt.h), behind what the
// other legs of its conference loaded there.  With a recording store (wmx_conf_recorders) wmx_rtp_record_rings stands behind that and
// directly in front of the egress, in the ticks in which a tap is running: what the egress is about to encode for a tapped leg, as PCM
// in the store's format (wmix_amd/csrc/leg_record.h), into two more `down` buffers of the slot.
//
// PER SLOT (slot_ring.h, made once, `slots` of them): pinned host rows -- n_legs x max_packets datagram rows of 176 bytes (172 on a
// 4-byte boundary), what recvfrom returned per row, n_legs x 172 bytes out -- their device twins and the events.  PER HANDLE: the mixer
// (rings, layout, leg cursors, envelopes), the senders, the PCM rows between ingest and load, d_len, the host's mute and the mask
// talker selection writes for the load, the ring's copy-in and copy-out stream.  wmx_conf_submit(slot k) queues H2D on the copy-in stream
// -> (event) -> the launches on the caller's stream -> (event) -> D2H on the copy-out stream -> (event) and returns at once: with three
// slots the upload of tick t + 1 and the download of tick t - 1 run beside the launches of tick t.  The per-handle buffers are shared
// by every tick, so the handle takes ONE compute stream, like wmx_pipe.
#include <vector>
#include "pipe_internal.h"
#include "leg_calls.h"
#include "leg_state.h"

namespace {
using wmx::kLegRow;
using wmx::kLegRowBytes;
constexpr int kInRow = 176;    // a datagram row in: 172 bytes, rows on 4-byte boundaries
using wmx::kDatagram;  // a datagram out: 12-byte RTP header + 160 G.711 codes
static_assert(wmx::kLegMaxCalls == WMX_MIX_MAX_LEG_PACKETS, "leg_calls.h and include/wmix_amd.h name one limit");
}  // namespace

struct wmx_conf {
    int device;  // first member of every handle (wmx_handle_device)
    int n_legs, max_packets;
    wmx_mix *mix;
    wmx_rtp *snd;
    int16_t *d_pcm;    // [n_legs][max_packets][160] between ingest and load
    uint32_t *d_len;   // [n_legs][max_packets] 320 for a slot that is a call
    uint16_t *d_seq;   // [n_legs][max_packets] header bytes 2..3 as stored (sequencing on)
    uint32_t *d_calls; // [n_legs] the call list the sequencer leaves for the load
    bool seq_on;
    int max_gap;
    bool conceal_on;      // only with seq_on: wmx_rtp_conceal_legs between the selection and the load
    int16_t *d_rep;       // [n_legs][4][160] the repaired rows, made when concealment is first switched on
    uint32_t *d_rep_len;  // [n_legs][4], behind them
    bool dtmf_on, dtmf_suppress, dtmf_made;  // wmx_rtp_detect_dtmf_legs in front of the selection; made: the senders hold its state
    int dtmf_pt;
    bool denoise_on;  // wmx_nsx_process_legs in front of the selection
    wmx_nsx *nsx;     // a suppressor stream per leg, made when denoising is first switched on
    bool level_on;    // wmx_agc_process_legs behind the denoiser
    wmx_agc *agc;     // an AGC stream per leg, made when levelling is first switched on
    int level_value;  // the compression gain wmx_conf_level last gave every leg
    bool gate_on;      // wmx_vad_process_legs behind the leveller
    wmx_vad *vad;      // a VAD stream per leg (1 x 8000, 20 ms), made when the gate is first switched on
    wmx::LegState gate;  // rows judged voice / not voice per leg ([2][n_legs]: a table of two columns, leg_state.h), made with it
    bool echo_on;         // wmx_aecm_process_legs behind the denoiser (rows) and behind the egress (the far row)
    wmx_aecm *aecm;       // a canceller per leg (wmx_aecm_create_legs), made when echo control is first switched on
    int16_t *d_echo_far;  // [n_legs][160] what the tick sent to each leg, decoded; made with it
    bool prompts_made;  // wmx_mix_load_prompts behind the load: the mixer holds the store (wmx_conf_prompts)
    bool rec_made;      // wmx_rtp_record_rings in front of the egress: the senders hold the store (wmx_conf_recorders)
    int rec_taps;       // the store's taps and the bytes of a row: the slots' kRec is rec_taps rows, kRecLegs rec_taps int32
    size_t rec_row_bytes;
    uint8_t *d_mute;   // [n_legs] the host's mute
    uint8_t *d_mask;   // [n_legs] what selection leaves for the load
    uint8_t *h_mute;   // pinned: the upload's source
    bool mute_on;
    int max_speakers, decay_shift;  // max_speakers 0: selection off
    uint32_t floor;
    enum { kIn, kRecv, kOut, kRec, kRecLegs };  // the slots' buffers (slot_ring.h); the last two from wmx_conf_recorders on
    wmx::SlotRing ring;
};

// the launches of one tick on rows that are on the device; d_rec NULL: the taps are not launched (no store, or none is running)
static int conf_launches(wmx_conf *h, const uint8_t *d_in, const int32_t *d_recv, uint8_t *d_out, int16_t *d_rec, long rec_stride,
                         int32_t *d_rec_legs, void *stream) {
    const int K = h->max_packets;
    const uint32_t *calls = h->seq_on ? h->d_calls : nullptr;  // the stages' order: the sequencer's list, or the slots'
    int rc = wmx_rtp_ingest_legs_codecs(h->snd, K, d_in, (long)K * kInRow, kInRow, d_recv, h->d_pcm, (long)K * kLegRow, kLegRow, h->d_len,
                                        h->seq_on ? h->d_seq : nullptr, stream);
    if (rc != 0) return rc;
    if (h->seq_on) {  // in front of the selection: it must not hear a late packet or a duplicate
        rc = wmx_rtp_sequence_legs(h->snd, K, h->max_gap, h->d_seq, h->d_len, h->d_calls, stream);
        if (rc != 0) return rc;
    }
    if (h->dtmf_on) {  // in front of the selection: it and the load must see a suppressed row
        rc = wmx_rtp_detect_dtmf_legs(h->snd, K, d_in, (long)K * kInRow, kInRow, d_recv, h->d_pcm, (long)K * kLegRow, kLegRow, h->d_len,
                                      calls, h->dtmf_pt, h->dtmf_suppress ? 1 : 0, stream);
        if (rc != 0) return rc;
    }
    if (h->denoise_on) {  // behind the keypad, which is judged on the row as it arrived; selection, concealment and the load see the cleaned rows
        rc = wmx_nsx_process_legs(h->nsx, h->d_pcm, (long)K * kLegRow, kLegRow, K, h->d_len, calls, stream);
        if (rc != 0) return rc;
    }
    if (h->echo_on) {  // behind the denoiser and in front of the leveller, the heartbeat's order (NS -> AEC -> AGC -> VAD): the rows only
        rc = wmx_aecm_process_legs(h->aecm, h->d_pcm, (long)K * kLegRow, kLegRow, K, h->d_len, calls, nullptr, 0, stream);
        if (rc != 0) return rc;
    }
    if (h->level_on) {  // behind the denoiser: the level detector hears the cleaned row; selection, concealment and the load see the levelled rows
        rc = wmx_agc_process_legs(h->agc, h->d_pcm, (long)K * kLegRow, kLegRow, K, h->d_len, calls, stream);
        if (rc != 0) return rc;
    }
    if (h->gate_on) {  // behind the leveller: the decision is made on the levelled row; selection, concealment and the load see the gated rows
        rc = wmx_vad_process_legs(h->vad, h->d_pcm, (long)K * kLegRow, kLegRow, K, h->d_len, calls, h->gate.at<uint32_t>(wmx::kGateVoiced), stream);
        if (rc != 0) return rc;
    }
    const uint8_t *host_mute = h->mute_on ? h->d_mute : nullptr, *load_mute = host_mute;
    if (h->max_speakers > 0) {
        rc = wmx_mix_select_speakers_legs(h->mix, h->d_pcm, kLegRowBytes, (long)K * kLegRow, kLegRow, K, h->d_len, host_mute, h->max_speakers,
                                          h->floor, h->decay_shift, h->d_mask, stream);
        if (rc != 0) return rc;
        load_mute = h->d_mask;
    }
    if (h->seq_on && h->conceal_on) {  // every call becomes a data call: the plain load, four slots
        constexpr int C = WMX_MIX_MAX_LEG_PACKETS;
        rc = wmx_rtp_conceal_legs(h->snd, K, h->d_pcm, (long)K * kLegRow, kLegRow, h->d_len, h->d_calls, h->d_rep, h->d_rep_len, stream);
        if (rc != 0) return rc;
        rc = wmx_mix_load_minus_legs(h->mix, h->d_rep, kLegRowBytes, 8000, 1, 16, (long)C * kLegRow, kLegRow, C, h->d_rep_len, load_mute, 1, stream);
    } else if (h->seq_on)
        rc = wmx_mix_load_minus_legs_calls(h->mix, h->d_pcm, kLegRowBytes, 8000, 1, 16, (long)K * kLegRow, kLegRow, K, h->d_len, h->d_calls, load_mute,
                                           1, stream);
    else
        rc = wmx_mix_load_minus_legs(h->mix, h->d_pcm, kLegRowBytes, 8000, 1, 16, (long)K * kLegRow, kLegRow, K, h->d_len, load_mute, 1, stream);
    if (rc != 0) return rc;
    if (h->prompts_made) {  // behind the legs' calls, so that a ring receives its prompt's call last; in front of the drain
        rc = wmx_mix_load_prompts(h->mix, stream);
        if (rc != 0) return rc;
    }
    if (d_rec) {  // behind everything that loads a ring, so that the row is what the egress encodes; it zeroes nothing
        rc = wmx_rtp_record_rings(h->snd, h->mix, d_rec, rec_stride, d_rec_legs, stream);
        if (rc != 0) return rc;
    }
    uint32_t bytes = 0;
    rc = wmx_rtp_egress_rings(h->snd, h->mix, d_out, kDatagram, &bytes, stream);
    if (rc == 0 && bytes != (uint32_t)kDatagram) {
        wmx::set_error("wmx_conf: egress made %u-byte datagrams", bytes);
        return WMX_ESTATE;
    }
    if (rc == 0 && h->echo_on) {  // the far end of leg g is the datagram just made for it, as its speaker plays it: far only
        rc = wmx_rtp_decode_sent_legs(h->snd, d_out, kDatagram, h->d_echo_far, kLegRow, stream);
        if (rc == 0) rc = wmx_aecm_process_legs(h->aecm, nullptr, 0, 0, 1, nullptr, nullptr, h->d_echo_far, kLegRow, stream);
    }
    return rc;
}

// the listed legs' streams (NULL = all) of a per-leg stage as its init leaves them: the suppressor (ns_init), the AGC (agc_init, each
// leg with the compression gain it has), the gate (vad_init: `reduce` back to 4)
template <class Stage>
static int conf_reset_stage(wmx_conf *h, Stage *stage, int (*reset_streams)(Stage *, const int32_t *, int, void *), const int32_t *host_idx,
                            int n, void *stream) {
    if (host_idx) return n > 0 ? reset_streams(stage, host_idx, n, stream) : 0;
    std::vector<int32_t> all((size_t)h->n_legs);
    for (int g = 0; g < h->n_legs; g++) all[(size_t)g] = g;
    return reset_streams(stage, all.data(), h->n_legs, stream);
}

extern "C" {

int wmx_conf_destroy(wmx_conf *h) {
    WMX_ON_DEVICE(h);
    if (!h) return 0;
    (void)hipDeviceSynchronize();
    h->ring.destroy();
    if (h->d_pcm) (void)hipFree(h->d_pcm);
    if (h->d_len) (void)hipFree(h->d_len);
    if (h->d_calls) (void)hipFree(h->d_calls);  // d_seq lies behind it
    if (h->d_rep) (void)hipFree(h->d_rep);  // d_rep_len lies behind it
    if (h->d_mute) (void)hipFree(h->d_mute);  // d_mask lies behind it
    if (h->h_mute) (void)hipHostFree(h->h_mute);
    if (h->nsx) wmx_nsx_destroy(h->nsx);
    if (h->agc) wmx_agc_destroy(h->agc);
    if (h->vad) wmx_vad_destroy(h->vad);
    h->gate.destroy();
    if (h->aecm) wmx_aecm_destroy(h->aecm);
    if (h->d_echo_far) (void)hipFree(h->d_echo_far);
    if (h->mix) wmx_mix_destroy(h->mix);
    if (h->snd) wmx_rtp_destroy(h->snd);
    delete h;
    return 0;
}

// law: WMX_LAW_A or WMX_LAW_U of what is SENT, every leg's initial out_law; every payload received is decoded as A-law, as the
// reference's receive thread does, until wmx_conf_set_codecs says what a leg negotiated
int wmx_conf_create(wmx_conf **out, int n_legs, int slots, int max_packets, int law) {
    if (!out) return WMX_EINVAL;
    *out = nullptr;
    if (n_legs < 1 || !wmx::slots_ok(slots) || max_packets < 1 || max_packets > WMX_MIX_MAX_LEG_PACKETS || (law != WMX_LAW_A && law != WMX_LAW_U)) {
        wmx::set_error("wmx_conf_create: n_legs=%d slots=%d (1 .. %d) max_packets=%d (1 .. %d) law=%d", n_legs, slots, wmx::kMaxSlots,
                       max_packets, WMX_MIX_MAX_LEG_PACKETS, law);
        return WMX_EINVAL;
    }
    wmx_conf *h = new wmx_conf();
    if ((h->device = wmx::current_device()) < 0) {
        delete h;
        return WMX_ENODEV;
    }
    h->n_legs = n_legs;
    h->max_packets = max_packets;
    h->gate = wmx::LegState("hipMemset(gate counters)", "handle", n_legs, wmx::kLegGateColumns);
    const size_t rows = (size_t)n_legs * (size_t)max_packets;
    int rc = wmx_mix_create(&h->mix, n_legs, 1, 8000);
    if (rc == 0) rc = wmx_rtp_create(&h->snd, n_legs, law);
    // the cursors and the envelopes are made by the first call that needs them: here, so that no submit allocates
    if (rc == 0) rc = wmx_mix_reset_leg_cursors(h->mix, nullptr, 0, nullptr);
    if (rc == 0) rc = wmx_mix_reset_speakers(h->mix, nullptr, 0, nullptr);
    if (rc == 0) rc = wmx_rtp_reset_sequence(h->snd, nullptr, 0, nullptr);
    if (rc == 0) rc = wmx_rtp_set_codecs(h->snd, nullptr, 0, WMX_CODEC_REFERENCE, law, nullptr);
    if (rc == 0) {
        hipError_t e = hipMalloc(&h->d_pcm, rows * kLegRow * sizeof(int16_t));
        if (e == hipSuccess) e = hipMalloc(&h->d_len, rows * sizeof(uint32_t));
        const size_t calls_bytes = (size_t)n_legs * sizeof(uint32_t), seq_bytes = rows * sizeof(uint16_t);
        if (e == hipSuccess) e = hipMalloc(&h->d_calls, calls_bytes + 4 + seq_bytes);
        if (e == hipSuccess) e = hipMemset(h->d_calls, 0, calls_bytes + 4 + seq_bytes);
        if (e == hipSuccess) h->d_seq = reinterpret_cast<uint16_t *>(h->d_calls + (n_legs + 1) / 2 * 2);  // on an 8-byte boundary
        if (e == hipSuccess) e = hipMalloc(&h->d_mute, 2 * (size_t)n_legs);
        if (e == hipSuccess) e = hipMemset(h->d_mute, 0, 2 * (size_t)n_legs);
        if (e == hipSuccess) e = hipMemset(h->d_len, 0, rows * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemset(h->d_pcm, 0, rows * kLegRow * sizeof(int16_t));
        if (e == hipSuccess) h->d_mask = h->d_mute + n_legs;
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&h->h_mute), (size_t)n_legs, hipHostMallocDefault);
        // kIn, kRecv, kOut
        if (e == hipSuccess) e = h->ring.make(slots, {{rows * kInRow, true, -1}, {rows * sizeof(int32_t), true, -1}, {(size_t)n_legs * kDatagram, false, -1}});
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = wmx::hip_fail(e, "wmx_conf_create: buffers / streams / events", __FILE__, __LINE__);
    }
    if (rc != 0) {
        wmx_conf_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

// ---- setters: between submits, each ordered on `stream`
int wmx_conf_set_conferences(wmx_conf *h, int n_conf, const int32_t *host_off, const int32_t *host_members, void *stream) {
    if (!h) return WMX_EINVAL;
    return wmx_mix_set_conferences(h->mix, n_conf, host_off, host_members, stream);
}

// host_mask: n_legs bytes by leg, non-zero = that leg is loaded nowhere (it still hears the others); NULL = nobody is muted
int wmx_conf_mute(wmx_conf *h, const uint8_t *host_mask, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    if (!host_mask) {
        h->mute_on = false;
        return 0;
    }
    hipStream_t s = wmx::as_stream(stream);
    WMX_HIP(hipStreamSynchronize(s));  // an earlier upload has left h_mute, and no launch in flight reads a mask half written
    memcpy(h->h_mute, host_mask, (size_t)h->n_legs);
    WMX_HIP(hipMemcpyAsync(h->d_mute, h->h_mute, (size_t)h->n_legs, hipMemcpyHostToDevice, s));
    h->mute_on = true;
    return 0;
}

// max_speakers 0 = selection off; else the arguments of wmx_mix_select_speakers_legs
int wmx_conf_speakers(wmx_conf *h, int max_speakers, uint32_t floor, int decay_shift) {
    if (!h) return WMX_EINVAL;
    if (max_speakers < 0 || max_speakers > WMX_MIX_MAX_PARTIES || decay_shift < 0 || decay_shift > 31) {
        wmx::set_error("wmx_conf_speakers: max_speakers=%d must be 0 .. %d and decay_shift=%d 0 .. 31", max_speakers, WMX_MIX_MAX_PARTIES, decay_shift);
        return WMX_EINVAL;
    }
    h->max_speakers = max_speakers;
    h->floor = floor;
    h->decay_shift = decay_shift;
    return 0;
}

// on != 0: the legs' packets are put in sequence order, late packets and duplicates make no call and a gap of up to max_gap packets
// becomes silence calls (wmx_rtp_sequence_legs); 0: the reference's arrival order.  Between submits.
int wmx_conf_sequence(wmx_conf *h, int on, int max_gap) {
    if (!h) return WMX_EINVAL;
    if (max_gap < 0 || max_gap > WMX_MIX_MAX_LEG_PACKETS - 1) {
        wmx::set_error("wmx_conf_sequence: max_gap=%d must be 0 .. %d", max_gap, WMX_MIX_MAX_LEG_PACKETS - 1);
        return WMX_EINVAL;
    }
    h->seq_on = on != 0;
    h->max_gap = max_gap;
    return 0;
}

// on != 0: with sequencing on, the silence calls of a gap are synthesised from the leg's own history and the packet behind the gap is
// cross-faded in (wmx_rtp_conceal_legs); 0 (the default): zeros, the launches of a handle that never heard of it.  Between submits.
// The repaired rows and the history are made the first time it is switched on.
int wmx_conf_conceal(wmx_conf *h, int on) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    if (on && !h->d_rep) {
        const size_t rows = (size_t)h->n_legs * WMX_MIX_MAX_LEG_PACKETS;
        void *p = nullptr;
        int rc = wmx::zeroed_block(&p, rows * (kLegRow * sizeof(int16_t) + sizeof(uint32_t)), "hipMemset(repaired rows)");
        if (rc == 0 && (rc = wmx_rtp_reset_conceal(h->snd, nullptr, 0, nullptr)) != 0) (void)hipFree(p);
        if (rc != 0) return rc;
        h->d_rep = static_cast<int16_t *>(p);
        h->d_rep_len = reinterpret_cast<uint32_t *>(h->d_rep + rows * kLegRow);
    }
    h->conceal_on = on != 0;
    return 0;
}

// concealed (uint32) of every leg (wmx_rtp_export_conceal); blocking
int wmx_conf_export_conceal(wmx_conf *h, uint32_t *concealed, void *stream) {
    if (!h) return WMX_EINVAL;
    return wmx_rtp_export_conceal(h->snd, nullptr, concealed, stream);
}

// on != 0: every leg's keypad is listened to, in band and in RFC 4733 packets of payload type event_pt (wmx_rtp_detect_dtmf_legs);
// suppress != 0: a block that is a tone goes on as zeros.  0 (the default): the launches of a handle that never heard of it.  Between
// submits.  The state is made the first time it is switched on.
int wmx_conf_dtmf(wmx_conf *h, int on, int suppress, int event_pt) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    if (event_pt < 96 || event_pt > 127) {
        wmx::set_error("wmx_conf_dtmf: event_pt=%d must be 96 .. 127 (a dynamic payload type; 101 in most offers)", event_pt);
        return WMX_EINVAL;
    }
    if (on && !h->dtmf_made) {
        const int rc = wmx_rtp_reset_dtmf(h->snd, nullptr, 0, nullptr);
        if (rc != 0) return rc;
        h->dtmf_made = true;
    }
    h->dtmf_on = on != 0;
    h->dtmf_suppress = suppress != 0;
    h->dtmf_pt = event_pt;
    return 0;
}

// count (uint32) and ring (8 uint8) of every leg (wmx_rtp_export_dtmf); blocking
int wmx_conf_export_dtmf(wmx_conf *h, uint32_t *count, uint8_t *ring, void *stream) {
    if (!h) return WMX_EINVAL;
    return wmx_rtp_export_dtmf(h->snd, count, ring, stream);
}

// on != 0: every leg's rows of the tick go through the leg's own fixed-point noise suppressor (wmx_nsx_process_legs: 1 x 8000, the
// policy ns_init sets) behind the DTMF detection and in front of the selection; 0 (the default): the launches of a handle that never
// heard of it.  Between submits.  The suppressor is made the first time it is switched on; off and on again keeps its state.
int wmx_conf_denoise(wmx_conf *h, int on) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    if (on && !h->nsx) {
        const int rc = wmx_nsx_create(&h->nsx, h->n_legs, 1, 8000);
        if (rc != 0) return rc;
    }
    h->denoise_on = on != 0;
    return 0;
}

// the legs' suppressor, for wmx_nsx_export_stream / wmx_nsx_import_stream on a leg; NULL until denoising is first switched on
wmx_nsx *wmx_conf_denoiser(wmx_conf *h) { return h ? h->nsx : nullptr; }

// on != 0: every leg's rows of the tick go through the leg's own AGC (wmx_agc_process_legs: 1 x 8000, interval 10 ms, compression gain
// `value` dB as agc_init takes it) directly behind the denoiser and in front of the selection; 0 (the default): the launches of a handle
// that never heard of it.  Between submits.  The AGC is made the first time it is switched on; on a made one another `value` is
// agc_addition for every leg (wmx_agc_set_gain: the state stays), and off and on again keeps state and gains.  A value the AGC refuses
// changes nothing, the switch included; off does not look at the value.
int wmx_conf_level(wmx_conf *h, int on, int value) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    if (!on) {
        h->level_on = false;
        return 0;
    }
    if (!h->agc) {
        const int rc = wmx_agc_create(&h->agc, h->n_legs, 1, 8000, 10, value);
        if (rc != 0) return rc;
        h->level_value = value;
    } else if (value != h->level_value) {
        const int rc = wmx_agc_set_gain(h->agc, value);
        if (rc != 0) return rc;
        h->level_value = value;
    }
    h->level_on = true;
    return 0;
}

// the legs' AGC, for wmx_agc_set_gain_streams / wmx_agc_stream_gain / wmx_agc_export_stream / wmx_agc_import_stream on a leg; NULL until
// levelling is first switched on
wmx_agc *wmx_conf_leveller(wmx_conf *h) { return h ? h->agc : nullptr; }

// on != 0: every leg's rows of the tick go through the leg's own voice-activity gate (wmx_vad_process_legs: 1 x 8000, 20 ms, one row
// one vad_process) directly behind the leveller and in front of the selection; 0 (the default): the launches of a handle that never
// heard of it.  Between submits.  The VAD and the handle's counters are made the first time it is switched on -- every leg's `reduce`
// at 4, as vad_init leaves it --; off and on again keeps both.
int wmx_conf_gate(wmx_conf *h, int on) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    if (on && !h->vad) {
        int rc = h->gate.make();
        if (rc == 0) rc = wmx_vad_create(&h->vad, h->n_legs, 1, 8000, 20);
        if (rc != 0) return rc;
    }
    h->gate_on = on != 0;
    return 0;
}

// the legs' VAD, for wmx_vad_export_stream / wmx_vad_import_stream / wmx_vad_export_reduce; NULL until the gate is first switched on
wmx_vad *wmx_conf_gater(wmx_conf *h) { return h ? h->vad : nullptr; }

// reduce (uint8, 0 .. 4) and the rows judged voice / not voice (uint32) of every leg as the work queued on `stream` leaves them; any
// pointer may be NULL; blocking.  Before the first switch-on: reduce 4, counts 0 -- what the first switch-on makes.
int wmx_conf_export_gate(wmx_conf *h, uint8_t *reduce, uint32_t *voiced, uint32_t *unvoiced, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    const size_t n = (size_t)h->n_legs;
    if (reduce && !h->vad) memset(reduce, 4, n);
    if (reduce && h->vad) {
        std::vector<int16_t> r(n);
        const int rc = wmx_vad_export_reduce(h->vad, r.data(), stream);
        if (rc != 0) return rc;
        for (size_t g = 0; g < n; g++) reduce[g] = (uint8_t)r[g];
    }
    return h->gate.export_to({voiced, unvoiced}, wmx::as_stream(stream));
}

// on != 0: every leg's rows of the tick go through the leg's own fixed-point echo canceller (wmx_aecm_process_legs: aec_init(1, 8000, 20)
// per leg, every row one aec_process with delay_ms reported) behind the denoiser and in front of the leveller, and behind the egress the
// datagram the tick sent to the leg, decoded with the law it was encoded in, is the canceller's far row; 0 (the default): the launches
// of a handle that never heard of it.  Between submits.  The canceller and the far rows are made the first time it is switched on, every
// leg at delay_ms; on a made one delay_ms is set for every leg again; off and on again keeps the state.  A delay outside 0 .. 500 changes
// nothing, the switch included; off does not look at it.
int wmx_conf_echo(wmx_conf *h, int on, int delay_ms) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    if (!on) {
        h->echo_on = false;
        return 0;
    }
    if (delay_ms < 0 || delay_ms > 500) {
        wmx::set_error("wmx_conf_echo: delay_ms=%d must be 0 .. 500", delay_ms);
        return WMX_EINVAL;
    }
    if (!h->aecm) {
        void *p = nullptr;
        int rc = wmx::zeroed_block(&p, (size_t)h->n_legs * kLegRow * sizeof(int16_t), "hipMemset(far rows)");
        if (rc != 0) return rc;
        wmx_aecm *a = nullptr;
        if ((rc = wmx_aecm_create_legs(&a, h->n_legs)) != 0) {
            (void)hipFree(p);
            return rc;
        }
        h->aecm = a;
        h->d_echo_far = static_cast<int16_t *>(p);
    }
    const int rc = wmx_aecm_set_delay_legs(h->aecm, nullptr, 0, delay_ms, nullptr);
    if (rc != 0) return rc;
    WMX_HIP(hipStreamSynchronize(nullptr));  // (the setters without a stream are complete when they return)
    h->echo_on = true;
    return 0;
}

// the legs' canceller, for wmx_aecm_set_delay_legs / wmx_aecm_export_stream / wmx_aecm_import_stream on a leg; NULL until echo control is
// first switched on
wmx_aecm *wmx_conf_canceller(wmx_conf *h) { return h ? h->aecm : nullptr; }

// ec_startup, the far ring's fill in ms, knownDelay and the estimator's last_delay (int32 each) of every leg as the work queued on
// `stream` leaves them (wmx_aecm_export_legs); any pointer may be NULL; blocking.  Before the first switch-on: 1, 0, 0, -2 -- what the
// first switch-on makes.
int wmx_conf_export_echo(wmx_conf *h, int32_t *startup, int32_t *far_ms, int32_t *known_delay, int32_t *delay_blocks, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    const size_t n = (size_t)h->n_legs;
    int32_t *host[4] = {startup, far_ms, known_delay, delay_blocks};
    if (!h->aecm) {
        const int32_t fresh[4] = {1, 0, 0, -2};
        for (int i = 0; i < 4; i++)
            for (size_t g = 0; host[i] && g < n; g++) host[i][g] = fresh[i];
        return 0;
    }
    hipStream_t s = wmx::as_stream(stream);
    int32_t *d = nullptr;
    WMX_HIP(hipMalloc(reinterpret_cast<void **>(&d), 4 * n * sizeof(int32_t)));
    int rc = wmx_aecm_export_legs(h->aecm, d, d + n, d + 2 * n, d + 3 * n, stream);
    hipError_t e = hipSuccess;
    for (int i = 0; rc == 0 && e == hipSuccess && i < 4; i++)
        if (host[i]) e = hipMemcpyAsync(host[i], d + (size_t)i * n, n * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d);
    if (rc == 0 && e != hipSuccess) rc = wmx::hip_fail(e, "wmx_conf_export_echo", __FILE__, __LINE__);
    return rc;
}

// a G.711 codec per leg (wmx_rtp_set_codecs over the legs; NULL = all): between submits, ordered on `stream`
int wmx_conf_set_codecs(wmx_conf *h, const int32_t *host_idx, int n, int in_codec, int out_law, void *stream) {
    if (!h) return WMX_EINVAL;
    return wmx_rtp_set_codecs(h->snd, host_idx, n, in_codec, out_law, stream);
}

// in_codec, out_law (uint8) and refused (uint32) of every leg (wmx_rtp_export_codecs); any pointer may be NULL; blocking
int wmx_conf_export_codecs(wmx_conf *h, uint8_t *in_codec, uint8_t *out_law, uint32_t *refused, void *stream) {
    if (!h) return WMX_EINVAL;
    return wmx_rtp_export_codecs(h->snd, in_codec, out_law, refused, stream);
}

// ---- prompts: announcements and hold music per leg (wmix_amd/csrc/leg_prompt.h; the mixer owns the store, as it owns the rings)
// max_clips clips of max_samples samples in all, 1 x 8000 int16, and one state entry per leg: once, between submits, blocking; a
// second call is WMX_ESTATE.  From then on every tick calls wmx_mix_load_prompts behind the load; it launches while a leg can be
// playing.
int wmx_conf_prompts(wmx_conf *h, int max_clips, long max_samples) {
    if (!h) return WMX_EINVAL;
    const int rc = wmx_mix_prompts(h->mix, max_clips, max_samples);
    if (rc == 0) h->prompts_made = true;
    return rc;
}

// one more clip (a blocking copy of host memory) -> its index in *clip; 0 samples, a full table, an arena too small: WMX_EINVAL; no
// store: WMX_ESTATE; nothing is stored then
int wmx_conf_add_clip(wmx_conf *h, const int16_t *host_pcm, long samples, int *clip) {
    if (!h) return WMX_EINVAL;
    return wmx_mix_add_clip(h->mix, host_pcm, samples, clip);
}

// the listed legs (NULL = every leg) start `clip` from its first sample with a fresh cursor: repeat passes (0: until stopped), gap_ticks
// (0 .. 65 535) ticks of pause between two; ordered on `stream`.  A bad leg or clip index changes nothing.
int wmx_conf_play(wmx_conf *h, const int32_t *host_idx, int n, int clip, int repeat, int gap_ticks, void *stream) {
    if (!h) return WMX_EINVAL;
    return wmx_mix_play(h->mix, host_idx, n, clip, repeat, gap_ticks, stream);
}

// the same with the reference's `reduce` (0 .. 15): while the prompt makes calls the rest of the conference reaches the leg divided by
// reduce + 1 (leg_prompt.h, REDUCE)
int wmx_conf_play_duck(wmx_conf *h, const int32_t *host_idx, int n, int clip, int repeat, int gap_ticks, int reduce, void *stream) {
    if (!h) return WMX_EINVAL;
    return wmx_mix_play_duck(h->mix, host_idx, n, clip, repeat, gap_ticks, reduce, stream);
}

// the listed legs (NULL = every leg) go idle; what is in their rings plays out; ordered on `stream`
int wmx_conf_stop(wmx_conf *h, const int32_t *host_idx, int n, void *stream) {
    if (!h) return WMX_EINVAL;
    return wmx_mix_stop(h->mix, host_idx, n, stream);
}

// clip (int32, -1 when idle), the samples consumed of the current pass, the passes left (uint32; 0 while playing: until stopped) and the
// prompts that ran to their end since the leg's reset (uint32) of every leg as the work queued on `stream` leaves them; any pointer may
// be NULL; blocking.  Without a store: -1, 0, 0, 0.
int wmx_conf_export_prompts(wmx_conf *h, int32_t *clip, uint32_t *pos, uint32_t *left, uint32_t *done, void *stream) {
    if (!h) return WMX_EINVAL;
    return wmx_mix_export_prompts(h->mix, clip, pos, left, done, stream);
}

// per leg the divisor the next tick's load applies to what the others add to its ring, 1 for none; blocking
int wmx_conf_export_duck(wmx_conf *h, uint8_t *divisor, void *stream) {
    if (!h) return WMX_EINVAL;
    return wmx_mix_export_duck(h->mix, divisor, stream);
}

int wmx_conf_set_play_correct(wmx_conf *h, uint32_t bytes) { return h ? wmx_mix_set_play_correct(h->mix, bytes) : WMX_EINVAL; }

// a new call in a used slot: fresh cursor, dropped = 0, env = 0, the ring zeroed, seq = timestamp = 0, the sequence rule unsynced,
// refused = 0, the concealment history and count zero, the DTMF state fresh, the noise suppressor as ns_init leaves it, the AGC as
// agc_init leaves it, the gate as vad_init leaves it (`reduce` 4) and its two counters zero, no prompt playing and done = 0; the leg keeps
// its codec and its compression gain
int wmx_conf_reset_legs(wmx_conf *h, const int32_t *host_idx, int n, void *stream) {
    if (!h || (host_idx && n < 0)) return WMX_EINVAL;
    // before the first of them: a bad index resets nothing
    if (wmx::idx_check(host_idx, n, h->n_legs, "wmx_conf_reset_legs: leg", "handle")) return WMX_EINVAL;
    int rc = wmx_mix_reset_leg_cursors(h->mix, host_idx, n, stream);
    if (rc == 0) rc = wmx_mix_reset_speakers(h->mix, host_idx, n, stream);
    if (rc == 0) rc = wmx_mix_reset_rings(h->mix, host_idx, n, stream);
    if (rc == 0) rc = wmx_rtp_reset_streams(h->snd, host_idx, n, stream);
    if (rc == 0) rc = wmx_rtp_reset_sequence(h->snd, host_idx, n, stream);
    if (rc == 0 && h->d_rep) rc = wmx_rtp_reset_conceal(h->snd, host_idx, n, stream);  // never switched on: no state to reset
    if (rc == 0 && h->dtmf_made) rc = wmx_rtp_reset_dtmf(h->snd, host_idx, n, stream);  // a new call inherits no half key press
    if (rc == 0 && h->nsx) rc = conf_reset_stage(h, h->nsx, wmx_nsx_reset_streams, host_idx, n, stream);  // nor the old call's noise estimate
    if (rc == 0 && h->agc) rc = conf_reset_stage(h, h->agc, wmx_agc_reset_streams, host_idx, n, stream);  // nor its level estimate
    if (rc == 0 && h->vad) rc = conf_reset_stage(h, h->vad, wmx_vad_reset_streams, host_idx, n, stream);  // nor its noise model and hangover
    if (rc == 0 && h->vad) rc = h->gate.reset("wmx_conf_reset_legs: leg", host_idx, n, wmx::as_stream(stream));
    if (rc == 0 && h->aecm)  // nor the old call's echo path, far end and start-up; the reported delay stays
        rc = conf_reset_stage(h, h->aecm, +[](wmx_aecm *a, const int32_t *idx, int k, void *st) { return wmx_aecm_reset_streams(a, idx, k, -1, st); },
                              host_idx, n, stream);
    if (rc == 0 && h->prompts_made) rc = wmx_mix_reset_prompts(h->mix, host_idx, n, stream);  // nor the old call's announcement
    if (rc == 0 && h->rec_made) rc = wmx_rtp_reset_record(h->snd, host_idx, n, stream);  // nor its recording: wmix_reset ends the record threads
    return rc;
}

// ---- recording: what a leg hears as PCM (wmix_amd/csrc/leg_record.h; the senders own the store, as they own the DTMF state)
// max_taps taps of one format, chn (1, 2) x freq (1 .. 48 000): once, between submits, blocking; a second call is WMX_ESTATE.  Every slot
// gets two more down buffers: max_taps rows of wmx_conf_rec_row_bytes() and max_taps int32.  From then on a tick in which a tap is
// running calls wmx_rtp_record_rings in front of the egress and downloads the two; every other tick launches and copies what it did.
int wmx_conf_recorders(wmx_conf *h, int max_taps, int chn, int freq) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    int rc = h->ring.wait(-1);  // the ring takes buffers only while it is idle
    if (rc == 0) rc = wmx_rtp_recorders(h->snd, max_taps, chn, freq);
    if (rc != 0) return rc;
    // rows back to back: those of the two formats the kernel moves 16 bytes at a time (320 and 640 bytes) stay on 16-byte boundaries
    const size_t row_bytes = (size_t)wmx_rtp_record_row_bytes(h->snd);
    hipError_t e = h->ring.add({(size_t)max_taps * row_bytes, false, -1});
    if (e == hipSuccess) e = h->ring.add({(size_t)max_taps * sizeof(int32_t), false, -1});
    for (int k = 0; e == hipSuccess && k < h->ring.n(); k++) {  // until a tap has run in a slot, no row of it is valid
        memset(h->ring.host(k, wmx_conf::kRecLegs), 0xFF, (size_t)max_taps * sizeof(int32_t));
        e = hipMemset(h->ring.dev(k, wmx_conf::kRecLegs), 0xFF, (size_t)max_taps * sizeof(int32_t));
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return wmx::hip_fail(e, "wmx_conf_recorders: the slots' rows", __FILE__, __LINE__);
    h->rec_taps = max_taps;
    h->rec_row_bytes = row_bytes;
    h->rec_made = true;
    return 0;
}

// the listed legs each take the lowest free tap (a leg that has one is restarted in place) and record `ticks` rows from the next tick
// on, 0 = until stopped; taps_out (n int32, or NULL) takes the taps.  Too few free taps: WMX_ESTATE, nothing started.
int wmx_conf_record(wmx_conf *h, const int32_t *host_idx, int n, int ticks, int32_t *taps_out, void *stream) {
    if (!h) return WMX_EINVAL;
    return wmx_rtp_record(h->snd, host_idx, n, ticks, taps_out, stream);
}

// the listed legs' taps (NULL = every tap) are free from the next tick on; their written counts stay
int wmx_conf_record_stop(wmx_conf *h, const int32_t *host_idx, int n, void *stream) {
    if (!h) return WMX_EINVAL;
    return wmx_rtp_record_stop(h->snd, host_idx, n, stream);
}

// leg (int32, -1: free), left and written (uint32) of every TAP as the work queued on `stream` leaves them; any pointer may be NULL;
// blocking.  Without a store: WMX_ESTATE.
int wmx_conf_export_record(wmx_conf *h, int32_t *leg, uint32_t *left, uint32_t *written, void *stream) {
    if (!h) return WMX_EINVAL;
    return wmx_rtp_export_record(h->snd, leg, left, written, stream);
}

// the bytes of a row, constant: what wmix_pcm_zoom writes for one package of 320 bytes; 0 without a store
int wmx_conf_rec_row_bytes(const wmx_conf *h) { return h ? (int)h->rec_row_bytes : WMX_EINVAL; }
// valid after wmx_conf_wait(h, slot), like wmx_conf_out: row i is valid exactly when rec_legs[i] >= 0, and is that leg's.  NULL without
// a store.
const int16_t *wmx_conf_rec(wmx_conf *h, int slot) {
    return h && h->rec_made ? static_cast<int16_t *>(h->ring.host(slot, wmx_conf::kRec)) : nullptr;
}
const int32_t *wmx_conf_rec_legs(wmx_conf *h, int slot) {
    return h && h->rec_made ? static_cast<int32_t *>(h->ring.host(slot, wmx_conf::kRecLegs)) : nullptr;
}

// ---- the slots' pinned rows
int wmx_conf_slots(const wmx_conf *h) { return h ? h->ring.n() : WMX_EINVAL; }
int wmx_conf_in_row_bytes(const wmx_conf *h) { return h ? kInRow : WMX_EINVAL; }
uint8_t *wmx_conf_in(wmx_conf *h, int slot) { return h ? static_cast<uint8_t *>(h->ring.host(slot, wmx_conf::kIn)) : nullptr; }
int32_t *wmx_conf_recv(wmx_conf *h, int slot) { return h ? static_cast<int32_t *>(h->ring.host(slot, wmx_conf::kRecv)) : nullptr; }
const uint8_t *wmx_conf_out(wmx_conf *h, int slot) { return h ? static_cast<uint8_t *>(h->ring.host(slot, wmx_conf::kOut)) : nullptr; }
int wmx_conf_next_slot(const wmx_conf *h) { return h ? h->ring.next : WMX_EINVAL; }
wmx_mix *wmx_conf_mix(wmx_conf *h) { return h ? h->mix : nullptr; }
wmx_rtp *wmx_conf_senders(wmx_conf *h) { return h ? h->snd : nullptr; }

// One tick on rows that are on the device already: d_in n_legs x max_packets rows of 176 bytes, d_recv n_legs x max_packets,
// d_out n_legs x 172 bytes.
int wmx_conf_step_resident(wmx_conf *h, const uint8_t *d_in, const int32_t *d_recv, uint8_t *d_out, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h || !d_in || !d_recv || !d_out) {
        wmx::set_error("wmx_conf_step_resident: bad argument");
        return WMX_EINVAL;
    }
    if (wmx_mix_conferences(h->mix) < 1) {
        wmx::set_error("wmx_conf_step_resident: no layout (wmx_conf_set_conferences)");
        return WMX_EINVAL;
    }
    if (h->rec_made && wmx::rtp_record_running(h->snd)) {  // before anything is launched: a recording never silently loses a tick
        wmx::set_error("wmx_conf_step_resident: a recording tap is running and this call has no rows for it (wmx_conf_step_resident_rec)");
        return WMX_ESTATE;
    }
    return conf_launches(h, d_in, d_recv, d_out, nullptr, 0, nullptr, stream);
}

// The resident step with taps: d_rec max_taps rows rec_stride int16 apart (>= wmx_conf_rec_row_bytes() / 2), d_rec_legs max_taps int32,
// both on the device; every tap writes its entry of d_rec_legs, a running one its row.  Without a store: WMX_ESTATE.
int wmx_conf_step_resident_rec(wmx_conf *h, const uint8_t *d_in, const int32_t *d_recv, uint8_t *d_out, int16_t *d_rec, long rec_stride,
                               int32_t *d_rec_legs, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h || !d_in || !d_recv || !d_out || !d_rec || !d_rec_legs) {
        wmx::set_error("wmx_conf_step_resident_rec: bad argument");
        return WMX_EINVAL;
    }
    if (!h->rec_made) {
        wmx::set_error("wmx_conf_step_resident_rec: no store (wmx_conf_recorders)");
        return WMX_ESTATE;
    }
    if (wmx_mix_conferences(h->mix) < 1) {
        wmx::set_error("wmx_conf_step_resident_rec: no layout (wmx_conf_set_conferences)");
        return WMX_EINVAL;
    }
    if (rec_stride < (long)(wmx_rtp_record_row_bytes(h->snd) / 2)) {
        wmx::set_error("wmx_conf_step_resident_rec: rec_stride %ld < the %d samples of a row", rec_stride, wmx_rtp_record_row_bytes(h->snd) / 2);
        return WMX_EINVAL;
    }
    return conf_launches(h, d_in, d_recv, d_out, d_rec, rec_stride, d_rec_legs, stream);
}

// Queue the next slot: its in / recv rows must hold this tick's arrivals.  Blocks only if that slot is still in flight from `slots`
// submits ago.  A failure before the first launch has advanced nothing; a later one has lost the tick (the cursors that moved stay
// moved, as a receive thread's do), and in both cases the rotation and the slots in flight are as before and the streams are drained.
int wmx_conf_submit(wmx_conf *h, int *slot, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    if (wmx_mix_conferences(h->mix) < 1) {
        wmx::set_error("wmx_conf_submit: no layout (wmx_conf_set_conferences)");
        return WMX_EINVAL;
    }
    wmx::SlotRing &ring = h->ring;
    const int k = ring.next;
    hipStream_t main = wmx::as_stream(stream);
    int rc = ring.retire(k);  // only completes what an earlier submit promised
    if (rc == 0) rc = ring.upload(k, main);
    if (rc != 0) return rc;
    // The taps: launched, and their two buffers downloaded, only in a tick in which one is running -- the host knows from its copy of
    // leg_record.h's state.  In every other tick the slot's legs say -1 from here: a host write of max_taps words, no copy.
    const bool rec = h->rec_made && wmx::rtp_record_running(h->snd);
    if (h->rec_made && !rec) memset(ring.host(k, wmx_conf::kRecLegs), 0xFF, (size_t)h->rec_taps * sizeof(int32_t));
    rc = conf_launches(h, static_cast<uint8_t *>(ring.dev(k, wmx_conf::kIn)), static_cast<int32_t *>(ring.dev(k, wmx_conf::kRecv)),
                       static_cast<uint8_t *>(ring.dev(k, wmx_conf::kOut)), rec ? static_cast<int16_t *>(ring.dev(k, wmx_conf::kRec)) : nullptr,
                       (long)(h->rec_row_bytes / sizeof(int16_t)), rec ? static_cast<int32_t *>(ring.dev(k, wmx_conf::kRecLegs)) : nullptr, stream);
    if (rc == 0) rc = ring.done(k, main);
    // a few KB: at once, behind the tick's own last launch
    if (rc == 0) rc = ring.download(k, nullptr, rec ? ~0u : ~(1u << wmx_conf::kRec | 1u << wmx_conf::kRecLegs));
    if (rc != 0) {
        char why[512];
        snprintf(why, sizeof(why), "%s", wmx_last_error());
        ring.drain(main, true);
        wmx::set_error("wmx_conf_submit: the tick is lost (%s)", why);
        return rc;
    }
    ring.commit(k, false);
    if (slot) *slot = k;
    return 0;
}

// Blocks until the slot's datagrams are in its out rows (at once for a slot that is not in flight); slot < 0: every slot.
int wmx_conf_wait(wmx_conf *h, int slot) {
    WMX_ON_DEVICE(h);
    return h ? h->ring.wait(slot) : WMX_EINVAL;
}

// Non-blocking wmx_conf_wait: 1 = the rows of `slot` (< 0: of every slot) are in host memory, 0 = still on their way.
int wmx_conf_poll(wmx_conf *h, int slot) {
    WMX_ON_DEVICE(h);
    return h ? h->ring.poll(slot) : WMX_EINVAL;
}

// the sequence rule's state of every leg (wmx_rtp_export_sequence); any pointer may be NULL; blocking
int wmx_conf_export_sequence(wmx_conf *h, uint16_t *next, uint8_t *synced, uint32_t *lost, uint32_t *late, uint32_t *dup, uint32_t *resync,
                             uint32_t *overflow, void *stream) {
    if (!h) return WMX_EINVAL;
    return wmx_rtp_export_sequence(h->snd, next, synced, lost, late, dup, resync, overflow, stream);
}

// head, tick, dropped (uint32), env (uint32) and speaking (uint8) of every leg as the work queued on `stream` leaves them; any pointer
// may be NULL; blocking
int wmx_conf_export_legs(wmx_conf *h, uint32_t *head, uint32_t *tick, uint32_t *dropped, uint32_t *env, uint8_t *speaking, void *stream) {
    if (!h) return WMX_EINVAL;
    int rc = 0;
    if (head || tick || dropped) rc = wmx_mix_export_leg_cursors(h->mix, head, tick, dropped, stream);
    if (rc == 0 && (env || speaking)) rc = wmx_mix_export_speakers(h->mix, env, speaking, stream);
    return rc;
}

}  // extern "C"
