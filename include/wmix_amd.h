/* wmix_amd.h -- C ABI of libwmix_amd.so: the MI355X (gfx950) implementation of
 * wmix's per-frame DSP hot path.
 *
 * Two layers are exported:
 *
 *  (1) the REFERENCE'S OWN signatures, unchanged, so the wmix daemon links
 *      against libwmix_amd.so instead of src/webrtc.c + libwebrtc{vad,aec,ns,agc}
 *      + src/g711codec.c (+ the two arithmetic functions of src/wmix.c).  They take
 *      HOST pointers exactly like the reference and are thin adapters over a
 *      batch of one stream (H2D copy, one launch, D2H copy).  Declared in
 *      include/wmix_compat.h.
 *
 *  (2) the BATCHED entry points below (prefix wmx_): many independent 10 ms
 *      streams per launch, PCM and state resident in HBM.  Plain pointers and
 *      sizes only; `stream` is a hipStream_t passed as void* (NULL = default
 *      stream).  All d_* pointers are DEVICE pointers.  Every function returns 0
 *      on success, a negative value on failure (WMX_EHIP_BASE - hipError_t for HIP
 *      errors, WMX_E* otherwise); wmx_last_error() describes the last failure on the
 *      calling thread.  There is NO CPU fallback: without a usable HIP device the
 *      calls fail.
 */
#ifndef WMIX_AMD_H
#define WMIX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WMX_EINVAL (-10001) /* bad argument (unsupported freq / chn / size) */
#define WMX_ENODEV (-10002) /* no HIP device */
#define WMX_ESTATE (-10003) /* wrong handle kind */
/* A failing HIP runtime call returns WMX_EHIP_BASE - (int)hipError_t (hipErrorOutOfMemory = 2 -> -11002): outside the
 * reference's own return values (0 / -1), which some entry points hand through (wmx_aec_run: -1 = the wrapper stopped
 * at a delay outside [0, 500]). */
#define WMX_EHIP_BASE (-11000)
#define WMX_IS_HIP_ERROR(rc) ((rc) <= WMX_EHIP_BASE && (rc) > WMX_EHIP_BASE - 10000)

const char *wmx_last_error(void);
int wmx_device_count(void);
/* Device affinity: every wmx_* handle records the HIP device that is current on the creating thread and every entry
 * point that takes the handle runs on that device (and restores the caller's), so a host with one thread per GPU needs
 * no thread-local hipSetDevice discipline.  Device pointers passed to a call must live on
 * the handle's device.  Works for any wmx_* handle type; WMX_EINVAL for NULL. */
int wmx_handle_device(const void *handle);
/* library/ABI version: major*10000 + minor*100 + patch */
int wmx_version(void);
/* "default" for the product build; else the developer flags the library was built with (prefixed "TIMING-ONLY (wrong results): "
 * when one of them is a timing experiment's switch).  The Python mirror, build(), smoke() and bench.py refuse anything but "default"
 * unless WMIX_AMD_ALLOW_VARIANT_BUILD=1. */
const char *wmx_build_info(void);

/* ------------------------------------------------------------------ per-stream lifetime inside a batch
 * The reference creates each handle lazily in the record heartbeat and releases it when its switch drops or recording
 * idles (src/wmix.c:565-600, 617-618, 635-636, 683-684, 702-703, 783-813; *_init / *_release in src/webrtc.c:40-82,
 * 153-164, 217-274, 485-505, 560-602, 646-661, 694-753, 841-860): the streams of a batch join, leave and restart on their
 * own.  Every stateful module therefore has
 *   wmx_<m>_reset_streams(h, idx, n, stream)  <m>_release + <m>_init for the n streams listed in the HOST array idx (a
 *                                             refill kernel ordered on `stream` like the process calls around it);
 *   wmx_<m>_set_active(h, mask, stream)       mask: HOST array of n_streams bytes; 0 = the stream is not called -- state
 *                                             and PCM rows untouched, like a handle nobody calls; NULL = all active.  The
 *                                             mask stays in force until the next set_active.
 * The AEC / AECM, whose control plane is shared by the streams that were started together, add COHORTS, see there.
 * Bad index -> WMX_EINVAL, nothing reset. */

/* Stream migration between batches / GPUs (a stream that outlives its batch, or that moves to another device for balance):
 *   wmx_<m>_stream_state_bytes(h)            size of one stream's state blob for this handle's format
 *   wmx_<m>_export_stream(h, i, blob)        the complete state of stream i into HOST memory (blocking: the device is drained)
 *   wmx_<m>_import_stream(h, i, blob[, c])   the reverse, into any handle of the same module and format (WMX_ESTATE otherwise);
 *                                            for the AEC / AECM `c` >= 0 also makes the stream a member of cohort c
 *   wmx_{aec,aecm}_cohort_state_bytes / _export_cohort / _import_cohort   the shared part: control plane + far-end history
 * A stream imported together with its cohort continues bit for bit as if it had never moved (tests/test_lifetime_gpu.py). */

/* ------------------------------------------------------------------ G.711
 * Replaces g711{a,u}_encode / g711{a,u}_decode (src/g711codec.h:30-34,
 * src/g711codec.c:82-216) for device-resident buffers.  law: 0 = A-law, 1 = mu-law.
 * Bit-exact with the reference including its 16-bit-domain segment table and the
 * negative A-law path. */
#define WMX_LAW_A 0
#define WMX_LAW_U 1
int wmx_g711_encode(int law, const int16_t *d_pcm, uint8_t *d_code, size_t n_samples, void *stream);
int wmx_g711_decode(int law, const uint8_t *d_code, int16_t *d_pcm, size_t n_codes, void *stream);

/* ------------------------------------------------------------------ NS (float noise suppressor)
 * Batched form of ns_init / ns_process / ns_release (src/webrtc.h:47-51, src/webrtc.c:560-661):
 * n_streams independent streams, each with the state WebRtcNs_Create/Init/set_policy(2) would
 * give it.  freq in {8000,16000,32000}, chn in {1,2}; anything else -> WMX_EINVAL (ns_init
 * returns NULL there; 24000 passes the wrapper's `freq % 8000` test but WebRtcNs_Init refuses it, and for VAD / AGC
 * the reference then hands out a handle whose every process call fails -- here creation fails for all four).  A packet is 10 ms = freq/100 frames of chn interleaved int16.
 *
 * wmx_ns_process runs n_packets consecutive packets of every stream in one launch.  Packet p of
 * stream s starts at d_in + s*stream_stride + p*packet_stride (strides in int16 elements), same
 * for d_out; d_out may alias d_in (the daemon always processes in place).  Reference quirks are
 * kept: the right channel of a 2-channel stream is treated as a high band, and at 32 kHz only the
 * first 160 frames of each packet are processed, the rest of the output packet is zero
 * (SURVEY.md section 0 quirks 2-3).
 *
 * Every spectral / time sum is added in the reference's index order: bit-exact with the CPU path.  (The faster re-associated mode of
 * rounds 1-5, wmx_ns_set_ordered(h, 0), was outside north_star's +-1 LSB -- up to 13 LSB on a few samples -- and is gone.) */
typedef struct wmx_ns wmx_ns;
int wmx_ns_create(wmx_ns **out, int n_streams, int chn, int freq);
int wmx_ns_destroy(wmx_ns *h);
int wmx_ns_packet_samples(const wmx_ns *h); /* int16 elements per packet = freq/100*chn */
int wmx_ns_process(wmx_ns *h, const int16_t *d_in, int16_t *d_out, int n_packets, long stream_stride,
                   long packet_stride, void *stream);
/* debugging / tests: copy one stream's state block (layout: wmix_amd/csrc/ns_layout.h) and its
 * 3 x 1000 histogram counters to host memory (either pointer may be NULL). */
int wmx_ns_state_words(const wmx_ns *h);
int wmx_ns_export_state(const wmx_ns *h, int stream_index, float *host_words, unsigned short *host_hist);
int wmx_ns_reset_streams(wmx_ns *h, const int32_t *idx, int n, void *stream);
int wmx_ns_set_active(wmx_ns *h, const uint8_t *host_mask, void *stream);
int wmx_ns_stream_state_bytes(const wmx_ns *h);
int wmx_ns_export_stream(wmx_ns *h, int stream_index, void *host_blob);
int wmx_ns_import_stream(wmx_ns *h, int stream_index, const void *host_blob);

/* ------------------------------------------------------------------ NSX (fixed-point noise suppressor)
 * Batched form of the SAME three wrapper functions when the reference is built with its MAKE_WEBRTC_NSX switch
 * (src/webrtc.c:512-521: ns_init / ns_process / ns_release over WebRtcNsx_Create / Init / set_policy(2) / Process,
 * W:modules/audio_processing/ns/nsx_core.c).  Same packet rule, strides, aliasing and quirks as wmx_ns_* (right channel =
 * high band, second half of a 32 kHz packet zero).  Integer path: bit-exact.  The legacy ns_init picks this
 * implementation when the environment has WMIX_AMD_NSX=1 (the build-time macro of the reference becomes a run-time
 * switch). */
typedef struct wmx_nsx wmx_nsx;
int wmx_nsx_create(wmx_nsx **out, int n_streams, int chn, int freq);
int wmx_nsx_destroy(wmx_nsx *h);
int wmx_nsx_packet_samples(const wmx_nsx *h);
int wmx_nsx_state_bytes(const wmx_nsx *h); /* per-stream state block in HBM (the 3 x 1000 int16 histograms come on top) */
int wmx_nsx_process(wmx_nsx *h, const int16_t *d_in, int16_t *d_out, int n_packets, long stream_stride,
                    long packet_stride, void *stream);
int wmx_nsx_reset_streams(wmx_nsx *h, const int32_t *idx, int n, void *stream);
int wmx_nsx_set_active(wmx_nsx *h, const uint8_t *host_mask, void *stream);
int wmx_nsx_stream_state_bytes(const wmx_nsx *h);
int wmx_nsx_export_stream(wmx_nsx *h, int stream_index, void *host_blob);
int wmx_nsx_import_stream(wmx_nsx *h, int stream_index, const void *host_blob);
/* The ragged form for the legs of a conference bridge, on a handle created with chn == 1, freq == 8000: stream g is leg g, and a tick
 * brings it 0 .. max_packets (1 .. WMX_MIX_MAX_LEG_PACKETS) rows of 160 samples (20 ms), slot k at d_pcm + g * leg_stride +
 * k * packet_stride (strides in samples), with d_len[g * max_packets + k] == 320 where the slot holds a row.  The leg's rows are taken
 * in the order the load makes its calls (wmix_amd/csrc/leg_dtmf.h): d_calls NULL, the slots with d_len == 320 in slot order; else
 * d_calls[g] is the leg's call list (WMX_RTP_CALLS_*, what wmx_rtp_sequence_legs leaves), walked in list order, where a silence call
 * or a data call naming a row that is not readable feeds NOTHING -- a lost packet is not 20 ms of zeros to the noise estimator.  Each
 * row taken is two 80-sample blocks of the suppressor, processed in place; the bits are those of wmx_nsx_process over the same rows in
 * the same order.  A leg with no row this tick touches nothing: its state is neither loaded nor stored.  A row that is not taken --
 * a late packet, a duplicate, a refused packet -- keeps its bytes.  wmx_nsx_set_active's mask holds here too.
 * ALIGNMENT: d_pcm on a 2-byte boundary (the rows are read and written sample by sample as int16; the strides count samples, so
 * every row then is).  Nothing wider is needed.
 * WMX_EINVAL, nothing launched: a handle that is not 1 x 8000; max_packets outside 1 .. 4; d_pcm or d_len NULL; rows that overlap
 * (packet_stride < 160, or with more than one leg leg_stride < max_packets * packet_stride); d_pcm on an odd address. */
int wmx_nsx_process_legs(wmx_nsx *h, int16_t *d_pcm, long leg_stride, long packet_stride, int max_packets, const uint32_t *d_len,
                         const uint32_t *d_calls, void *stream);

/* ------------------------------------------------------------------ VAD (voice-activity gate)
 * Batched form of vad_init / vad_process / vad_release (src/webrtc.h:32-36, src/webrtc.c:40-164):
 * WebRtcVad mode 3 decides speech/no-speech per packet; a per-stream `reduce` in [0,4] moves one
 * step per decision and the packet is shifted right by it, in place.  Packet = intervalMs worth of
 * frames (20 ms only when freq <= 16000 and interval_ms % 20 == 0, else 10 ms).
 *
 * One "call" = one vad_process() invocation covering packets_per_call packets; the reference
 * analyses and attenuates only packet 0 of a call and so do we.  Call c of
 * stream s starts at d_pcm + s*stream_stride + c*call_stride (int16 elements).  Integer path:
 * bit-exact. */
typedef struct wmx_vad wmx_vad;
int wmx_vad_create(wmx_vad **out, int n_streams, int chn, int freq, int interval_ms);
int wmx_vad_destroy(wmx_vad *h);
int wmx_vad_packet_samples(const wmx_vad *h); /* int16 elements per packet = freq/1000*intervalMs*chn */
int wmx_vad_process(wmx_vad *h, int16_t *d_pcm, int packets_per_call, int n_calls, long stream_stride,
                    long call_stride, void *stream);
int wmx_vad_reset_streams(wmx_vad *h, const int32_t *idx, int n, void *stream);
int wmx_vad_set_active(wmx_vad *h, const uint8_t *host_mask, void *stream);
int wmx_vad_stream_state_bytes(const wmx_vad *h);
int wmx_vad_export_stream(wmx_vad *h, int stream_index, void *host_blob);
int wmx_vad_import_stream(wmx_vad *h, int stream_index, const void *host_blob);
/* The ragged form for the legs of a conference bridge, on a handle created with chn == 1, freq == 8000 and an interval_ms that is a
 * multiple of 20 (a packet of 160 samples, exactly one row): stream g is leg g, and a tick brings it 0 .. max_packets
 * (1 .. WMX_MIX_MAX_LEG_PACKETS) rows of 160 samples (20 ms), slot k at d_pcm + g * leg_stride + k * packet_stride (strides in
 * samples), with d_len[g * max_packets + k] == 320 where the slot holds a row.  Arguments, order and refusals are those of
 * wmx_nsx_process_legs and wmx_agc_process_legs: the leg's rows are taken in the order the load makes its calls
 * (wmix_amd/csrc/leg_calls.h): d_calls NULL, the slots with d_len == 320 in slot order; else d_calls[g] is the leg's call list
 * (WMX_RTP_CALLS_*, what wmx_rtp_sequence_legs leaves), walked in list order, where a silence call or a data call naming a row that is
 * not readable feeds NOTHING -- a lost packet is not 20 ms of zeros to the noise model.  Each row taken is one vad_process of the
 * reference on one 160-sample packet, in place: the decision, one step of the leg's `reduce` (0 .. 4; a fresh stream starts at 4, so
 * a new call is attenuated in its first rows and heard in full from its fifth), the row shifted right by it.  The bits are those of
 * wmx_vad_process(h, rows, 1, n, ...) over the same rows in the same order.  A leg with no row this tick touches nothing: its state is
 * neither loaded nor stored.  A row that is not taken -- a late packet, a duplicate, a refused packet -- keeps its bytes and is never
 * addressed.  wmx_vad_set_active's mask holds here too.
 * d_voice: NULL, or 2 * n_streams words on the device, owned by the caller (who zeroes them): word g is incremented per row taken of
 * leg g whose decision, after hangover, is voice, word n_streams + g per row taken whose decision is not.
 * ALIGNMENT: d_pcm on a 2-byte boundary is all that is required.  When d_pcm is on a 16-byte boundary and both strides are multiples
 * of 8 samples a row travels as 16-byte words through registers; otherwise it is read and written sample by sample.  Same bits.
 * WMX_EINVAL, nothing launched: a handle whose packet is not 160 samples of 1 x 8000; max_packets outside 1 .. 4; d_pcm or d_len NULL;
 * rows that overlap (packet_stride < 160, or with more than one leg leg_stride < max_packets * packet_stride); d_pcm on an odd address.
 * wmx_vad_export_reduce: `reduce` of every stream (int16, n_streams of them) as the work queued on `stream` leaves it; blocking. */
int wmx_vad_process_legs(wmx_vad *h, int16_t *d_pcm, long leg_stride, long packet_stride, int max_packets, const uint32_t *d_len,
                         const uint32_t *d_calls, uint32_t *d_voice, void *stream);
int wmx_vad_export_reduce(wmx_vad *h, int16_t *host_reduce, void *stream);

/* ------------------------------------------------------------------ AGC (legacy fixed-point, adaptive digital)
 * Batched form of agc_init / agc_process / agc_addition / agc_release (src/webrtc.h:55-60,
 * src/webrtc.c:694-860): target 0 dBFS, compression gain `value` dB, limiter off.  Channels are
 * averaged to mono, processed as one band and duplicated back.  Packet = 10 ms (5 ms at 32 kHz,
 * SURVEY.md section 0 quirk 4).  `value` outside the reference's gain-table range makes create/set_gain
 * fail with WMX_EINVAL (agc_init returns NULL there).  Integer path: bit-exact.
 *
 * The compression gain is PER STREAM, as it is per handle in the reference (agc_init's `value`, agc_addition(fp, value);
 * the daemon: src/wmix.c:684, 1068-1070): wmx_agc_create / wmx_agc_set_gain give every stream of the batch one value;
 * wmx_agc_set_gain_streams is agc_addition for the listed streams (state untouched, new gain curve from the next packet on),
 * wmx_agc_reset_streams_gain is agc_release + agc_init(.., value, ..) for them; wmx_agc_reset_streams re-creates a stream
 * with the gain it has.  One 32-entry table per distinct value in use; a batch whose streams all share one value runs
 * the same kernels as before.  The value travels with wmx_agc_export_stream / _import_stream. */
typedef struct wmx_agc wmx_agc;
int wmx_agc_create(wmx_agc **out, int n_streams, int chn, int freq, int interval_ms, int value);
int wmx_agc_destroy(wmx_agc *h);
int wmx_agc_set_gain(wmx_agc *h, int value); /* agc_addition for every stream of the batch (blocking) */
/* idx: HOST array of n stream indices; ordered on `stream` like the process calls around it.  A value the reference's
 * WebRtcAgc_set_config refuses -> WMX_EINVAL, nothing changed. */
int wmx_agc_set_gain_streams(wmx_agc *h, const int32_t *idx, int n, int value, void *stream);
int wmx_agc_reset_streams_gain(wmx_agc *h, const int32_t *idx, int n, int value, void *stream);
int wmx_agc_stream_gain(const wmx_agc *h, int stream_index); /* the compression gain stream i runs with */
int wmx_agc_packet_samples(const wmx_agc *h);
int wmx_agc_gain_table(const wmx_agc *h, int32_t *host_table32); /* the 32 Q16 gains of the batch's own value (tests) */
int wmx_agc_process(wmx_agc *h, const int16_t *d_in, int16_t *d_out, int n_packets, long stream_stride,
                    long packet_stride, void *stream);
int wmx_agc_reset_streams(wmx_agc *h, const int32_t *idx, int n, void *stream); /* each stream keeps its gain */
int wmx_agc_set_active(wmx_agc *h, const uint8_t *host_mask, void *stream);
int wmx_agc_stream_state_bytes(const wmx_agc *h);
int wmx_agc_export_stream(wmx_agc *h, int stream_index, void *host_blob);
int wmx_agc_import_stream(wmx_agc *h, int stream_index, const void *host_blob);
/* The ragged form for the legs of a conference bridge, on a handle created with chn == 1, freq == 8000: stream g is leg g, and a tick
 * brings it 0 .. max_packets (1 .. WMX_MIX_MAX_LEG_PACKETS) rows of 160 samples (20 ms), slot k at d_pcm + g * leg_stride +
 * k * packet_stride (strides in samples), with d_len[g * max_packets + k] == 320 where the slot holds a row.  Arguments, order and
 * refusals are those of wmx_nsx_process_legs: the leg's rows are taken in the order the load makes its calls
 * (wmix_amd/csrc/leg_calls.h): d_calls NULL, the slots with d_len == 320 in slot order; else d_calls[g] is the leg's call list
 * (WMX_RTP_CALLS_*, what wmx_rtp_sequence_legs leaves), walked in list order, where a silence call or a data call naming a row that is
 * not readable feeds NOTHING -- a lost packet is not 20 ms of silence to the level detector.  Each row taken is two 80-sample packets
 * of the AGC, processed in place with the leg's own compression gain; the bits are those of wmx_agc_process over the same rows in the
 * same order, which are one agc_process of the reference per leg.  A leg with no row this tick touches nothing: its state is neither
 * loaded nor stored.  A row that is not taken -- a late packet, a duplicate, a refused packet -- keeps its bytes.  wmx_agc_set_active's
 * mask holds here too.
 * ALIGNMENT: d_pcm on a 2-byte boundary (the rows are read and written sample by sample as int16; the strides count samples, so
 * every row then is).  Nothing wider is needed.
 * WMX_EINVAL, nothing launched: a handle that is not 1 x 8000; max_packets outside 1 .. 4; d_pcm or d_len NULL; rows that overlap
 * (packet_stride < 160, or with more than one leg leg_stride < max_packets * packet_stride); d_pcm on an odd address. */
int wmx_agc_process_legs(wmx_agc *h, int16_t *d_pcm, long leg_stride, long packet_stride, int max_packets, const uint32_t *d_len,
                         const uint32_t *d_calls, void *stream);

/* ------------------------------------------------------------------ AEC (float echo canceller)
 * Batched form of aec_init / aec_setFrameFar / aec_process / aec_process2 / aec_release
 * (src/webrtc.h:40-45, src/webrtc.c:217-505): n_streams near-end streams cancelled against ONE
 * shared far-end reference (BASELINE.json configs[2..3]; a batch of one stream is the reference's
 * per-handle case).  freq in {8000,16000}; packet = 10 ms (20 ms only at 8000 Hz with
 * interval_ms % 20 == 0).  Only channel 0 of far and near is used; the output is duplicated to
 * every channel.
 *
 * wmx_aec_run processes n_packets consecutive packets: mode bit 1 buffers the far-end packet
 * (aec_setFrameFar), bit 2 processes the near-end packet (aec_process), 3 does both in the
 * reference's order (aec_process2).  d_far is the shared far-end (packet p at
 * d_far + p*far_packet_stride); near/out packet p of stream s at s*stream_stride + p*packet_stride;
 * d_out may alias d_near.  delay_ms is the reported sound-card delay (the daemon passes 0).
 * Returns 0, a WMX_E* error, or -1 where the reference wrapper would return non-zero (delay outside
 * [0,500]: the offending packet HAS been processed with the delay clamped, as WebRtcAec_Process does,
 * so the state has moved on; its output is left unwritten and nothing after it runs).
 * Float path: same operation order as the reference and the same powf (glibc's algorithm, restated
 * in csrc/libm_dev.h); tests require bit-exactness. */
typedef struct wmx_aec wmx_aec;
int wmx_aec_create(wmx_aec **out, int n_streams, int chn, int freq, int interval_ms);
int wmx_aec_destroy(wmx_aec *h);
int wmx_aec_packet_samples(const wmx_aec *h);
int wmx_aec_run(wmx_aec *h, int mode, const int16_t *d_far, long far_packet_stride, const int16_t *d_near,
                int16_t *d_out, int n_packets, long stream_stride, long packet_stride, int delay_ms, void *stream);
/* Far-end groups: the reference handle owns its far-end (aec_process2(fp, far, near, ...), src/webrtc.c:410), so a batch
 * need not share one.  n_far far-ends per batch; host array stream_far[n_streams] gives each stream's far-end in
 * [0, n_far).  All far-ends are driven in lockstep (same packet count and reported delay per call).  wmx_aec_run_groups
 * takes far-end g's packet p at d_far + g*far_group_stride + p*far_packet_stride.  wmx_aec_create / wmx_aec_run are the
 * n_far = 1 forms.  Cost: one far-end wave per group in front of the near kernel; configs with one far-end run unchanged. */
int wmx_aec_create_groups(wmx_aec **out, int n_streams, int chn, int freq, int interval_ms, int n_far, const int32_t *stream_far);
int wmx_aec_run_groups(wmx_aec *h, int mode, const int16_t *d_far, long far_packet_stride, long far_group_stride,
                       const int16_t *d_near, int16_t *d_out, int n_packets, long stream_stride, long packet_stride,
                       int delay_ms, void *stream);
int wmx_aec_state_words(const wmx_aec *h);
int wmx_aec_export_state(const wmx_aec *h, int stream_index, float *host_words);
/* Cohorts.  Everything in the AEC that decides WHERE data goes (ProcessNormal's start-up machine and delay filter, the ring
 * positions, the block counters, W:echo_cancellation.c:599-872, aec_core.c:1719-1850) depends on when the handle was
 * created and on the delays it was called with, never on the audio -- and so does the blocking of the far-end (64-sample
 * blocks counted from the handle's first packet).  Streams that were started at the same packet and report the same delay
 * form a COHORT: one control plane on the host, one far-end history on the device.  A far-end group of
 * wmx_aec_create_groups IS a cohort (stream_far may be NULL there: every stream starts in cohort 0).  A stream joins by
 *     wmx_aec_reset_cohort(h, c, stream)               -- once per cohort and join time: aec_init of the shared part
 *     wmx_aec_reset_streams(h, idx, n, c, stream)      -- aec_release + aec_init of the streams, now members of c (c = -1:
 *                                                         membership unchanged, e.g. one cohort and every stream restarted)
 * and leaves through the active mask.  wmx_aec_run_cohorts is wmx_aec_run_groups with a reported delay PER COHORT
 * (aec_process2's delayms is per handle, src/webrtc.c:410), an optional on/off byte per cohort (0: not called, control plane
 * and far history stand still) and an optional per-cohort return code (what aec_process2 would have returned to its
 * members; a rejected cohort runs nothing after the offending packet, the others carry on).  All arrays are HOST arrays of
 * wmx_aec_cohorts(h) entries.  Returns 0, WMX_E*, or the first non-zero cohort code. */
int wmx_aec_cohorts(const wmx_aec *h);
int wmx_aec_reset_cohort(wmx_aec *h, int cohort, void *stream);
/* Cohorts come and go with the handles they stand for (the reference makes a handle inside the heartbeat on first use and
 * releases it when its switch drops or recording idles, src/wmix.c:565-600, 635-636): wmx_aec_add_cohort starts a NEW one --
 * aec_init of the shared part at this point of the packet sequence; a retired id when there is one, else the next, with the
 * device buffers growing by doubling -- and returns its id in *cohort; wmx_aec_retire_cohort says that every member was
 * released: the cohort is never called again and its id may be handed out again.  wmx_aec_cohorts(h) = ids in use, retired
 * ones included = the length of the per-cohort arrays.  Per launch only packets x cohorts plans of 224 bytes cross PCIe (the
 * comfort noise's phases are not in them: they lie in a device table indexed by the stream's own block count). */
int wmx_aec_add_cohort(wmx_aec *h, int *cohort, void *stream);
int wmx_aec_retire_cohort(wmx_aec *h, int cohort);
/* Coalescing.  Handles of the reference that were created at different times but are called with the same delay end up with
 * control planes that differ only in WHERE their rings stand (W: echo_cancellation.c:599-872 and aec_core.c:1719-1850 are index
 * arithmetic on fill levels): from then on they compute the same far-end spectra, far power and plans, once per handle.  This
 * call merges such cohorts: (1) it completes the merges whose check -- launched by an earlier call -- came back equal: the far-end
 * slabs of the two cohorts were compared on the device, word for word under the rotation between their ring positions (that
 * includes the running far power, an IIR from each handle's own start); the members of `from` then get their re-blocking rings
 * rotated to the positions of `into`, its id, and `from` is retired; every stream keeps the comfort-noise generator it would have
 * as its own handle (its state is the stream's block count, part of the stream's state).  The pairs are reported in
 * merged_from[] / merged_into[] (*n_merged of them, at most cap) so that the caller can redirect its own tables; the id range
 * wmx_aec_cohorts(h) shrinks behind the last live cohort.  (2) it proposes up to max_pairs (<= 32) new pairs -- equal fill
 * levels and delay filter, start-up over, lowest id leads -- and launches their comparison behind the work already in
 * `stream`.  Nothing waits for the device: a pair proposed by one call is merged by a later one.  A pair is dropped when its two
 * cohorts are not called identically in between (delay, cohort_on, private far-end packets).  max_pairs = 0: only (1).
 * Merged streams are bound to one reported delay from then on, like the members of any cohort. */
/* cohorts of the id range that are not retired (what a launch really computes far-end spectra and plans for) */
int wmx_aec_live_cohorts(const wmx_aec *h);
int wmx_aec_coalesce(wmx_aec *h, int max_pairs, int32_t *merged_from, int32_t *merged_into, int cap, int *n_merged, void *stream);
int wmx_aec_reset_streams(wmx_aec *h, const int32_t *idx, int n, int cohort, void *stream);
int wmx_aec_set_active(wmx_aec *h, const uint8_t *host_mask, void *stream);
int wmx_aec_stream_state_bytes(const wmx_aec *h);
int wmx_aec_export_stream(wmx_aec *h, int stream_index, void *host_blob);
int wmx_aec_import_stream(wmx_aec *h, int stream_index, const void *host_blob, int cohort);
int wmx_aec_cohort_state_bytes(const wmx_aec *h);
int wmx_aec_export_cohort(wmx_aec *h, int cohort, void *host_blob);
int wmx_aec_import_cohort(wmx_aec *h, int cohort, const void *host_blob);
int wmx_aec_run_cohorts(wmx_aec *h, int mode, const int16_t *d_far, long far_packet_stride, long far_group_stride,
                        const int16_t *d_near, int16_t *d_out, int n_packets, long stream_stride, long packet_stride,
                        const int32_t *delay_ms, const uint8_t *cohort_on, int32_t *cohort_rc, void *stream);
/* In-stream timing of the two AEC kernels (bench.py's roofline entry): with timing on, every near-end launch is bracketed
 * by HIP events recorded on the launch stream -- before the far kernel, between the two, after the near kernel.
 * wmx_aec_timing waits for the last one, returns the number of launches and the summed durations (ms) since the previous
 * call and starts over. */
int wmx_aec_set_timing(wmx_aec *h, int on);
int wmx_aec_timing(wmx_aec *h, int *n_launches, double *far_ms, double *near_ms);
/* Host side of the same launches: their number and the seconds the per-cohort control planes (index arithmetic, W:
 * echo_cancellation.c:599-872 per cohort and packet) took on the caller's thread since the previous call. */
int wmx_aec_host_ctl(wmx_aec *h, long *n_launches, double *seconds);

/* ------------------------------------------------------------------ the record heartbeat: NS -> AEC -> AGC -> VAD in one call
 * wmix_shmem_write_circle (src/wmix.c:613-709) runs, per WMIX_INTERVAL_MS of captured audio and on one buffer in place,
 * ns_process -> aec_process2(far, near = out = buffer, delayms) -> agc_process -> vad_process, each behind its
 * webrtcEnable[] switch.  wmx_chain is that heartbeat for a batch: `stages` = the switches, one wmx_chain_process per tick
 * launches the enabled stages back to back on `stream` (no host synchronisation, nothing copied).
 * n10 = 10 ms packets per stream in the tick (the daemon's 20 ms tick is 2); packet p of stream s lies at
 * s*stream_stride + p*packet_stride in d_in / d_out (int16 elements; d_out == d_in is the daemon's case), the shared
 * far-end's 10 ms packet p at d_far + p*far_packet_stride.  vad_process is ONE call per tick, as in the heartbeat.  Stages
 * whose own packet is 20 ms (AEC at 8 kHz / VAD, when interval_ms % 20 == 0) need the tick contiguous (packet_stride == one
 * 10 ms packet).  delay_ms / cohort_on / cohort_rc: HOST arrays of n_cohorts entries as in wmx_aec_run_cohorts (NULL: delay 0 as
 * the daemon passes it, every cohort on, no codes wanted).  Returns 0, WMX_E*, or -1 when a cohort's delay was rejected.
 * The lifetime calls forward to every stage; the stage handles themselves are reachable for everything else. */
#define WMX_CHAIN_NS 1u
#define WMX_CHAIN_AEC 2u
#define WMX_CHAIN_AGC 4u
#define WMX_CHAIN_VAD 8u
/* The reference's two build-time alternates of the same stages (src/webrtc.c:512-521: -DMAKE_WEBRTC_NSX puts WebRtcNsx_* behind
 * ns_*; :168-191: `#undef MAKE_WEBRTC_AEC` puts WebRtcAecm_* behind aec_*), as stage bits of the one library: with WMX_CHAIN_NSX the
 * NS stage (WMX_CHAIN_NS must be set too) is the fixed-point suppressor, with WMX_CHAIN_AECM the AEC stage is the fixed-point
 * canceller.  A chain of NSX + AECM + AGC + VAD is integer end to end: bit-exact against the reference. */
#define WMX_CHAIN_NSX 16u
#define WMX_CHAIN_AECM 32u
typedef struct wmx_chain wmx_chain;
int wmx_chain_create(wmx_chain **out, int n_streams, int chn, int freq, int interval_ms, int agc_value, unsigned stages,
                     int n_cohorts);
/* stream_cohort: HOST array of n_streams entries (NULL: every stream in cohort 0) -- the cohort (control plane + far-end) each stream
 * belongs to from the start; wmx_chain_process_groups hands every cohort its OWN far-end: cohort c's 10 ms packet p at
 * d_far + c * far_group_stride + p * far_packet_stride (aec_process2's far-end is per handle, src/webrtc.c:410) */
int wmx_chain_create_groups(wmx_chain **out, int n_streams, int chn, int freq, int interval_ms, int agc_value, unsigned stages,
                            int n_cohorts, const int32_t *stream_cohort);
int wmx_chain_process_groups(wmx_chain *h, const int16_t *d_far, long far_packet_stride, long far_group_stride, const int16_t *d_in,
                             int16_t *d_out, int n10, long stream_stride, long packet_stride, const int32_t *delay_ms,
                             const uint8_t *cohort_on, int32_t *cohort_rc, void *stream);
int wmx_chain_destroy(wmx_chain *h);
/* webrtcEnable[] at run time (the daemon's message thread sets the switches, src/wmix.c:1010-1050): a stage whose bit drops is released
 * (src/wmix.c:783-813), one whose bit comes on is made anew -- fresh state for every stream, the cohorts the chain was created with,
 * agc_value as agc_init's value (< 0: the chain's own) -- stages that stay on keep their state.  stages = 0 is a heartbeat with every
 * switch off (the package passes through; such a chain works in place).  wmx_chain_create takes stages = 0 too.  A control-plane call:
 * the device is drained when a stage goes. */
int wmx_chain_set_stages(wmx_chain *h, unsigned stages, int agc_value);
unsigned wmx_chain_stages(const wmx_chain *h);
int wmx_chain_process(wmx_chain *h, const int16_t *d_far, long far_packet_stride, const int16_t *d_in, int16_t *d_out, int n10,
                      long stream_stride, long packet_stride, const int32_t *delay_ms, const uint8_t *cohort_on,
                      int32_t *cohort_rc, void *stream);
int wmx_chain_reset_streams(wmx_chain *h, const int32_t *idx, int n, int cohort, void *stream);
int wmx_chain_reset_cohort(wmx_chain *h, int cohort, void *stream);
/* wmx_chain_reset_streams with agc_init's own `value` for the new handles (the daemon creates the AGC with the volumeAgc of
 * that moment, src/wmix.c:684), and agc_addition for the listed streams of a running chain (src/wmix.c:1068-1070); a chain
 * without an AGC stage ignores the value */
int wmx_chain_reset_streams_gain(wmx_chain *h, const int32_t *idx, int n, int cohort, int agc_value, void *stream);
int wmx_chain_set_agc_gain_streams(wmx_chain *h, const int32_t *idx, int n, int agc_value, void *stream);
/* wmx_aec_add_cohort / wmx_aec_retire_cohort / wmx_aec_cohorts of the chain's AEC (a chain without one has a single cohort) */
int wmx_chain_add_cohort(wmx_chain *h, int *cohort, void *stream);
int wmx_chain_retire_cohort(wmx_chain *h, int cohort);
/* wmx_aec_coalesce / wmx_aecm_coalesce of the chain's echo canceller (a chain without one merges nothing) */
int wmx_chain_coalesce(wmx_chain *h, int max_pairs, int32_t *merged_from, int32_t *merged_into, int cap, int *n_merged, void *stream);
int wmx_chain_cohorts(const wmx_chain *h);
int wmx_chain_set_active(wmx_chain *h, const uint8_t *host_mask, void *stream);
int wmx_chain_stream_state_bytes(const wmx_chain *h);
int wmx_chain_export_stream(wmx_chain *h, int stream_index, void *host_blob);
int wmx_chain_import_stream(wmx_chain *h, int stream_index, const void *host_blob, int cohort);
wmx_ns *wmx_chain_ns(wmx_chain *h);
wmx_aec *wmx_chain_aec(wmx_chain *h);
wmx_agc *wmx_chain_agc(wmx_chain *h);
wmx_vad *wmx_chain_vad(wmx_chain *h);

/* ------------------------------------------------------------------ AECM (fixed-point echo canceller)
 * Batched form of the SAME five wrapper functions when the reference is built with its AECM switch (`#undef
 * MAKE_WEBRTC_AEC`, src/webrtc.c:168-191: WebRtcAecm_Create / Init / BufferFarend / Process, echo mode 3, comfort noise on,
 * W:modules/audio_processing/aecm/).  Same arguments, modes, strides, aliasing and return values as wmx_aec_*; one shared
 * far-end per batch.  When the reference returns -1 for a delay outside [0, 500] ms the packet HAS been processed with
 * the delay clamped (state advances) but its output is not written, as in the wrapper.  Integer path: bit-exact.  At
 * 8 kHz with 20 ms packets the reference replays an uninitialised buffer (farendOld[1]); it is zero here.
 * The legacy aec_init picks this implementation when the environment has WMIX_AMD_AECM=1. */
typedef struct wmx_aecm wmx_aecm;
int wmx_aecm_create(wmx_aecm **out, int n_streams, int chn, int freq, int interval_ms);
int wmx_aecm_destroy(wmx_aecm *h);
int wmx_aecm_packet_samples(const wmx_aecm *h);
int wmx_aecm_state_bytes(const wmx_aecm *h);
int wmx_aecm_run(wmx_aecm *h, int mode, const int16_t *d_far, long far_packet_stride, const int16_t *d_near,
                 int16_t *d_out, int n_packets, long stream_stride, long packet_stride, int delay_ms, void *stream);
/* Cohorts, as for the float AEC (see wmx_aec_run_cohorts): n_cohorts control planes + far-end histories per batch; every
 * stream starts in cohort 0.  far_group_stride: int16 elements between the far-end packets of consecutive cohorts (0: every
 * cohort hears the same far-end). */
int wmx_aecm_create_cohorts(wmx_aecm **out, int n_streams, int chn, int freq, int interval_ms, int n_cohorts);
int wmx_aecm_cohorts(const wmx_aecm *h);
int wmx_aecm_reset_cohort(wmx_aecm *h, int cohort, void *stream);
int wmx_aecm_add_cohort(wmx_aecm *h, int *cohort, void *stream); /* as wmx_aec_add_cohort / wmx_aec_retire_cohort */
int wmx_aecm_retire_cohort(wmx_aecm *h, int cohort);
/* as wmx_aec_coalesce / wmx_aec_live_cohorts: cohorts whose control planes have converged (the AECM's has no periodic counters: one
 * cohort per reported delay and phase of the 80-in-64 re-blocking remains) are merged after their far-end slabs -- far ring, frame
 * ring, the 256-block history of far spectra, Q-domains and binary spectra, the binary spectrum's running thresholds -- compared
 * equal on the device; the members' near and out frame rings are rotated; the comfort-noise generator was per stream already */
int wmx_aecm_coalesce(wmx_aecm *h, int max_pairs, int32_t *merged_from, int32_t *merged_into, int cap, int *n_merged, void *stream);
int wmx_aecm_live_cohorts(const wmx_aecm *h);
/* Why two cohorts do (not) fold: the words of the control plane that decide its future, positions taken out -- cohorts are proposed
 * for a merge when these are equal.  AEC (11): fill levels of the near / out / far-spectrum / far-sample rings, system delay, known
 * delay of the core, knownDelay, timeForDelayChange, msInSndCardBuf, filtDelay, lastDelayDiff (the core's two block counters, noise
 * floor and delay estimate, count with the stream).  AECM (8): fill levels of the far / frame / out rings, knownDelay, timeForDelayChange, msInSndCardBuf, filtDelay,
 * lastDelayDiff.  Returns 0, 1 (the cohort is retired or still in its start-up phase: no key), or WMX_E*. */
int wmx_aec_cohort_key(const wmx_aec *h, int cohort, int32_t *key11);
int wmx_aecm_cohort_key(const wmx_aecm *h, int cohort, int32_t *key8);
int wmx_aecm_reset_streams(wmx_aecm *h, const int32_t *idx, int n, int cohort, void *stream);
int wmx_aecm_set_active(wmx_aecm *h, const uint8_t *host_mask, void *stream);
int wmx_aecm_stream_state_bytes(const wmx_aecm *h);
int wmx_aecm_export_stream(wmx_aecm *h, int stream_index, void *host_blob);
int wmx_aecm_import_stream(wmx_aecm *h, int stream_index, const void *host_blob, int cohort);
int wmx_aecm_cohort_state_bytes(const wmx_aecm *h);
int wmx_aecm_export_cohort(wmx_aecm *h, int cohort, void *host_blob);
int wmx_aecm_import_cohort(wmx_aecm *h, int cohort, const void *host_blob);
int wmx_aecm_run_cohorts(wmx_aecm *h, int mode, const int16_t *d_far, long far_packet_stride, long far_group_stride,
                         const int16_t *d_near, int16_t *d_out, int n_packets, long stream_stride, long packet_stride,
                         const int32_t *delay_ms, const uint8_t *cohort_on, int32_t *cohort_rc, void *stream);
/* Echo control for the legs of a conference bridge: one canceller per leg, the leg's own sent audio as its far end.
 * wmx_aecm_create_legs makes n_legs cancellers, each the reference's handle aec_init(1, 8000, 20) that lives as long as the call does:
 * stream g is leg g, with a near state, far-end buffers AND a control plane of its own, all on the device -- a leg's call pattern
 * differs from every other leg's from the first jittered tick, so nothing is planned on the host and there are no cohorts: every
 * cohort entry point (wmx_aecm_run, _run_cohorts, _cohorts, _add_ / _retire_ / _reset_cohort, _coalesce, _live_cohorts, _cohort_key,
 * _cohort_state_bytes, _export_ / _import_cohort) returns WMX_ESTATE with a text on such a handle.  About 49 KB per leg, of which
 * 34.8 KB are the 256 far spectra the canceller looks back into.
 * wmx_aecm_process_legs, per tick, for every leg, in this order:
 *   1. the near rows.  Rows, strides, lengths, call lists and their refusals are those of wmx_nsx_process_legs: the leg's rows are
 *      taken in the order the load makes its calls, every row taken is ONE aec_process of 160 frames with the leg's reported delay, in
 *      place; a silence call or a data call on a row that is not readable feeds nothing; a row that is not taken -- late, duplicate,
 *      refused -- keeps its bytes.
 *   2. the far row.  d_far + g * far_leg_stride: the 160 samples this tick sent to leg g (what its speaker plays), one
 *      aec_setFrameFar of 160 frames.
 * d_pcm == NULL && d_len == NULL: far only; d_far == NULL: rows only; a far-only and a rows-only call compose to the combined one.  A
 * leg with no row this tick still buffers its far row: its far ring and control plane move, its near state (3.4 KB) is neither loaded
 * nor stored.  A leg switched off by wmx_aecm_set_active does neither step.  The bits are the reference's handle called in that
 * order (and those of wmx_aecm_run_cohorts with one cohort per leg, called alike); farendOld[1] starts as zeros, as above.
 * WHAT IT DOES: with a speech-like far end, an echo of 0.3 x far delayed by 517 samples and a reported delay of 20 ms, the echo's rms
 * falls to 0.10 - 0.14 of what it was within five seconds.  Stationary coloured noise and a tiled one-second excerpt do not
 * converge: the delay estimator needs a signal that is not periodic.  An echo path shorter than the reported delay is non-causal and
 * is not cancelled (517 -> 37 samples at 60 ms: 0.6).
 * WMX_EINVAL, nothing launched: a handle not made by wmx_aecm_create_legs; d_pcm and d_len and d_far all NULL; with rows, what
 * wmx_nsx_process_legs refuses; d_far on an odd address, or far_leg_stride < 160 with more than one leg.
 * wmx_aecm_set_delay_legs: the reported delay (ms in the sound card's buffers, 0 .. 500, else WMX_EINVAL and nothing changes -- the
 * wrapper's "-1, output unwritten" therefore cannot occur at run time) of the n legs listed in the host array idx, NULL: of all legs.
 * 0 at create; kept across wmx_aecm_reset_streams, like the AGC's gain.
 * wmx_aecm_export_legs: device arrays of n_legs int32, any of them NULL -- ec_startup (1 until the far ring has filled to the
 * reported delay), the far ring's fill in ms, knownDelay (samples), and the delay estimator's last_delay in 64-sample blocks (-2 before a
 * first estimate).
 * On such a handle wmx_aecm_reset_streams leaves the listed legs as aec_init does, far end and control plane included (cohort ignored);
 * wmx_aecm_set_active works as on any handle; wmx_aecm_export_stream / _import_stream carry the leg's WHOLE state -- near state,
 * far-end buffers, control plane, reported delay -- in one versioned blob of wmx_aecm_stream_state_bytes (cohort ignored). */
int wmx_aecm_create_legs(wmx_aecm **out, int n_legs);
int wmx_aecm_process_legs(wmx_aecm *h, int16_t *d_pcm, long leg_stride, long packet_stride, int max_packets, const uint32_t *d_len,
                          const uint32_t *d_calls, const int16_t *d_far, long far_leg_stride, void *stream);
int wmx_aecm_set_delay_legs(wmx_aecm *h, const int32_t *idx, int n, int delay_ms, void *stream);
int wmx_aecm_export_legs(wmx_aecm *h, int32_t *d_startup, int32_t *d_far_ms, int32_t *d_known_delay, int32_t *d_delay_blocks, void *stream);
/* the fixed-point stage handles of a chain made with WMX_CHAIN_NSX / WMX_CHAIN_AECM (NULL otherwise) */
wmx_nsx *wmx_chain_nsx(wmx_chain *h);
wmx_aecm *wmx_chain_aecm(wmx_chain *h);

/* ------------------------------------------------------------------ resample + mix
 * Batched forms of wmix_pcm_zoom (src/wmix.c:139-222) and of wmix_load_data + the play thread's drain
 * (src/wmix.c:1639-1957, 1347-1366).  Strides in int16 elements.  Integer path: bit-exact, including the
 * dead 2ch->2ch branch of wmix_pcm_zoom (writes 0 bytes) and the order-dependent saturating add. */
/* out_capacity: bytes available per output row; a conversion that needs more returns WMX_EINVAL with *out_len = the
 * bytes it needs (wmix_len_of_out gives the same figure beforehand) and writes nothing. */
int wmx_pcm_zoom(int inChn, int inFreq, const int16_t *d_in, uint32_t inLen, int outChn, int outFreq, int16_t *d_out,
                 uint32_t out_capacity, long in_stride, long out_stride, int n_streams, uint32_t *out_len, void *stream);
typedef struct wmx_mix wmx_mix;
int wmx_mix_create(wmx_mix **out, int n_groups, int ring_chn, int ring_freq);
int wmx_mix_destroy(wmx_mix *m);
int wmx_mix_set(wmx_mix *m, uint32_t head_off, uint32_t tick, int reduce_mode); /* wmix->head/tick/reduceMode */
/* VIEW_PLAY_CORRECT = PLAT_PLAY_CORRECT (src/wmixPlat.h:20; src/wmix.c:1668-1669): bytes in front of the play head where a source
 * without a cursor starts.  Compile-time in the reference, per platform directory: platform/alsa/plat.h:21 chn*freq*16/8/5 (200 ms;
 * what wmx_mix_create sets), platform/hi3516/plat.h:16 and platform/t31/plat.h:16 0.  A whole number of frames inside the ring, else
 * WMX_EINVAL.  (The legacy wmix_load_data of wmix_compat.h reads WMIX_AMD_PLAY_CORRECT=<bytes> from the environment.) */
int wmx_mix_set_play_correct(wmx_mix *m, uint32_t bytes);
int wmx_mix_ring_bytes(const wmx_mix *m);
/* wmx_mix_load, wmx_mix_load_minus and wmx_mix_load_minus_conf divide by the mixer's own reduce_mode alone: no ring is ducked under
 * its prompt (wmx_mix_play_duck) by them.  Only wmx_mix_load_minus_legs and wmx_mix_load_minus_legs_calls duck. */
int wmx_mix_load(wmx_mix *m, const int16_t *d_src, uint32_t srcU8Len, int freq, int channels, int sample, int n_src,
                 long group_stride, long source_stride, int reduce, uint32_t *head, uint32_t *tick, void *stream);
/* The bridge load: a mixer whose n_groups rings are read as n_groups / parties conferences of `parties` consecutive rings; ring
 * c*parties+q is what participant q of conference c hears -- everybody except themself.
 * For every conference c and every q: the ring c*parties+q afterwards holds what the reference's ring holds after
 * wmix_load_data(source s of conference c) for s = 0 .. parties-1, s != q, s not muted, in index order, every call from
 * the cursor (*head, *tick) -- wmx_mix_load's cursor rule, formats, reduce rule, look-ahead note and return values.
 * Source s of conference c at d_src + c*conf_stride + s*source_stride (int16 elements).  d_mute: NULL or n_groups bytes
 * ON THE DEVICE, non-zero = that participant's source is not loaded anywhere (they still hear the others).
 * One launch, every source read once: the saturating add is order dependent, so this is NOT "total minus own"
 * (wmix_amd/csrc/mix_minus.h).  WMX_EINVAL, nothing launched: parties < 2, parties > WMX_MIX_MAX_PARTIES, n_groups % parties != 0,
 * and whatever wmx_mix_load refuses.  It ducks no ring under a prompt (see wmx_mix_load). */
#define WMX_MIX_MAX_PARTIES 32
int wmx_mix_load_minus(wmx_mix *m, int parties, const int16_t *d_src, uint32_t srcU8Len, int freq, int channels, int sample,
                       long conf_stride, long source_stride, const uint8_t *d_mute, int reduce, uint32_t *head, uint32_t *tick,
                       void *stream);
/* The bridge load for conferences of different sizes whose legs join and leave.  A layout is n_conf conferences; conference c is the
 * ordered list host_members[host_off[c] .. host_off[c+1]) of ring indices (host_off[0] == 0, n_conf + 1 entries).  The indices of a
 * conference need not be consecutive or ascending: list order is the order of the saturating adds.  A ring is in at most one
 * conference; a ring in none is an idle leg (nothing is loaded into it, its source is not read).  A conference of 0 or 1 members is a
 * placeholder that keeps its index and loads nothing.  The layout is copied into buffers the handle owns, on `stream`; n_conf == 0
 * clears it.  wmx_mix_conferences: the n_conf in force.
 * wmx_mix_load_minus_conf: for every conference c of >= 2 members and every member q, the ring of q afterwards holds what the
 * reference's ring holds after wmix_load_data(source of member s) for every member s != q that is not muted, in list order, every
 * call from conference c's cursor (head[c], tick[c]) -- wmx_mix_load's cursor rule, formats, reduce rule, look-ahead note and return
 * values.  They all end at the same cursor, which is written back to head[c], tick[c]; a conference of fewer than 2 members gets
 * head[c] = UINT32_MAX, tick[c] = 0 (its cursor is forgotten).  So a leg that joins a running conference is loaded from the
 * conference's cursor, a conference that forms starts from a fresh one -- which may be the START of the ring (src/wmix.c:1666-1673),
 * so conferences alive together can write at different ring positions for good -- and a leg that leaves plays out what was loaded
 * ahead of its play head.  Source of ring r at d_src + r*source_stride (int16 elements); d_mute: NULL or n_groups bytes ON THE DEVICE,
 * by ring index; head / tick: HOST arrays of n_conf entries, in and out.  At most one launch per size class (<= 4, <= 8, <= 16,
 * <= 32 members) that has a conference; a call that finds every conference where the previous one left it relative to the others
 * uploads nothing (wmix_amd/csrc/bridge_layout.h).
 * WMX_EINVAL, nothing launched, rings, layout and cursors unchanged: a conference of more than WMX_MIX_MAX_PARTIES members, a ring
 * index outside [0, n_groups), a ring listed twice (in one conference or in two), host_off that does not ascend from 0,
 * wmx_mix_load_minus_conf without a layout, and whatever wmx_mix_load refuses.  It ducks no ring under a prompt (see wmx_mix_load). */
int wmx_mix_set_conferences(wmx_mix *m, int n_conf, const int32_t *host_off, const int32_t *host_members, void *stream);
int wmx_mix_conferences(const wmx_mix *m);
int wmx_mix_load_minus_conf(wmx_mix *m, const int16_t *d_src, uint32_t srcU8Len, int freq, int channels, int sample,
                            long source_stride, const uint8_t *d_mute, int reduce, uint32_t *head, uint32_t *tick, void *stream);
/* Talker selection on the device: of the legs of a conference only the loudest max_speakers are loaded into the others' rings.  The
 * call goes in front of the bridge load it feeds and writes that load's d_mute: wmx_mix_select_speakers addresses sources and indexes
 * masks like wmx_mix_load_minus, wmx_mix_select_speakers_conf like wmx_mix_load_minus_conf (the layout in force).
 * The rule is integer and exact (wmix_amd/csrc/speakers.h).  The mixer keeps one uint32 envelope env[r] per ring, zero at first.  For
 * the member at list position p (ring r) of a conference of at least 2 members:
 *   level    = sum of |x| over the srcU8Len / 2 int16 elements of the leg's source row as they lie there (all channels, before
 *              resampling and the reduce division; |-32768| = 32768)
 *   env'     = max(level, env - (env >> decay_shift)), stored for every member, the host-muted ones too
 *   eligible = !d_mute[r] && env' >= floor
 *   rank     = the eligible members s of the conference with env'[s] > env'[p], or env'[s] == env'[p] and s < p (list positions)
 *   speaking = eligible && rank < max_speakers;   d_mute_out[r] = !speaking
 * Every other ring (in no conference, or in one of 0 or 1 members) gets speaking = 0, d_mute_out = 1 and keeps its env.
 * d_mute: the host's mute, NULL or n_groups bytes ON THE DEVICE by ring; d_mute_out: n_groups bytes ON THE DEVICE.  Every source
 * element is read once; no host synchronisation, no upload and no allocation after the first call.
 * WMX_EINVAL, nothing launched, env unchanged: max_speakers outside 1 .. WMX_MIX_MAX_PARTIES, decay_shift outside 0 .. 31, a NULL
 * d_src or d_mute_out, a row of more than 131 071 elements (its level could overflow), the _conf form without a layout, and what the
 * corresponding load refuses about parties and n_groups.
 * wmx_mix_reset_speakers: env = 0 for the n rings host_idx lists (NULL = every ring), on `stream`: what a new call in a reused slot
 * does.  wmx_mix_export_speakers: env and speaking of every ring (n_groups entries each; either may be NULL) as the work queued on
 * `stream` leaves them; blocking. */
int wmx_mix_select_speakers(wmx_mix *m, int parties, const int16_t *d_src, uint32_t srcU8Len, long conf_stride, long source_stride,
                            const uint8_t *d_mute, int max_speakers, uint32_t floor, int decay_shift, uint8_t *d_mute_out, void *stream);
int wmx_mix_select_speakers_conf(wmx_mix *m, const int16_t *d_src, uint32_t srcU8Len, long source_stride, const uint8_t *d_mute,
                                 int max_speakers, uint32_t floor, int decay_shift, uint8_t *d_mute_out, void *stream);
int wmx_mix_reset_speakers(wmx_mix *m, const int32_t *host_idx, int n, void *stream);
int wmx_mix_export_speakers(const wmx_mix *m, uint32_t *host_env, uint8_t *host_speaking, void *stream);
/* Talker selection over leg packets, in front of wmx_mix_load_minus_legs: that call's layout, addressing (packet k of ring r at d_src +
 * r*source_stride + k*packet_stride) and d_len convention (slot k of ring r is a call if and only if d_len[r*max_packets + k] ==
 * srcU8Len).  The rule above with one change: level = the maximum, over the slots of the leg that are calls, of the level of that
 * slot's row; a leg with no call this tick has level 0.  So a leg whose slot 0 is a hole and whose packet sits in a later slot is as
 * loud as its packet.  Envelope, hold, floor, ranking and ties as above; d_mute_out is written for every ring and env stored for every
 * member.  With max_packets == 1 and every slot a call the result is wmx_mix_select_speakers_conf's.  One wave per conference, the rows
 * of the slots that are calls read once; no host synchronisation, no upload and no allocation after the first call.
 * WMX_EINVAL, nothing launched, env unchanged: what the _conf form refuses, max_packets outside 1 .. WMX_MIX_MAX_LEG_PACKETS, a NULL
 * d_len, rows that overlap (packet_stride < srcU8Len / 2 with more than one slot, source_stride shorter than a leg's slots). */
int wmx_mix_select_speakers_legs(wmx_mix *m, const int16_t *d_src, uint32_t srcU8Len, long source_stride, long packet_stride,
                                 int max_packets, const uint32_t *d_len, const uint8_t *d_mute, int max_speakers, uint32_t floor,
                                 int decay_shift, uint8_t *d_mute_out, void *stream);
/* The bridge load with a cursor per leg, for legs whose packets come early, late or not at all (an RTP leg delivers 0 .. 3 datagrams
 * in a tick).  Every wmix_thread_rtp_recv_pcma keeps a cursor of its own and calls wmix_load_data once per datagram that arrived
 * (src/wmixTask.c:1266-1316); here the mixer keeps one cursor (head, tick) per ring ON THE DEVICE, fresh (UINT32_MAX, 0) at first
 * and after wmx_mix_reset_leg_cursors, and a tick brings up to max_packets packets per leg: packet k of ring r at d_src +
 * r*source_stride + k*packet_stride (int16 elements), all of one format and one srcU8Len; wmx_mix_load's look-ahead note holds for
 * every packet row.  d_len: n_groups x max_packets uint32 ON THE DEVICE; slot k of leg r is a call if and only if
 * d_len[r*max_packets + k] == srcU8Len, any other value means the slot made no call, in the middle of a burst too.
 * Over the layout in force (wmx_mix_set_conferences): for every conference of >= 2 members, every member q and every member s != q
 * in list order, the ring of q afterwards holds what the reference's ring holds after wmix_load_data(packet k of s, &cursor of s)
 * for the slots k that are calls, in slot order; every call starts where leg s's previous call ended, in this tick or an earlier
 * one -- wmx_mix_load's cursor rule (a leg that fell behind the play head jumps to head + play_correct, one that runs ahead writes
 * further ahead), formats, reduce rule and return values.  d_mute (NULL or n_groups bytes ON THE DEVICE, by ring): a muted leg's
 * calls are made with zeros (WCT_SILENCE, src/wmixTask.c:1307-1309): its cursor moves, no ring changes.  A leg without a valid slot
 * makes no call and its cursor stays, so it falls behind as the play head moves and jumps when it returns.  A ring in no conference,
 * or in one of 0 or 1 members, keeps its cursor and receives nothing.
 * The one departure from the reference: a call whose end cursor would lie more than one ring ahead of the mixer's tick is not made,
 * nor are that leg's later slots of this tick (the reference laps the play head there and adds to what is queued); dropped[r] counts
 * the calls left out.
 * No host synchronisation, no upload and no allocation after the first call: one small kernel applies the cursor rule per leg
 * (wmix_amd/csrc/leg_cursor.h), then at most one load launch per size class (<= 4, <= 8, <= 16, <= 32 members) that has a conference;
 * every source element is read once.
 * WMX_EINVAL, nothing launched, rings, layout and cursors unchanged: no layout in force, max_packets outside 1 ..
 * WMX_MIX_MAX_LEG_PACKETS, a NULL d_src or d_len, max_packets packets that do not fit the ring, and whatever wmx_mix_load refuses about
 * the format.
 * wmx_mix_reset_leg_cursors: a fresh cursor and dropped = 0 for the n rings host_idx lists (NULL = every ring), on `stream`: what a
 * new call in a reused slot does.  wmx_mix_export_leg_cursors: head, tick and dropped of every ring (n_groups entries each; any may
 * be NULL) as the work queued on `stream` leaves them; blocking. */
#define WMX_MIX_MAX_LEG_PACKETS 4
int wmx_mix_load_minus_legs(wmx_mix *m, const int16_t *d_src, uint32_t srcU8Len, int freq, int channels, int sample,
                            long source_stride, long packet_stride, int max_packets, const uint32_t *d_len, const uint8_t *d_mute,
                            int reduce, void *stream);
/* The same load fed a CALL LIST per leg instead of the valid slots in slot order (wmx_rtp_sequence_legs writes the lists).  d_calls:
 * n_groups uint32 ON THE DEVICE, WMX_RTP_CALLS_* below; leg r makes WMX_RTP_CALLS_COUNT calls in list order, each with the cursor rule
 * above.  A silence call is a call with zeros (WCT_SILENCE): the cursor moves by one packet, no ring changes; a column that only
 * silence covers is not written.  d_len still says which rows are readable: a data call that names a slot k with
 * d_len[r*max_packets + k] != srcU8Len (or k >= max_packets) is made as a silence call.  The lap rule drops from the list's tail and
 * counts in dropped[r].  With every list "the valid slots in slot order, no silence" rings and cursors are byte for byte
 * wmx_mix_load_minus_legs'.  Refuses what that call refuses, and a NULL d_calls, and a ring that does not hold
 * WMX_MIX_MAX_LEG_PACKETS calls (a list may hold that many whatever max_packets is). */
int wmx_mix_load_minus_legs_calls(wmx_mix *m, const int16_t *d_src, uint32_t srcU8Len, int freq, int channels, int sample,
                                  long source_stride, long packet_stride, int max_packets, const uint32_t *d_len,
                                  const uint32_t *d_calls, const uint8_t *d_mute, int reduce, void *stream);
int wmx_mix_reset_leg_cursors(wmx_mix *m, const int32_t *host_idx, int n, void *stream);
int wmx_mix_export_leg_cursors(const wmx_mix *m, uint32_t *host_head, uint32_t *host_tick, uint32_t *host_dropped, void *stream);
/* wmx_mix_reset_rings: zero the n rings host_idx lists (NULL = every ring), on `stream`: a new call in a reused slot must not hear what
 * the old call had loaded ahead of the play head.  Head and tick are the mixer's, not the ring's, and stay.  A bad index: WMX_EINVAL,
 * nothing reset. */
int wmx_mix_reset_rings(wmx_mix *m, const int32_t *host_idx, int n, void *stream);
/* A prompt per ring: an announcement, a beep or hold music played into ring r by a task of its own, as wmix_task_play_wav
 * (src/wmixTask.c:1353-1595) plays a file into the daemon's ring -- a chunk per wmix_load_data call with the task's own cursor, and at the
 * end of the file it stops or sleeps `interval` and starts over, `repeat` times.  Only a mixer of 1 x 8000 rings has prompts: clips are
 * stored in the ring's own format (wmx_pcm_zoom converts anything else, once), so nothing is resampled in a tick.
 * wmx_mix_prompts(m, max_clips, max_samples): the store, made ONCE and blocking -- one arena of max_samples int16, one clip table
 * (offset, samples) of max_clips entries and one 32-byte state entry per ring; a second call is WMX_ESTATE.  wmx_mix_add_clip appends a
 * clip from HOST memory (blocking copy) and gives its index; clips stay until the mixer is destroyed.  Refused with nothing stored:
 * 0 samples, a full table, an arena too small (WMX_EINVAL), no store (WMX_ESTATE).
 * wmx_mix_play(m, host_idx, n, clip, repeat, gap_ticks, stream): the n rings host_idx lists (NULL = every ring) start `clip` from its
 * first sample with a FRESH cursor (the reference's NULL head: a new task); repeat = passes, 0 = until stopped; gap_ticks (0 .. 65 535)
 * = ticks of pause between two passes, the reference's `interval`.  A play over a playing ring replaces it; what is in the ring plays
 * out.  wmx_mix_stop: the listed rings go idle.  wmx_mix_reset_prompts: idle and done = 0, what a new call in a reused slot does; a mixer
 * without a store has nothing to reset.  All three are ordered on `stream`; a bad ring or clip index, a negative repeat or a gap outside
 * its range is WMX_EINVAL and changes nothing; play and stop without a store are WMX_ESTATE.
 * wmx_mix_load_prompts(m, stream): ONE tick of every ring's prompt, one launch, one wave per ring; call it behind the tick's load and in
 * front of its drain -- ring r then receives the other legs' calls first and the prompt's call last, and volumeAdd saturates, so the
 * order is part of the result.  The rule (wmix_amd/csrc/leg_prompt.h), per ring:
 *   idle: nothing.   wait > 0: wait--, no call.   Otherwise ONE wmix_load_data call of n = min(160, samples - pos) samples (2 n bytes of
 *   8000 / 1 / 16, reduce 1) with the task's cursor, pos += n; inside a pass the cursor is kept from call to call.   pos == samples on
 *   the last pass: idle, done++.   pos == samples with passes left: left-- unless endless, pos = 0, wait = gap_ticks, and the cursor is
 *   FRESH again, as the reference resets it behind its sleep (`head.U8 = wmix->head.U8; tick = 0`, src/wmixTask.c:1580-1581): the first
 *   call of EVERY pass jumps to head + VIEW_PLAY_CORRECT, so the pause heard between two passes is gap_ticks ticks (plus the 320 - 2 n
 *   bytes a short last call leaves unwritten) at every play_correct.
 * A repeated play inherits the reference's rule for the ring's end: a pass that begins where head + play_correct lies behind it starts
 * at the ring's START (src/wmix.c:1666-1673), so with play_correct 3 200 the passes that begin in the last 200 ms of a one-second lap
 * land on top of one another there; one long pass, or a platform with play_correct 0, has no such seam.
 * A ring in no conference, or alone in one, still plays its prompt.  The call never laps the play head (one call per tick, at most
 * play_correct + 320 bytes ahead).  Without a store wmx_mix_load_prompts launches nothing, and neither does it in a tick in which no ring
 * can still be playing: the host keeps, per ring, the launch by which its prompt has ended for certain, from the clip's length, repeat
 * and gap_ticks (never for an endless play), so a bridge that plays a beep now and then pays for the launch only while it sounds.
 * wmx_mix_play_duck(..., reduce, stream): wmx_mix_play with the reference's `reduce` (0 .. 15, wmixConf.h:72; anything else is
 * WMX_EINVAL), the argument of every play call of the reference (wmix.h:48-98): while the prompt plays, everything else loaded into its
 * ring is divided by D = reduce + 1 and the prompt itself is not.  wmx_mix_play is this with reduce 0.  The rule (leg_prompt.h, REDUCE):
 * ring r is DUCKED in a tick exactly when its prompt makes a call in that tick and was started with reduce > 0 -- on the state as the
 * tick's load finds it, in front of wmx_mix_load_prompts: playing, no pause left, samples left.  In a ducked tick every call another leg
 * makes into ring r adds trunc(c / D) per sample, the C division BEFORE the saturating add (src/wmix.c:1675-1676, 1685; a silence call
 * or a muted source adds 0 as ever); the prompt's own call is undivided and still last.  The pause between two passes is not ducked,
 * the first tick of the next pass is (src/wmixTask.c:1525-1527, 1555-1557); stop, reset and the end of the last pass release the duck; a
 * play over a playing ring replaces the divisor.  The play task takes the mode only if reduceMode == 1, so rings are ducked only while
 * the mixer's reduce_mode is 1; on any other mixer a ducking play is an ordinary play.  For a ducked ring the load's rdce is
 * (reduce == D) ? 1 : D with the load's own `reduce`.  Only wmx_mix_load_minus_legs and wmx_mix_load_minus_legs_calls duck: in a tick in
 * which a ducking play can still be making calls (the host's bound, as for wmx_mix_load_prompts) they launch one block per conference
 * in front of the sweeps, which fills the ducked members' rings by the plain ordered fold -- the members other than itself in list order,
 * x = clamp16(x + c / D) -- and the sweeps leave those rings alone; every other ring comes out of the two sweeps as ever, the ducked
 * member's source in it undivided.  Every other tick launches exactly what it launched before.  A ducked ring in no conference, or
 * alone in one, has nothing to duck.  wmx_mix_export_duck: per ring (n_groups bytes) the divisor the next load will apply, 1 for none,
 * as the work queued on `stream` leaves it; blocking; 1 everywhere without a store or on a mixer whose reduce_mode is not 1.
 * wmx_mix_export_prompts: per ring the clip (int32, -1 when idle), the samples consumed of the current pass, the
 * passes left (0 while playing: endless) and the prompts that ran to their end since the ring's reset (uint32), as the work queued on
 * `stream` leaves them; any pointer NULL; blocking; without a store -1, 0, 0, 0. */
int wmx_mix_prompts(wmx_mix *m, int max_clips, long max_samples);
int wmx_mix_add_clip(wmx_mix *m, const int16_t *host_pcm, long samples, int *clip);
int wmx_mix_play(wmx_mix *m, const int32_t *host_idx, int n, int clip, int repeat, int gap_ticks, void *stream);
int wmx_mix_play_duck(wmx_mix *m, const int32_t *host_idx, int n, int clip, int repeat, int gap_ticks, int reduce, void *stream);
int wmx_mix_export_duck(const wmx_mix *m, uint8_t *host_divisor, void *stream);
int wmx_mix_stop(wmx_mix *m, const int32_t *host_idx, int n, void *stream);
int wmx_mix_reset_prompts(wmx_mix *m, const int32_t *host_idx, int n, void *stream);
int wmx_mix_load_prompts(wmx_mix *m, void *stream);
int wmx_mix_export_prompts(const wmx_mix *m, int32_t *host_clip, uint32_t *host_pos, uint32_t *host_left, uint32_t *host_done,
                           void *stream);
int wmx_mix_drain(wmx_mix *m, int16_t *d_out, uint32_t bytes, long out_stride, void *stream);
int wmx_mix_export(const wmx_mix *m, int group, int16_t *host_ring, uint32_t *head_off, uint32_t *tick);

/* ------------------------------------------------------------------ math/fft.c (stand-alone radix-2 FFT helpers)
 * Batched form of FFT / FFTR / IFFT / IFFTR (math/fft.h:19-38, math/fft.c:121-398): n_batch independent
 * transforms of N points per launch, arrays laid out [n_batch][N] float on the device.  kind: 0 FFT, 1 FFTR,
 * 2 IFFT, 3 IFFTR.  As in the reference any of the arrays may be NULL: a NULL input reads as zeros, a NULL output is
 * skipped; the inverses have no amplitude / phase outputs (d_out_af / d_out_pf are ignored for kind >= 2); the real
 * variants never read d_in_im.  N must be a power of two, 2 <= N <= 4096, else WMX_EINVAL.  Bit-exact for
 * re / im / amplitude (the twiddles are the reference's double cos/sin values, tabulated on the host);
 * the phase curve is a double atan2 rounded to float. */
#define WMX_MFFT_FFT 0
#define WMX_MFFT_FFTR 1
#define WMX_MFFT_IFFT 2
#define WMX_MFFT_IFFTR 3
int wmx_mfft(int kind, int n_batch, unsigned N, const float *d_in_re, const float *d_in_im, float *d_out_re,
             float *d_out_im, float *d_out_af, float *d_out_pf, void *stream);
/* Batched fft_stream (math/fft.h:51, math/fft.c:413-424): for every stream, move pool[in_len..2*in_len) to the front,
 * append the in_len new samples behind it, transform the st_len-point pool and write the amplitude / phase curves
 * (either may be NULL).  d_in [n_streams][in_len], d_pool [n_streams][st_len] (updated in place), outputs
 * [n_streams][st_len].  Requires 2*in_len <= st_len (the reference reads past the pool otherwise). */
int wmx_mfft_stream(int n_streams, const float *d_in, unsigned in_len, float *d_pool, unsigned st_len, float *d_out_af,
                    float *d_out_pf, void *stream);

/* ------------------------------------------------------------------ RTP / G.711 packet edge
 * Egress: for n_streams senders set up like wmix_thread_rtp_send_pcma does (src/wmixTask.c:1058: v = 2, m = 1,
 * seq = timestamp = ssrc = 0; pt 8 for law WMX_LAW_A, pt 0 for WMX_LAW_U), one call produces one datagram per stream
 * from that stream's PCM: wmix_pcm_zoom(in_chn, in_freq -> out_chn, out_freq), G.711 encode, timestamp += codes /
 * out_chn, network-order header (src/rtp.c:35-70, src/rtp.h:37-75), seq += 1 -- the loop body of
 * src/wmixTask.c:1124-1143 fused into one kernel.  d_pcm rows are pcm_stride int16 apart and in_bytes long; d_packets
 * rows packet_stride bytes apart; *packet_bytes receives 12 + number of codes.
 * Ingest (stateless): payload size by payload type as rtp_recv decides it (160 for PCMA / PCMU, else 0;
 * src/rtp.c:86-95) and G711a2PCM of the payload (src/wmixTask.c:1282): d_pcm rows get 160 int16, d_pcm_bytes[s] = 320
 * or 0, d_seq_raw[s] = header bytes 2..3 as the reference leaves them (no ntohs).  Optional outputs may be NULL. */
typedef struct wmx_rtp wmx_rtp;
int wmx_rtp_create(wmx_rtp **out, int n_streams, int law);
int wmx_rtp_destroy(wmx_rtp *h);
int wmx_rtp_egress(wmx_rtp *h, int in_chn, int in_freq, const int16_t *d_pcm, uint32_t in_bytes, long pcm_stride, int out_chn,
                   int out_freq, uint8_t *d_packets, long packet_stride, uint32_t *packet_bytes, void *stream);
int wmx_rtp_ingest(int n_streams, const uint8_t *d_packets, long packet_stride, int16_t *d_pcm, long pcm_stride,
                   uint32_t *d_pcm_bytes, uint16_t *d_seq_raw, void *stream);
/* Ingest for legs that deliver up to max_packets datagrams in a tick, in front of wmx_mix_load_minus_legs: the receive loop's
 * `ret > 0 && retSize > 0` (src/wmixTask.c:1278-1284) per datagram slot.  Datagram slot k of leg r at d_packets + r*leg_stride +
 * k*packet_stride (bytes); d_recv_bytes: n_legs x max_packets int32 ON THE DEVICE, what recvfrom returned for the slot (<= 0 =
 * nothing there, the row is not read).  PCM row of slot k of leg r at d_pcm + r*source_stride + k*pcm_packet_stride (int16
 * elements).  Payload size by payload type and the decode are wmx_rtp_ingest's; d_len[r*max_packets + k] = 320 for a slot that is a
 * call, 0 otherwise -- and then the slot's 160 PCM elements are zeroed, so a level taken over slot-0 rows is 0 for an absent leg.
 * d_seq_raw (optional, n_legs x max_packets): as wmx_rtp_ingest leaves it for a slot where something arrived, 0 otherwise.
 * WMX_EINVAL: a NULL d_packets, d_recv_bytes, d_pcm or d_len, max_packets outside 1 .. 4, rows that overlap (packet_stride < 172,
 * pcm_packet_stride < 160, or a leg stride shorter than its max_packets rows). */
int wmx_rtp_ingest_legs(int n_legs, int max_packets, const uint8_t *d_packets, long leg_stride, long packet_stride,
                        const int32_t *d_recv_bytes, int16_t *d_pcm, long source_stride, long pcm_packet_stride, uint32_t *d_len,
                        uint16_t *d_seq_raw, void *stream);
/* Play and send in one kernel, for a mixer whose rings are 1 x 8000 and a sender set with as many streams as the mixer has rings: per
 * ring, the 160 samples at the ring head are read, zeroed as the play thread does (src/wmix.c:1351-1352), encoded with the handle's law
 * and written behind the 12-byte header; then head and tick advance as wmx_mix_drain advances them, seq and timestamp as
 * wmx_rtp_egress does.  Datagrams, rings, head, tick, seq and timestamp afterwards are byte for byte those of wmx_mix_drain(320 bytes)
 * followed by wmx_rtp_egress(1, 8000 -> 1, 8000); the PCM row between the two never exists.  *packet_bytes (optional) receives 172.
 * WMX_EINVAL, nothing launched, nothing advanced: another ring format, a ring count that is not the sender count, a NULL h, m or
 * d_packets, packet_stride < 172, a mixer and senders on different devices.
 * wmx_rtp_reset_streams: seq = timestamp = 0 for the n senders host_idx lists (NULL = all), on `stream`: what
 * wmix_thread_rtp_send_pcma starts a call from (src/wmixTask.c:1058).  A bad index: WMX_EINVAL, nothing reset. */
int wmx_rtp_egress_rings(wmx_rtp *h, wmx_mix *m, uint8_t *d_packets, long packet_stride, uint32_t *packet_bytes, void *stream);
/* What each leg was sent, as its phone's speaker plays it: the 160 G.711 codes behind the 12-byte header of leg g's outgoing datagram
 * (d_packets + g * packet_stride, what wmx_rtp_egress_rings has just written) decoded with leg g's outgoing law (wmx_rtp_set_codecs;
 * the law of create until then) into d_pcm + g * pcm_leg_stride (samples; d_pcm on a 2-byte boundary).  The far end of the leg's echo
 * canceller (wmx_aecm_process_legs).  WMX_EINVAL: a NULL pointer, packet_stride < 172, pcm_leg_stride < 160 with more than one leg. */
int wmx_rtp_decode_sent_legs(wmx_rtp *h, const uint8_t *d_packets, long packet_stride, int16_t *d_pcm, long pcm_leg_stride, void *stream);
int wmx_rtp_reset_streams(wmx_rtp *h, const int32_t *host_idx, int n, void *stream);
int wmx_rtp_export(wmx_rtp *h, int stream_index, uint16_t *seq, uint32_t *timestamp);
/* Reorder, de-duplicate and gap-fill legs by RTP sequence number, between wmx_rtp_ingest_legs and the selection / the load
 * (wmix_amd/csrc/leg_seq.h holds the rule).  The reference makes one wmix_load_data call per datagram in arrival order and never reads
 * the sequence number: a lost packet moves every later one 20 ms early, a duplicate is mixed twice, two packets swapped on the wire are
 * mixed swapped.  Here the handle keeps, per leg (its n_streams), `synced` and `next` -- the sequence number of the next call position
 * -- and the counters lost, late, dup, resync, overflow, ON THE DEVICE, and one launch (one lane per leg) decides which calls the leg
 * makes this tick and in which order.  Slot k of leg r is `ok` when d_len[r*max_packets + k] == 320 (what ingest left; an unknown
 * payload type is not ok, so a packet that consumed a sequence number without audio becomes a gap); its sequence number s is header
 * byte 2 * 256 + byte 3, read from d_seq_raw (n_legs x max_packets, as wmx_rtp_ingest_legs leaves it, no ntohs: swapped here).
 *   no slot ok: no calls, state unchanged.  Not synced: synced = 1, next = s of the first ok slot.
 *   (uint16)(next - s) in 1 .. WMX_RTP_SEQ_MISORDER: LATE, discarded.  Every other ok slot is a candidate at forward distance
 *   u = (uint16)(s - next); candidates ascending by u, ties by slot; the same u as the predecessor: a DUPlicate, discarded.
 *   Walk with pos = 0: gap = u - pos; gap > max_gap: RESYNC (a sender that restarted; no silence, gap = 0); else the candidate needs
 *   gap silence calls (LOST += gap) and one data call; when they do not fit in what is left of WMX_MIX_MAX_LEG_PACKETS calls it and
 *   every later candidate are discarded (OVERFLOW counts them); else pos = u + 1.  A packet more than WMX_RTP_SEQ_MISORDER back is
 *   far ahead in uint16 arithmetic and resyncs.  next += pos; no trailing silence -- what has not come may come next tick.
 * d_calls[r] receives the list (WMX_RTP_CALLS_*): for wmx_mix_load_minus_legs_calls; every discarded slot gets d_len = 0, so talker
 * selection behind this stage does not hear late packets or duplicates.  max_gap 0 .. 3.  No atomics, no host synchronisation, no
 * upload, no allocation after the first call (wmx_rtp_reset_sequence counts as one).
 * OUT OF SCOPE: placing a late packet into its still-unplayed gap; SSRC changes; timestamp-based placement.  (What a silence call
 * sounds like is wmx_rtp_conceal_legs' business, below.)
 * WMX_EINVAL, nothing launched, state unchanged: a NULL h, d_seq_raw, d_len or d_calls, max_packets outside 1 .. 4, max_gap outside
 * 0 .. 3.
 * wmx_rtp_reset_sequence: unsynced and counters 0 for the n legs host_idx lists (NULL = all), on `stream`: a new call may start at any
 * sequence number.  A bad index: WMX_EINVAL, nothing reset.
 * wmx_rtp_export_sequence: next (uint16), synced (uint8) and the counters (uint32), n_streams entries each, any pointer NULL, as the
 * work queued on `stream` leaves them; blocking. */
#define WMX_RTP_SEQ_MISORDER 16
#define WMX_RTP_CALLS_COUNT(c) ((c) & 7u)                           /* 0 .. WMX_MIX_MAX_LEG_PACKETS */
#define WMX_RTP_CALLS_SLOT(c, j) (((c) >> (4 + 4 * (j))) & 3u)      /* the slot call j reads */
#define WMX_RTP_CALLS_SILENCE(c, j) (((c) >> (6 + 4 * (j))) & 1u)   /* call j is made with zeros */
int wmx_rtp_sequence_legs(wmx_rtp *h, int max_packets, int max_gap, const uint16_t *d_seq_raw, uint32_t *d_len, uint32_t *d_calls,
                          void *stream);
int wmx_rtp_reset_sequence(wmx_rtp *h, const int32_t *host_idx, int n, void *stream);
int wmx_rtp_export_sequence(wmx_rtp *h, uint16_t *next, uint8_t *synced, uint32_t *lost, uint32_t *late, uint32_t *dup,
                            uint32_t *resync, uint32_t *overflow, void *stream);
/* Conceal lost packets from each leg's own history, between wmx_rtp_sequence_legs (and the selection) and the load
 * (wmix_amd/csrc/leg_plc.h holds the rule).  The sequence rule makes a gap of 1 .. 3 lost packets that many WCT_SILENCE calls: the cursor
 * stays right, and every other leg of the conference hears 20 .. 60 ms of hard zero cut into speech, with a click at both edges.  The
 * reference has no counterpart.  Here the handle keeps, per leg (its n_streams) and ON THE DEVICE, hist[320] int16 -- the last 320
 * samples the leg emitted, newest at index 319, all 0 when fresh -- and a counter `concealed`, and one launch rewrites every leg's
 * calls of the tick into rows that are all data.  Integer arithmetic; >> is an arithmetic shift on int32.
 *   Input per leg: its PCM rows (slot k of leg r at d_pcm + r*source_stride + k*pcm_packet_stride, int16 elements), d_len (n_legs x
 *   max_packets) and the call list d_calls[r] exactly as wmx_rtp_sequence_legs leaves them (WMX_RTP_CALLS_*), walked in list order.  A
 *   data call that names a slot k >= max_packets, or a slot with d_len != 320, is a silence call, as the load treats it.
 *   A RUN is a maximal sequence of consecutive silence calls in the list.  At the start of a run: h0 = hist is frozen; q[i] = h0[i] >> 4
 *   (|q| <= 2048); for every lag L in 40 .. 120, c(L) = sum over i = 160 .. 319 of q[i] * q[i - L] (i - L >= 40; |c| <= 160 * 2^22 <
 *   2^31); L* = the smallest L with the largest c(L).  No normalisation, no threshold: an all-zero history gives L* = 40 and zeros out.
 *   SYNTHESIS: sample i of the n-th silence call of the run (n = 1, 2, ..) has k = (n - 1) * 160 + i, s = h0[320 - L* + (k mod L*)],
 *   g = max(0, 32768 - 68 * k), y = (s * g) >> 15.  concealed += 1 per synthesised packet.
 *   BLEND: a data call that directly follows a run of n_s silence calls in the same list, x its row: for i in 0 .. 31, cont = the
 *   synthesis formula at k = n_s * 160 + i and y[i] = (x[i] * i + cont * (32 - i)) >> 5; for i in 32 .. 159, y[i] = x[i].  A data call
 *   not preceded by silence in the list -- the first call, a data call after another, a resync -- is emitted unchanged.
 *   HISTORY: after each call its 160 emitted samples are appended to hist, keeping the last 320.  The history follows the list, not the
 *   load's lap rule (a call the load later drops has still been heard by the history), and mute does not enter the rule: a muted leg's
 *   state advances, and the load writes zeros for it as before.
 * Out: d_pcm_out, n_legs x 4 x 160 int16, the emitted rows in call order (rows j >= count are not written), and d_len_out, n_legs x
 * 4 uint32: 320 for j < count, else 0 -- every call has become a data call, so wmx_mix_load_minus_legs with max_packets = 4,
 * source_stride 640 and packet_stride 160 consumes them unchanged.  A leg with no calls has unchanged state and a d_len_out row of
 * zeros.  d_pcm, d_len and d_calls are only read.  One launch (one wave per leg); no atomics, no host synchronisation, no upload, no
 * allocation after the first call (wmx_rtp_reset_conceal counts as one).
 * STILL OUT OF SCOPE: placing a late packet into its unplayed gap, timestamp-based placement, comfort noise.
 * WMX_EINVAL, nothing launched, state unchanged: a NULL pointer, max_packets outside 1 .. 4, rows that overlap (pcm_packet_stride <
 * 160, a source_stride shorter than a leg's max_packets rows, repaired rows that overlap the rows they are made from).
 * wmx_rtp_reset_conceal: hist = 0 and concealed = 0 for the n legs host_idx lists (NULL = all), on `stream`.  A bad index: WMX_EINVAL,
 * nothing reset.
 * wmx_rtp_export_conceal: hist (n_streams x 320 int16) and concealed (n_streams uint32), either pointer NULL, as the work queued on
 * `stream` leaves them; blocking. */
int wmx_rtp_conceal_legs(wmx_rtp *h, int max_packets, const int16_t *d_pcm, long source_stride, long pcm_packet_stride,
                         const uint32_t *d_len, const uint32_t *d_calls, int16_t *d_pcm_out, uint32_t *d_len_out, void *stream);
int wmx_rtp_reset_conceal(wmx_rtp *h, const int32_t *host_idx, int n, void *stream);
int wmx_rtp_export_conceal(wmx_rtp *h, int16_t *hist, uint32_t *concealed, void *stream);
/* DTMF per leg, heard in band and read from RFC 4733 telephone-event packets, between wmx_rtp_ingest_legs_codecs (and
 * wmx_rtp_sequence_legs) and the selection / the load (wmix_amd/csrc/leg_dtmf.h holds the rule).  The reference has no counterpart: a
 * key pressed in band is mixed as loud voice and an event packet is an unknown payload type.  Here the handle keeps, per leg (its
 * n_streams) and ON THE DEVICE, the debounce state, the last event timestamp, a counter `count` and ring[8], and one launch judges
 * every block of every leg.  Integer arithmetic.
 *   DIGIT CODES are the RFC 4733 event numbers: 0 .. 9 the keys 0 .. 9, 10 `*`, 11 `#`, 12 .. 15 A .. D; keypad (row r, column c) is
 *   code {1,2,3,12, 4,5,6,13, 7,8,9,14, 10,0,11,15}[4 r + c].
 *   A BLOCK is the 160 samples of one data call (d_len == 320).  For f = 697, 770, 852, 941 (rows), 1209, 1336, 1477, 1633 (columns),
 *   coef = 27980, 26956, 25701, 24219, 19073, 16325, 13085, 9315: from s1 = s2 = 0, s0 = x[n] + ((coef * s1) >> 14) - s2; s2 = s1;
 *   s1 = s0 over n = 0 .. 159, then P = s1 * s1 + s2 * s2 - ((coef * s1) >> 14) * s2 (int64).  E = sum of x[n]^2; r*, c* the row and the
 *   column with the largest P, ties to the lower index.  The block is a TONE of the digit at (r*, c*) when P_r* >= 400000000 and P_c* >=
 *   400000000, P_c* <= 4 P_r* and P_r* <= 8 P_c*, 8 P_i <= P_r* for every other row and 8 P_i <= P_c* for every other column, and
 *   P_r* + P_c* >= 32 E.
 *   The leg's blocks are taken in the order the load makes its calls: d_calls NULL, the slots with d_len == 320 in slot order; else
 *   the list d_calls[r] as wmx_rtp_sequence_legs leaves it, where a silence call, or a data call that names a row that is not readable,
 *   is a block that is not a tone.  A leg with no block keeps its state.
 *   DEBOUNCE: cand = the previous block's digit or none, cur = the digit that is down or none.  A tone of d with cand == d and cur != d
 *   reports d once and sets cur = d; a block that is not a tone behind one that was not a tone either sets cur = none; then cand = this
 *   block's digit or none.  A key fills two consecutive packets before it is reported.
 *   EVENT PACKETS are read from the datagram rows (d_in, d_recv: what wmx_rtp_ingest_legs_codecs was given), whatever the list says:
 *   every slot in slot order with d_recv >= 16, (byte 1 & 0x7F) == event_pt and event = byte 12 <= 15 reports `event` once when the leg
 *   has no last event timestamp or bytes 4 .. 7 differ from it, and stores those four bytes: retransmissions and end packets of one key
 *   press report nothing more.  Events above 15 are ignored.  The packet stays refused for the audio path.
 *   REPORT: report number n (from 0) of a leg is ring[n & 7] = code | 0x80 from a packet, code heard in band; count counts them; a
 *   tick's packet reports are stored before its in-band reports.  A host that polls at least every 8 reports reads every digit.
 *   suppress != 0: every block that is a tone (its own decision, not the debounced one) is zeroed in d_pcm IN PLACE, d_len unchanged: a
 *   data call of zeros for the selection, the concealment history and the load behind this stage.
 * One launch (half a wave per leg); no atomics, no host synchronisation, no upload, no allocation after the first call
 * (wmx_rtp_reset_dtmf counts as one).  OUT OF SCOPE: generating DTMF towards a leg, events above 15, a block other than the packet.
 * WMX_EINVAL, nothing launched, state unchanged: a NULL pointer other than d_calls, max_packets outside 1 .. 4, event_pt outside
 * 96 .. 127, rows that overlap (packet_stride < 172, pcm_packet_stride < 160, a leg stride shorter than its max_packets rows).
 * wmx_rtp_reset_dtmf: the fresh state for the n legs host_idx lists (NULL = all), on `stream`.  A bad index: WMX_EINVAL, nothing reset.
 * wmx_rtp_export_dtmf: count (n_streams uint32) and ring (n_streams x 8 uint8), either pointer NULL, as the work queued on `stream`
 * leaves them; blocking. */
int wmx_rtp_detect_dtmf_legs(wmx_rtp *h, int max_packets, const uint8_t *d_in, long leg_stride, long packet_stride,
                             const int32_t *d_recv, int16_t *d_pcm, long source_stride, long pcm_packet_stride, const uint32_t *d_len,
                             const uint32_t *d_calls, int event_pt, int suppress, void *stream);
int wmx_rtp_reset_dtmf(wmx_rtp *h, const int32_t *host_idx, int n, void *stream);
int wmx_rtp_export_dtmf(wmx_rtp *h, uint32_t *count, uint8_t *ring, void *stream);
/* Recording taps: what a ring is about to play, as PCM (wmix_amd/csrc/leg_record.h; the reference's wmix_thread_record_wav,
 * src/wmixTask.c:410-505, on the daemon that a leg of the bridge is).  The senders hold the store, as they hold the DTMF state.
 * wmx_rtp_recorders(h, max_taps, chn, freq): the store, once, blocking; max_taps taps of ONE format, chn 1 or 2, freq 1 .. 48 000; a
 *   second call is WMX_ESTATE.  wmx_rtp_record_row_bytes: the bytes of a row, constant: what wmix_pcm_zoom writes for one package of 320
 *   bytes of 1 x 8000 (one zoom call per package: the reader that keeps up; the reference's recorder reads 1 .. 5 packages per call
 *   depending on thread timing); 0 without a store.
 * wmx_rtp_record(h, host_idx, n, ticks, host_taps_out, stream): the n listed streams start, ordered on `stream`: a stream that has a
 *   tap is restarted in place, the others take the lowest free taps; `ticks` rows each, 0 = until stopped; host_taps_out (n int32 or
 *   NULL) takes the taps.  Fewer free taps than needed: WMX_ESTATE and nothing started.
 * wmx_rtp_record_stop(h, host_idx, n, stream): the listed streams' taps (NULL = every tap) are free from the next tick on, written
 *   stays.  wmx_rtp_reset_record: the same with written = 0, what a new call in a used slot needs; without a store it does nothing.
 * wmx_rtp_record_rings(h, mix, d_rows, row_stride, d_legs, stream): one tick of every tap, IN FRONT OF wmx_rtp_egress_rings on the same
 *   mixer (n_streams rings of 1 x 8000, the play head on a package boundary: anything else is WMX_EINVAL): a running tap reads ring
 *   `leg` at the play head WITHOUT zeroing it, gathers through wmix_pcm_zoom's schedule 1 x 8000 -> chn x freq and writes the row to
 *   d_rows + tap * row_stride (int16 elements) and its leg to d_legs[tap]; a free tap writes -1 and no row.  A tap with left == 1
 *   frees itself behind the row.
 * wmx_rtp_export_record: leg (int32, -1 free), left and written (uint32) of every TAP, any pointer NULL; blocking. */
int wmx_rtp_recorders(wmx_rtp *h, int max_taps, int chn, int freq);
int wmx_rtp_record_row_bytes(const wmx_rtp *h);
int wmx_rtp_record(wmx_rtp *h, const int32_t *host_idx, int n, int ticks, int32_t *host_taps_out, void *stream);
int wmx_rtp_record_stop(wmx_rtp *h, const int32_t *host_idx, int n, void *stream);
int wmx_rtp_reset_record(wmx_rtp *h, const int32_t *host_idx, int n, void *stream);
int wmx_rtp_record_rings(wmx_rtp *h, wmx_mix *m, int16_t *d_rows, long row_stride, int32_t *d_legs, void *stream);
int wmx_rtp_export_record(wmx_rtp *h, int32_t *leg, uint32_t *left, uint32_t *written, void *stream);
/* A G.711 codec per stream, as each call negotiated it (wmix_amd/csrc/leg_codec.h holds the rule).  The reference's receive thread
 * accepts payload types 8 and 0 alike and decodes both with G711a2PCM (src/rtp.c:88-95, src/wmixTask.c:1282), and a send thread has one
 * law.  Here the handle keeps, per stream and ON THE DEVICE, in_codec, out_law and a `refused` counter:
 *   arrived = recvfrom returned > 0 for the slot; pt = header byte 1 & 0x7F; g711 = arrived && (pt == 8 || pt == 0)
 *   WMX_CODEC_REFERENCE (the default)  a call when g711, decoded as A-law whatever the pt: the reference, and wmx_rtp_ingest_legs
 *   WMX_CODEC_PCMA                     a call when g711 && pt == 8, decoded as A-law
 *   WMX_CODEC_PCMU                     a call when g711 && pt == 0, decoded as mu-law (G711u2PCM, src/g711codec.c)
 *   WMX_CODEC_BY_PT                    a call when g711, decoded as mu-law if pt == 0, else as A-law
 *   refused = arrived && !call, in every mode (telephone-event packets, the AAC tag, the other law on a strict leg): refused[stream]++.
 * A refused slot is what a slot of another payload type is for wmx_rtp_ingest_legs: d_len = 0 and a zeroed PCM row, d_seq_raw written;
 * as everything downstream goes by d_len it is invisible to wmx_rtp_sequence_legs (not late, not a duplicate, does not sync), to talker
 * selection and to the load.  out_law: WMX_LAW_A sends payload type 8 and PCM2G711a, WMX_LAW_U payload type 0 and PCM2G711u, per stream
 * in wmx_rtp_egress and wmx_rtp_egress_rings (whose identity with wmx_mix_drain + wmx_rtp_egress holds with mixed laws); initially
 * the law of wmx_rtp_create.  A handle on which no stream ever left the default runs the launches of a handle that knows no codecs.
 * wmx_rtp_set_codecs: in_codec and out_law for the n streams host_idx lists (NULL = all), on `stream`; no host synchronisation and no
 * upload.  The refused counts stay.  WMX_EINVAL, nothing changed: an index outside the handle, an in_codec outside 0 .. 3, an out_law
 * that is neither law.  wmx_rtp_reset_streams and wmx_rtp_reset_sequence keep a stream's codec (a new call sets its own);
 * wmx_rtp_reset_sequence zeroes its refused count with the other receive counters.
 * wmx_rtp_export_codecs: in_codec, out_law (uint8) and refused (uint32), n_streams entries each, any pointer NULL, as the work queued
 * on `stream` leaves them; blocking.
 * wmx_rtp_ingest_legs_codecs: wmx_rtp_ingest_legs (same layouts, same refusals) for n_legs = the handle's streams with the rule above
 * per leg.  No allocation after the first call on the handle (wmx_rtp_set_codecs counts as one). */
#define WMX_CODEC_REFERENCE 0
#define WMX_CODEC_PCMA 1
#define WMX_CODEC_PCMU 2
#define WMX_CODEC_BY_PT 3
int wmx_rtp_set_codecs(wmx_rtp *h, const int32_t *host_idx, int n, int in_codec, int out_law, void *stream);
int wmx_rtp_export_codecs(wmx_rtp *h, uint8_t *in_codec, uint8_t *out_law, uint32_t *refused, void *stream);
int wmx_rtp_ingest_legs_codecs(wmx_rtp *h, int max_packets, const uint8_t *d_packets, long leg_stride, long packet_stride,
                               const int32_t *d_recv_bytes, int16_t *d_pcm, long source_stride, long pcm_packet_stride,
                               uint32_t *d_len, uint16_t *d_seq_raw, void *stream);

/* ------------------------------------------------------------------ the packet edge as a pipeline
 * What wmix_thread_rtp_recv_pcma, the record heartbeat and wmix_thread_rtp_send_pcma do for one stream per 20 ms
 * (src/wmixTask.c:1278-1316, src/wmix.c:613-709, src/wmixTask.c:1124-1143), for n_streams per step with only the 172-byte
 * RTP/PCMA datagrams (src/rtp.h:51-78) crossing PCIe: datagram -> wmx_rtp_ingest -> wmx_chain_process (two 10 ms packets, 8 kHz
 * mono) -> wmx_rtp_egress -> datagram.  A wmx_pipe owns `slots` (1 .. 16) sets of PINNED host rows for the datagrams in and out,
 * their device twins, a copy-in and a copy-out HIP stream and the events between them, all made once:
 *   wmx_pipe_in / _out / _far(h, slot)  the slot's host rows: n_streams x 172 bytes in, the same out, 160 far-end samples
 *   wmx_pipe_submit(h, d_far, &slot, stream)  queues H2D -> ingest, chain, egress on `stream` -> D2H for the NEXT slot (round robin)
 *                  and returns at once; it blocks only when that slot is still in flight from `slots` steps ago.  d_far: the
 *                  shared far-end's two 10 ms packets on the device, or NULL = the slot's own wmx_pipe_far samples
 *   wmx_pipe_wait(h, slot)  blocks until that slot's datagrams are in its out rows (slot < 0: every slot)
 *   wmx_pipe_step_resident  the three launches alone, on datagrams that are on the device already (rows in_stride / out_stride
 *                  bytes apart)
 * With three slots the H2D of step k + 1 and the D2H of step k - 1 overlap the compute of step k. */
typedef struct wmx_pipe wmx_pipe;
int wmx_pipe_create(wmx_pipe **out, int n_streams, int slots, int law, int agc_value, unsigned stages);
/* The same pipeline for a host that holds PCM: the heartbeat's own boundary is a package in host memory, worked on in place
 * (buffSrc: wmix_ai_read, src/wmix.c:609-612; ns / aec_process2 / agc / vad on it, :613-709).  A row is one package of one stream --
 * chn x freq x interval_ms, wmx_pipe_datagram_bytes() = WMIX_PKG_SIZE bytes -- the slot's far-end one package of the same format;
 * there is no ingest / egress, the chain (made with chn, freq, interval_ms, agc_value, stages) runs in place on the uploaded rows.
 * wmx_pipe_step_resident on such a pipe wants in_stride == out_stride. */
int wmx_pipe_create_pcm(wmx_pipe **out, int n_streams, int slots, int chn, int freq, int interval_ms, int agc_value, unsigned stages);
/* The same for CALLS: every stream hears a far-end of its own, as every handle of the reference does (aec_process2(fp, far, near, ..),
 * src/webrtc.c:410-483; the far-end of a call is the other party).  wmx_pipe_far(h, slot) then is n_streams rows of one package each
 * (stream-major like the near rows), and so is d_far of wmx_pipe_submit / wmx_pipe_step_resident.  Every stream is a control cohort
 * with a far-end history of its own (122 KB of device memory); the float canceller must be among the stages. */
int wmx_pipe_create_pcm_calls(wmx_pipe **out, int n_streams, int slots, int chn, int freq, int interval_ms, int agc_value, unsigned stages);
int wmx_pipe_destroy(wmx_pipe *h);
int wmx_pipe_slots(const wmx_pipe *h);
int wmx_pipe_datagram_bytes(const wmx_pipe *h);
uint8_t *wmx_pipe_in(wmx_pipe *h, int slot);
const uint8_t *wmx_pipe_out(wmx_pipe *h, int slot);
int16_t *wmx_pipe_far(wmx_pipe *h, int slot);
/* Failing clean.  A submit that fails BEFORE its first launch (taking the slot, the uploads) has advanced nothing: the same rows may be
 * submitted again.  One that fails LATER has lost the step -- the stages that ran have consumed its input, like the reference's heartbeat
 * when aec_process2 fails behind ns_process (src/wmix.c:613-709) -- and wmx_pipe_failed_steps counts it; in both cases the rotation,
 * the slots in flight and the download still owed for the previous step are as before the call, and the streams are drained.  Use ONE
 * compute stream per pipe (the download of a step is ordered behind its own egress whatever stream a later submit is given, but the
 * chain's state is not). */
int wmx_pipe_submit(wmx_pipe *h, const int16_t *d_far, int *slot, void *stream);
int wmx_pipe_wait(wmx_pipe *h, int slot);
long wmx_pipe_failed_steps(const wmx_pipe *h);
/* non-blocking wmx_pipe_wait: 1 = the rows of `slot` (< 0: of every slot) are in host memory, 0 = still on their way */
int wmx_pipe_poll(wmx_pipe *h, int slot);
int wmx_pipe_step_resident(wmx_pipe *h, const uint8_t *d_in, long in_stride, const int16_t *d_far, uint8_t *d_out, long out_stride,
                           void *stream);
wmx_chain *wmx_pipe_chain(wmx_pipe *h);
wmx_rtp *wmx_pipe_senders(wmx_pipe *h);

/* ------------------------------------------------------------------ a conference bridge of RTP/G.711 legs as a pipeline
 * What one wmix_thread_rtp_recv_pcma per leg (src/wmixTask.c:1266-1316), the play thread (src/wmix.c:1347-1366) and one
 * wmix_thread_rtp_send_pcma per leg (src/wmixTask.c:1058-1143) do, for n_legs legs per 20 ms tick with only datagrams crossing PCIe.
 * A wmx_conf owns a mixer of n_legs rings of 1 x 8000, n_legs senders, and `slots` (1 .. 16) sets of PINNED host rows with their device
 * twins, a copy-in and a copy-out stream and the events between them, all made once.  A leg delivers 0 .. max_packets (1 .. 4)
 * datagrams in a tick:
 *   wmx_conf_in(h, slot)    n_legs x max_packets datagram rows of wmx_conf_in_row_bytes() = 176 bytes (172 used; 4-byte boundaries)
 *   wmx_conf_recv(h, slot)  n_legs x max_packets int32: what recvfrom returned for the row (<= 0: nothing there, the row is not read)
 *   wmx_conf_out(h, slot)   n_legs x 172 bytes: the datagram to send to each leg
 *   wmx_conf_submit(h, &slot, stream)  takes the NEXT slot (round robin; wmx_conf_next_slot names it beforehand), uploads its in and
 *                  recv rows on the copy-in stream and, behind them on `stream`: wmx_rtp_ingest_legs_codecs -> wmx_mix_select_speakers_legs
 *                  (if selection is on) -> wmx_mix_load_minus_legs (reduce 1, 320-byte packages of 1 x 8000) -> wmx_rtp_egress_rings;
 *                  then the download of the out rows on the copy-out stream.  Returns at once; blocks only when that slot is still in
 *                  flight from `slots` submits ago.  With three slots the upload of tick t + 1 and the download of tick t - 1 run
 *                  beside the launches of tick t.  No allocation, no host synchronisation, no upload beyond the slot's rows.
 *   wmx_conf_wait(h, slot)  blocks until that slot's datagrams are in its out rows (slot < 0: every slot); wmx_conf_poll: 1 / 0
 *   wmx_conf_step_resident  the launches alone, on rows that are on the device already (same shapes, rows contiguous)
 * Setters, between submits, each ordered on `stream`: wmx_conf_set_conferences (wmx_mix_set_conferences over the legs);
 * wmx_conf_mute (n_legs bytes by leg in HOST memory, NULL = nobody; a muted leg's cursor moves, no ring changes);
 * wmx_conf_speakers (max_speakers 0 = off, else wmx_mix_select_speakers_legs' arguments: the host's mute goes into the selection and
 * the selection's mask into the load); wmx_conf_set_play_correct (wmx_mix_set_play_correct); wmx_conf_reset_legs: what a new call in a
 * used slot needs -- a fresh cursor, dropped = 0, env = 0, the ring zeroed, seq = timestamp = 0 -- for the n legs host_idx lists
 * (NULL = all).  wmx_conf_export_legs: head, tick, dropped, env (uint32) and speaking (uint8) of every leg, any pointer NULL; blocking.
 * wmx_conf_sequence(h, on, max_gap): between submits.  Off (the default) is the launch sequence above, the reference's arrival order.
 * On, a tick is wmx_rtp_ingest_legs_codecs (which then also leaves the sequence numbers) -> wmx_rtp_sequence_legs(max_gap) -> the selection
 * if on (it sees the rewritten d_len) -> wmx_mix_load_minus_legs_calls -> wmx_rtp_egress_rings; its buffers are made at create.
 * wmx_conf_reset_legs also resets the listed legs' sequence state: a new call may start at any sequence number without counting a
 * resync.  wmx_conf_export_sequence: wmx_rtp_export_sequence of the handle's legs.  max_gap outside 0 .. 3: WMX_EINVAL.
 * wmx_conf_set_codecs(h, host_idx, n, in_codec, out_law, stream): between submits; a G.711 codec per leg, as each call negotiated it
 * (wmx_rtp_set_codecs over the legs, NULL = all).  The default is the reference's behaviour -- WMX_CODEC_REFERENCE: whatever arrives
 * with payload type 8 or 0 is decoded as A-law -- and the `law` of wmx_conf_create is every leg's initial out_law.  WMX_CODEC_PCMA /
 * WMX_CODEC_PCMU accept only their own payload type and decode with their own law, WMX_CODEC_BY_PT decodes each packet by its payload
 * type; a packet that arrived and makes no call is REFUSED: counted per leg, and invisible to sequencing, selection and the load.  So
 * an A-law leg and a mu-law leg of one conference hear each other, each in its own codec.  wmx_conf_reset_legs keeps the listed legs'
 * codecs and zeroes their refused counts.  wmx_conf_export_codecs: in_codec, out_law (uint8) and refused (uint32) of every leg, any
 * pointer NULL; blocking.  A handle that never sets a codec runs the launches it ran before there were any.
 * wmx_conf_conceal(h, on): between submits; off is the default.  With sequencing on and concealment on a tick is
 * wmx_rtp_ingest_legs_codecs -> wmx_rtp_sequence_legs -> the selection if on (unchanged: it sees the rewritten d_len and the rows as
 * they arrived, and does not hear synthesised audio) -> wmx_rtp_conceal_legs -> wmx_mix_load_minus_legs on the repaired rows with
 * max_packets = 4 -> wmx_rtp_egress_rings.  With sequencing off the stage is not launched and its state does not move; with
 * concealment off the launches are those of a handle that never heard of it.  The repaired rows and the history are made the first time
 * it is switched on, never inside a submit.  wmx_conf_reset_legs also resets the listed legs' concealment state.
 * wmx_conf_export_conceal: concealed (uint32) of every leg (wmx_rtp_export_conceal); blocking.
 * wmx_conf_dtmf(h, on, suppress, event_pt): between submits; off is the default.  On, wmx_rtp_detect_dtmf_legs runs behind the ingest
 * (behind wmx_rtp_sequence_legs with sequencing on, on its call list) and in front of the selection: with suppress != 0 the selection,
 * the concealment history and the load see a key pressed in band as a data call of zeros -- the other legs do not hear it and it wins
 * no talker slot.  event_pt 96 .. 127 is the payload type the legs negotiated for telephone-event (101 in most offers); outside:
 * WMX_EINVAL.  Off, the launches are those of a handle that never heard of it; the state is made the first time it is switched on,
 * never inside a submit.  wmx_conf_reset_legs also resets the listed legs' DTMF state.  wmx_conf_export_dtmf: count (uint32) and ring
 * (8 uint8) of every leg (wmx_rtp_export_dtmf), either pointer NULL; blocking.
 * wmx_conf_denoise(h, on): between submits; off is the default.  On, wmx_nsx_process_legs runs behind the ingest, behind
 * wmx_rtp_sequence_legs (it is given the call list exactly when the sequencer ran) and behind wmx_rtp_detect_dtmf_legs, and in front of
 * the selection: every row a leg's load will consume goes through that leg's own fixed-point noise suppressor (a wmx_nsx stream of
 * 1 x 8000 with the policy ns_init sets), in place, in the order the load consumes them.  The keypad is judged on the row as it
 * arrived, and a suppressed key goes in as the zeros it became; the selection, the concealment history and the load all see the
 * cleaned rows, so a steadily noisy leg neither holds a talker slot nor is repeated by concealment.  A lost packet feeds the
 * suppressor nothing; a late, duplicate or refused packet is not touched.  Mute and selection act at the load: a muted leg's rows are
 * cleaned all the same.  Off, the launches are those of a handle that never heard of it and the suppressor's state does not move; the
 * suppressor is made the first time it is switched on, never inside a submit, and switching off and on again keeps its state.
 * wmx_conf_reset_legs also resets the listed legs' suppressor state.  wmx_conf_denoiser: the legs' wmx_nsx (NULL until the first
 * switch-on), for wmx_nsx_export_stream / wmx_nsx_import_stream on a leg.
 * wmx_conf_level(h, on, value): between submits; off is the default.  On, wmx_agc_process_legs runs directly behind the denoiser (behind
 * the ingest, wmx_rtp_sequence_legs -- it is given the call list exactly when the sequencer ran -- and wmx_rtp_detect_dtmf_legs) and in
 * front of the selection: every row a leg's load will consume goes through that leg's own AGC (a wmx_agc stream of 1 x 8000, interval
 * 10 ms, compression gain `value` dB: agc_init's `value`, the reference's wmix->volumeAgc), in place, in the order the load consumes
 * them -- one agc_process of the reference per leg over those rows.  The keypad is judged on the row as it arrived, and a suppressed key
 * goes in as the zeros it became; the selection, the concealment history and the load all see the levelled rows, so a quiet handset
 * competes for a talker slot at the level it is heard at, and concealment's history is levelled audio that is not fed to the AGC
 * again.  A lost packet feeds the AGC nothing; a late, duplicate or refused packet is not touched.  Mute and selection act at the
 * load: a muted leg's rows are levelled all the same.  The first switch-on makes the AGC with `value` for every leg; on a handle that
 * has one, a call with another `value` is wmx_agc_set_gain -- agc_addition for every leg, the state kept (blocking) -- and the same
 * `value` changes no leg's gain.  A `value` that wmx_agc_create or wmx_agc_set_gain refuses is WMX_EINVAL and changes nothing, the
 * switch included; with on == 0 the value is not looked at.  Off, the launches are those of a handle that never heard of it and the AGC's state does not move; the AGC is never made
 * inside a submit, and switching off and on again keeps its state and every leg's gain.  wmx_conf_reset_legs gives the listed legs a
 * fresh AGC state (wmx_agc_reset_streams) once the AGC has been made: a reset leg keeps its compression gain.  wmx_conf_leveller: the
 * legs' wmx_agc (NULL until the first switch-on), for wmx_agc_set_gain_streams (one leg's volume), wmx_agc_stream_gain and
 * wmx_agc_export_stream / wmx_agc_import_stream on a leg.
 * wmx_conf_gate(h, on): between submits; off is the default.  On, wmx_vad_process_legs runs directly behind the leveller (behind the
 * ingest, wmx_rtp_sequence_legs -- it is given the call list exactly when the sequencer ran --, wmx_rtp_detect_dtmf_legs and the
 * denoiser) and in front of the selection: every row a leg's load will consume is one vad_process of that leg's own voice-activity
 * gate (a wmx_vad stream of 1 x 8000, interval 20 ms: WebRtcVad mode 3, the last stage of the reference's record heartbeat), in
 * place, in the order the load consumes them -- the decision moves the leg's `reduce` one step in 0 .. 4 and the row is shifted
 * right by it.  The keypad is judged on the row as it arrived; the selection, the concealment history and the load all see the gated
 * rows, so a leg that sends only stationary room noise is heard 24 dB down and falls under a talker floor.  A lost packet feeds the
 * gate nothing; a late, duplicate or refused packet is not touched.  Mute and selection act at the load: a muted leg's rows are
 * gated all the same.  A FRESH GATE IS SHUT: vad_init leaves `reduce` at 4, so the first rows of a new call -- after the first
 * switch-on and after wmx_conf_reset_legs -- are attenuated (>> 3, 2, 1 at best), and a call is heard in full from its fifth row.
 * That is the reference's behaviour and is kept.  The first switch-on makes the VAD and two counters per leg; off, the launches are
 * those of a handle that never heard of it and neither the VAD's state nor the counters move; the VAD is never made inside a submit,
 * and switching off and on again keeps state and counters.  wmx_conf_reset_legs gives the listed legs a fresh gate
 * (wmx_vad_reset_streams: `reduce` back to 4) and zeroes their counters once the gate has been made.  wmx_conf_gater: the legs'
 * wmx_vad (NULL until the first switch-on), for wmx_vad_export_stream / wmx_vad_import_stream on a leg.  wmx_conf_export_gate: reduce
 * (uint8, 0 .. 4), voiced and unvoiced (uint32: the rows taken that were judged voice, after hangover, and those that were not) of
 * every leg, any pointer NULL; blocking; before the first switch-on reduce is 4 and the counts are 0.
 * wmx_conf_echo(h, on, delay_ms): between submits; off is the default.  A speakerphone or a hybrid on one leg returns the whole
 * conference to every other ear, wins a talker slot doing so, and concealment then repeats it: the classic reason a bridge has a
 * canceller per port.  The far end of leg g is the datagram the handle itself sent to leg g.  On, wmx_aecm_process_legs runs twice per
 * tick: with the ROWS alone between the denoiser and the leveller (behind the DTMF detection where the denoiser is off) -- the order of
 * the reference's record heartbeat, NS -> AEC -> AGC -> VAD (src/wmix.c:613-709) --, every row a leg's load will consume one
 * aec_process of 160 frames of the leg's own canceller (aec_init(1, 8000, 20) in the AECM build) with the leg's reported delay, in
 * place, in the order the load consumes them; and with the FAR ROW alone behind wmx_rtp_egress_rings: the 160 G.711 codes of the
 * datagram this tick sent to the leg, decoded with the law they were encoded in (wmx_rtp_decode_sent_legs), one aec_setFrameFar.  The
 * selection, the concealment history and the load see the cancelled rows.  A leg with no row this tick still buffers its far row.  The
 * first switch-on makes the canceller (about 49 KB per leg) and the far rows, every leg at delay_ms; a later one sets every leg to
 * delay_ms again; a delay outside 0 .. 500 is WMX_EINVAL and changes nothing, the switch included; off does not look at it, runs the
 * launches of a handle that never heard of it, and off and on again keeps the state.  wmx_conf_reset_legs gives the listed legs a
 * fresh canceller, far end and control plane included; the reported delay stays.  wmx_conf_canceller: the legs' wmx_aecm (NULL until
 * the first switch-on), for wmx_aecm_set_delay_legs and wmx_aecm_export_stream / _import_stream on a leg.  wmx_conf_export_echo:
 * what wmx_aecm_export_legs gives, into host arrays of n_legs int32, any pointer NULL; blocking; before the first switch-on 1, 0, 0, -2.
 * Prompts: announcements and hold music per leg.  The bridge is one reference daemon per leg, and a prompt to leg g is a wmix_play on
 * daemon g: one more task, with its own cursor, loading ring g beside the receive threads of the other legs.  wmx_conf_prompts(h,
 * max_clips, max_samples) makes the store once (wmx_mix_prompts on the handle's mixer; between submits, blocking; a second call is
 * WMX_ESTATE), and nothing is allocated in a submit afterwards; wmx_conf_add_clip appends a clip of 1 x 8000 int16 from host memory
 * (wmx_mix_add_clip; other formats are the caller's to convert).  wmx_conf_play(h, host_idx, n, clip, repeat, gap_ticks, stream) /
 * wmx_conf_stop(h, host_idx, n, stream): wmx_mix_play / wmx_mix_stop over the legs (NULL = every leg), between submits, ordered on
 * `stream` like wmx_conf_set_codecs.  With a store a tick calls wmx_mix_load_prompts (which launches only while a leg can be playing)
 * BEHIND the load of the legs and IN FRONT OF wmx_rtp_egress_rings: within a tick ring g receives the other legs' calls first and the prompt's call last.  The rule per leg and tick
 * is the one stated at wmx_mix_load_prompts.  A prompt passes none of the per-leg stages: it is not sequenced, concealed, denoised,
 * levelled, gated or ranked by talker selection, and env / speaking do not see it; with echo control on it is part of what the leg is
 * sent, hence in the leg's far row.  A leg in no conference, or alone in one, receives no legs and still plays its prompt: hold music.
 * wmx_conf_reset_legs sets the listed legs idle with done = 0 once the store exists.  wmx_conf_export_prompts: wmx_mix_export_prompts
 * of the handle's legs.  A handle that never makes the store runs exactly the launches it ran before.  wmx_conf_play_duck(...,
 * reduce, stream): wmx_mix_play_duck over the legs -- the reference's `reduce`, 0 .. 15: while the prompt makes calls the rest of the
 * conference reaches leg g divided by reduce + 1, the prompt undivided on top, so that "one minute left" is understood over five people
 * talking; the gap between two passes is not ducked; the rule is stated at wmx_mix_play_duck.  With echo control on the far row of a
 * ducked leg is the ducked mix it was sent.  Only ticks in which a ducking prompt can be making a call run the ducking form of the
 * load.  wmx_conf_export_duck: wmx_mix_export_duck of the handle's legs.  Resampling inside the tick is left out, for the reason
 * given at wmx_mix_prompts.
 * Recording: what a leg hears, as PCM (the reference's wmix_record on the daemon that the leg is; the rule is stated at
 * wmx_rtp_recorders and in wmix_amd/csrc/leg_record.h).  wmx_conf_recorders(h, max_taps, chn, freq): once per handle, between submits,
 * blocking; makes the store (one format per handle: chn 1 or 2, freq whatever wmx_pcm_zoom accepts up to 48 000) and two more `down`
 * buffers per slot, max_taps rows of wmx_conf_rec_row_bytes(h) bytes back to back and max_taps int32; a second call is WMX_ESTATE.  The
 * row length is constant -- the zoom is stateless and every call has 320 bytes in: ONE wmix_pcm_zoom call per package, the reader that
 * keeps up, where the reference's recorder reads 1 .. 5 packages per call depending on thread timing -- and is the number the zoom
 * writes, not wmix_len_of_out's bound.  wmx_conf_record(h, host_idx, n, ticks, taps_out, stream): the listed legs each take the lowest
 * free tap and record from the next tick on, `ticks` rows (0 = until stopped; the reference counts seconds by bytes of the source format
 * and breaks behind the write that completes second `time`: 50 x time packages, one package for time == 0); a leg that has a tap is
 * restarted in place; too few free taps is WMX_ESTATE with nothing started.  wmx_conf_record_stop (NULL = every tap) and
 * wmx_conf_reset_legs end the recording of the legs they name, as the reference's wmix_reset ends its record threads: the tap is free
 * from the next tick on.  In a tick in which a tap is running wmx_rtp_record_rings stands BEHIND wmx_mix_load_prompts and IN FRONT OF
 * wmx_rtp_egress_rings, and the slot's two buffers are downloaded with the datagrams: wmx_conf_rec(h, slot) and wmx_conf_rec_legs(h,
 * slot) are valid after wmx_conf_wait(h, slot), like wmx_conf_out; row i is valid in that slot exactly when rec_legs[i] >= 0, and is leg
 * rec_legs[i]'s.  A TAPPED LEG'S ROW is the 160 samples its datagram of the tick encodes, converted: everybody of its conference but the
 * leg itself, its prompt on top, ducked if it is ducked -- NOT the leg's own voice.  A RECORDER OF A CONFERENCE is one more leg of it: a
 * member, muted (wmx_conf_mute), never fed, its datagram ignored; its row holds everybody.  Nothing else about the tick changes: ring,
 * datagram, every counter and every stage's state are what they are without the tap.  wmx_conf_export_record: leg, left and written of
 * every TAP (wmx_rtp_export_record).  wmx_conf_step_resident_rec(h, d_in, d_recv, d_out, d_rec, rec_stride, d_rec_legs, stream): the
 * resident step with taps, d_rec max_taps rows rec_stride int16 apart and d_rec_legs max_taps int32 on the device; plain
 * wmx_conf_step_resident while a tap is running is WMX_ESTATE before anything is launched, so a recording never silently loses a
 * tick.  A handle without a store (wmx_conf_rec is NULL), and a tick in which no tap is running, run exactly the launches and copies
 * they ran before.
 * wmx_conf_mix / wmx_conf_senders: the handle's mixer and senders, for wmx_mix_export / wmx_rtp_export.
 * Use ONE compute stream per handle: the PCM rows, d_len and the masks between the launches are per handle, not per slot.
 * WMX_EINVAL: slots outside 1 .. 16, max_packets outside 1 .. 4, a law that is not WMX_LAW_A / WMX_LAW_U (create); a submit or resident
 * step with no layout in force (no slot is taken); a leg index outside the handle (nothing is reset, no codec set); an in_codec outside
 * 0 .. 3 or an out_law that is neither law.  A submit that fails before its
 * first launch has advanced nothing; the rotation and the slots in flight are as before any failed submit. */
typedef struct wmx_conf wmx_conf;
int wmx_conf_create(wmx_conf **out, int n_legs, int slots, int max_packets, int law);
int wmx_conf_destroy(wmx_conf *h);
int wmx_conf_set_conferences(wmx_conf *h, int n_conf, const int32_t *host_off, const int32_t *host_members, void *stream);
int wmx_conf_mute(wmx_conf *h, const uint8_t *host_mask, void *stream);
int wmx_conf_speakers(wmx_conf *h, int max_speakers, uint32_t floor, int decay_shift);
int wmx_conf_sequence(wmx_conf *h, int on, int max_gap);
int wmx_conf_export_sequence(wmx_conf *h, uint16_t *next, uint8_t *synced, uint32_t *lost, uint32_t *late, uint32_t *dup,
                             uint32_t *resync, uint32_t *overflow, void *stream);
int wmx_conf_conceal(wmx_conf *h, int on);
int wmx_conf_export_conceal(wmx_conf *h, uint32_t *concealed, void *stream);
int wmx_conf_dtmf(wmx_conf *h, int on, int suppress, int event_pt);
int wmx_conf_export_dtmf(wmx_conf *h, uint32_t *count, uint8_t *ring, void *stream);
int wmx_conf_denoise(wmx_conf *h, int on);
wmx_nsx *wmx_conf_denoiser(wmx_conf *h);
int wmx_conf_level(wmx_conf *h, int on, int value);
wmx_agc *wmx_conf_leveller(wmx_conf *h);
int wmx_conf_gate(wmx_conf *h, int on);
wmx_vad *wmx_conf_gater(wmx_conf *h);
int wmx_conf_export_gate(wmx_conf *h, uint8_t *reduce, uint32_t *voiced, uint32_t *unvoiced, void *stream);
int wmx_conf_echo(wmx_conf *h, int on, int delay_ms);
wmx_aecm *wmx_conf_canceller(wmx_conf *h);
int wmx_conf_export_echo(wmx_conf *h, int32_t *startup, int32_t *far_ms, int32_t *known_delay, int32_t *delay_blocks, void *stream);
int wmx_conf_set_codecs(wmx_conf *h, const int32_t *host_idx, int n, int in_codec, int out_law, void *stream);
int wmx_conf_export_codecs(wmx_conf *h, uint8_t *in_codec, uint8_t *out_law, uint32_t *refused, void *stream);
int wmx_conf_prompts(wmx_conf *h, int max_clips, long max_samples);
int wmx_conf_add_clip(wmx_conf *h, const int16_t *host_pcm, long samples, int *clip);
int wmx_conf_play(wmx_conf *h, const int32_t *host_idx, int n, int clip, int repeat, int gap_ticks, void *stream);
int wmx_conf_play_duck(wmx_conf *h, const int32_t *host_idx, int n, int clip, int repeat, int gap_ticks, int reduce, void *stream);
int wmx_conf_stop(wmx_conf *h, const int32_t *host_idx, int n, void *stream);
int wmx_conf_export_prompts(wmx_conf *h, int32_t *clip, uint32_t *pos, uint32_t *left, uint32_t *done, void *stream);
int wmx_conf_export_duck(wmx_conf *h, uint8_t *divisor, void *stream);
int wmx_conf_recorders(wmx_conf *h, int max_taps, int chn, int freq);
int wmx_conf_record(wmx_conf *h, const int32_t *host_idx, int n, int ticks, int32_t *taps_out, void *stream);
int wmx_conf_record_stop(wmx_conf *h, const int32_t *host_idx, int n, void *stream);
int wmx_conf_export_record(wmx_conf *h, int32_t *leg, uint32_t *left, uint32_t *written, void *stream);
int wmx_conf_rec_row_bytes(const wmx_conf *h);
const int16_t *wmx_conf_rec(wmx_conf *h, int slot);
const int32_t *wmx_conf_rec_legs(wmx_conf *h, int slot);
int wmx_conf_set_play_correct(wmx_conf *h, uint32_t bytes);
int wmx_conf_reset_legs(wmx_conf *h, const int32_t *host_idx, int n, void *stream);
int wmx_conf_slots(const wmx_conf *h);
int wmx_conf_in_row_bytes(const wmx_conf *h);
uint8_t *wmx_conf_in(wmx_conf *h, int slot);
int32_t *wmx_conf_recv(wmx_conf *h, int slot);
const uint8_t *wmx_conf_out(wmx_conf *h, int slot);
int wmx_conf_next_slot(const wmx_conf *h);
int wmx_conf_submit(wmx_conf *h, int *slot, void *stream);
int wmx_conf_wait(wmx_conf *h, int slot);
int wmx_conf_poll(wmx_conf *h, int slot);
int wmx_conf_step_resident(wmx_conf *h, const uint8_t *d_in, const int32_t *d_recv, uint8_t *d_out, void *stream);
int wmx_conf_step_resident_rec(wmx_conf *h, const uint8_t *d_in, const int32_t *d_recv, uint8_t *d_out, int16_t *d_rec, long rec_stride,
                               int32_t *d_rec_legs, void *stream);
int wmx_conf_export_legs(wmx_conf *h, uint32_t *head, uint32_t *tick, uint32_t *dropped, uint32_t *env, uint8_t *speaking, void *stream);
wmx_mix *wmx_conf_mix(wmx_conf *h);
wmx_rtp *wmx_conf_senders(wmx_conf *h);

/* ------------------------------------------------------------------ the paced heartbeat over S streams in host memory
 * The reference's record thread is a PACED loop: one package of WMIX_INTERVAL_MS (20 ms, src/wmixConf.h:112) per tick, the tick's work
 * and a sleep adding up to WMIX_INTERVAL_MS * 1000 - 2000 us (src/wmix.c:536-538, 820: DELAY_US(intervalUs); the play thread likewise,
 * :1468-1474) -- a tick's processing must be over 2 ms before the next package is due.  wmx_rt is that tick for n_streams concurrent
 * streams whose packages lie in (pinned) host memory: the streams are cut into sub-batches of `sub_batch` streams (the last one shorter),
 * each a wmx_pipe of its own (state, chain, pinned rows, device twins) on ONE upload stream and ONE download stream, and a tick queues
 *     H2D(b) -> [ingest ->] NS -> AEC -> AGC -> VAD [-> egress] of sub-batch b on `stream` -> D2H(b)
 * for b = 0 .. B-1 back to back: the upload of sub-batch b + 1 and the download of sub-batch b - 1 run beside the compute of b, so the
 * tick's latency is one sub-batch's upload + everybody's compute + one sub-batch's download instead of the sum of all three.  The
 * download of sub-batch b is queued by the submit of b + 1, behind its noise suppressor (see wmx_pipe_submit); the last one by the wait.
 *   wmx_rt_create_pcm / _rtp   as wmx_pipe_create_pcm / wmx_pipe_create, for n_streams (long) in sub-batches; slots >= 1 sets of rows
 *   wmx_rt_batches, wmx_rt_batch_streams(b), wmx_rt_pipe(b)   the sub-batches; rows of tick slot k: wmx_pipe_in / _out(wmx_rt_pipe(h, b), k)
 *   wmx_rt_far(h, slot)        the tick's shared far-end in host memory (uploaded once per tick when d_far is NULL)
 *   wmx_rt_submit              queues one tick (the next slot, round robin) and returns; *slot = its slot
 *   wmx_rt_wait                blocks until every row of every queued tick is in host memory (wmx_rt_poll: the same without blocking)
 *   wmx_rt_tick                both: returns when the last row of the tick is in host memory -- the latency a paced host sees
 *   wmx_rt_step_resident       the tick's launches alone on rows already in HBM (row of stream s at d_rows + s * stride bytes, in place
 *                              for PCM; d_out rows for RTP)
 * Returns 0 or the first sub-batch's error; a failed sub-batch has lost its step (wmx_pipe_failed_steps), the others ran.  A submit first
 * retires its slot on EVERY sub-batch (the later sub-batches read sub-batch 0's copy of a far-end from host memory), so ticks may be
 * submitted with no wait in between; a host that stays within `slots` ticks never waits there.
 * LATE TICKS.  wmx_rt_submit queues a tick behind the one in flight: past capacity (or after a long stall of the device) the backlog
 * never drains and every later tick carries it.  wmx_rt_try_submit sheds instead -- a late package costs that package, not the rest of
 * the call (the reference's producers that fell behind jump to the play head, src/wmix.c:1666-1673):
 *   wmx_rt_try_submit          never blocks.  When the previous tick has not landed in host memory on every sub-batch (its last slot's
 *                              download complete, asked with hipEventQuery only; a download not yet queued has not landed -- wmx_rt_poll
 *                              / _wait queue it) it returns WMX_DROPPED and changes nothing: no slot, no upload, no launch, *slot not
 *                              written, no stream's state advanced (NS, AEC, AGC, VAD, the RTP senders' seq / timestamp).  Otherwise it
 *                              is wmx_rt_submit.
 *   wmx_rt_dropped_ticks       the ticks dropped so far (never in wmx_pipe_failed_steps)
 *   wmx_rt_next_slot           the slot the next (try_)submit takes: the host writes that tick's rows (and far rows) there first.  With
 *                              try_submit alone at most one tick is in flight, so with slots >= 2 that slot is always free.
 * Streams whose packages are not all due at the same instant are served better as P handles of S / P streams released tick / P apart
 * (wmx_rt_submit at a group's release, wmx_rt_poll on the groups in flight): the device never idles long enough for its power
 * management to clock it down, and the latency is a third.  Measured on one MI355X, 16 kHz, 20 ms ticks, 30 000 ticks: 557 056 streams
 * in four groups, 0 misses of tick - 2 ms; 393 216 streams released all at once miss 0.04 - 0.4 % of their ticks (the host's wake-ups
 * and rare stalls of the device).
 * examples/host_paced.c is the paced loop in C (clock_nanosleep(TIMER_ABSTIME), --phases P); bench.py --paced the same from Python. */
typedef struct wmx_rt wmx_rt;
int wmx_rt_create_pcm(wmx_rt **out, long n_streams, int sub_batch, int slots, int chn, int freq, int interval_ms, int agc_value, unsigned stages);
int wmx_rt_create_rtp(wmx_rt **out, long n_streams, int sub_batch, int slots, int law, int agc_value, unsigned stages);
/* calls: every stream its own far-end (wmx_pipe_create_pcm_calls); the far rows of sub-batch b are wmx_pipe_far(wmx_rt_pipe(h, b), slot),
 * a d_far on the device holds all n_streams rows (wmx_rt_far is sub-batch 0's) */
int wmx_rt_create_pcm_calls(wmx_rt **out, long n_streams, int sub_batch, int slots, int chn, int freq, int interval_ms, int agc_value, unsigned stages);
int wmx_rt_destroy(wmx_rt *h);
/* sub-batch b on the library's own compute stream b % n (n = 1, the default: all on the caller's stream, one behind the other; n >= 2:
 * forked from the caller's stream per tick and joined to it again, so that the tail of one sub-batch's kernels overlaps the head of the
 * next -- measured: no gain, the chain's kernels are bound by vector issue) */
int wmx_rt_set_compute_streams(wmx_rt *h, int n);
int wmx_rt_batches(const wmx_rt *h);
int wmx_rt_batch_streams(const wmx_rt *h, int batch);
wmx_pipe *wmx_rt_pipe(wmx_rt *h, int batch);
int16_t *wmx_rt_far(wmx_rt *h, int slot);
int wmx_rt_submit(wmx_rt *h, const int16_t *d_far, int *slot, void *stream);
/* WMX_DROPPED: a positive return, not an error -- the tick was shed (see LATE TICKS above) */
#define WMX_DROPPED 1
int wmx_rt_try_submit(wmx_rt *h, const int16_t *d_far, int *slot, void *stream);
long wmx_rt_dropped_ticks(const wmx_rt *h);
int wmx_rt_next_slot(const wmx_rt *h);
int wmx_rt_wait(wmx_rt *h);
int wmx_rt_poll(wmx_rt *h); /* non-blocking wmx_rt_wait: 1 = every row of every queued tick is in host memory, 0 = not yet */
int wmx_rt_tick(wmx_rt *h, const int16_t *d_far, int *slot, void *stream);
int wmx_rt_step_resident(wmx_rt *h, uint8_t *d_rows, long stride, const int16_t *d_far, uint8_t *d_out, long out_stride, void *stream);

/* ------------------------------------------------------------------ AEC far-end delay FIFO
 * Batched form of playPkgBuff_add/get and recordPkgBuff_add/get (src/wmix.c:432-526): n_slots packets
 * (AEC_FIFO_PKG_NUM = AEC_INTERVALMS / WMIX_INTERVAL_MS + 2, src/wmixConf.h:141) of pkg_bytes per stream, resident on
 * the device.  add: the packets of all streams (rows `stride` bytes apart) go into the slot under the cursor.
 * get: the packet the reference's index arithmetic selects for `delayms` is copied to d_out (rows `stride` bytes
 * apart) -- the arithmetic is reproduced as written, see oracle/orc_pkgfifo.c for what it amounts to.  A delay that
 * makes the reference read in front of its array returns WMX_EINVAL. */
typedef struct wmx_pkgfifo wmx_pkgfifo;
int wmx_pkgfifo_create(wmx_pkgfifo **out, int n_streams, int n_slots, int pkg_bytes, int interval_ms, int frame_bytes);
int wmx_pkgfifo_destroy(wmx_pkgfifo *h);
int wmx_pkgfifo_add(wmx_pkgfifo *h, const uint8_t *d_pkgs, long stride, void *stream);
int wmx_pkgfifo_get(wmx_pkgfifo *h, uint8_t *d_out, long stride, int delayms, void *stream);

/* ------------------------------------------------------------------ the daemon's tick: play package + record heartbeat
 * With WMIX_RECORD_PLAY_SYNC (src/wmixConf.h:144) the play thread does, per package of WMIX_INTERVAL_MS: drain the ring head
 * (src/wmix.c:1347-1366) -> playPkgBuff_add (:1419, :480-491) -> wmix_ao_write -> wmix_shmem_write_circle (:1439): ns_process ->
 * aec_process2(playPkgBuff_get(AEC_INTERVALMS), ..) -> agc_process -> vad_process on the captured package (:613-709) ->
 * wmix_pcm_zoom to 1 x 8000 (:730); the task threads feed the ring with wmix_load_data.  wmx_tick is n_groups such daemons side by
 * side: one ring, one FIFO row and one far-end per mix group, rec_per_group record streams per group (rows g * R .. g * R + R - 1)
 * whose echo canceller hears THAT group's playback, aec_delay_ms (= AEC_INTERVALMS, platform/alsa/plat.h:52: 400) late.  One mix
 * group = one control cohort with a far-end of its own.  chn / freq: the ring's and the capture's format (WMIX_CHN / WMIX_FREQ);
 * stages: WMX_CHAIN_* bits of the heartbeat.
 *   wmx_tick_load: this tick's wmix_load_data calls (= wmx_mix_load on the tick's mixer; same arguments and cursor rule).
 *   wmx_tick_play: the play side of one package.  d_play (may be NULL): n_groups rows, play_stride int16 apart <- what goes to the
 *                  sound card; the far-end package of every group (playPkgBuff_get) is left in wmx_tick_far(h): [n_groups][package]
 *                  int16 on the device.
 *   wmx_tick_record: the record side (the heartbeat).  d_rec: n_groups * rec_per_group rows of one package, rec_stride apart:
 *                  captured audio in, the chain's output out (in place, like the daemon's buffSrc).  d_rec_1x8000 (may be NULL):
 *                  rows of out_capacity bytes, out_stride int16 apart <- wmix_pcm_zoom(.., 1, 8000); *out_len = bytes per row.
 *   wmx_tick_run:  both, for audio captured beforehand (the daemon reads the capture between the two, src/wmix.c:609). */
typedef struct wmx_tick wmx_tick;
int wmx_tick_create(wmx_tick **out, int n_groups, int rec_per_group, int chn, int freq, int interval_ms, int aec_delay_ms, int agc_value,
                    unsigned stages);
int wmx_tick_destroy(wmx_tick *h);
/* the heartbeat's switches at run time (wmx_chain_set_stages on the tick's chain): the reference SHIPS with NS = 1, AGC = 1, VAD = 0,
 * AEC = 0 (src/wmix.c:1580-1584) and its message thread turns them (:1010-1050); a canceller that comes on hears one far-end per mix
 * group; 0 = a pure mix / FIFO / zoom tick */
int wmx_tick_set_stages(wmx_tick *h, unsigned stages, int agc_value);
/* webrtcEnable[WR_NS_PA] (src/wmix.c:1370-1386): on = 1 puts ns_process over the played package, in front of playPkgBuff_add (ns_init of
 * one suppressor per group now); on = 0 releases it */
int wmx_tick_play_ns(wmx_tick *h, int on);
/* wmix->rwTest (src/wmix.c:714-732), the self send-receive test: while on, wmx_tick_record loads the chain's output of each group's
 * first record stream back into the group's play ring (wmix_load_data with the heartbeat's own cursor, reduce 1) before the zoom;
 * switching it off forgets the cursor (:728-732) */
int wmx_tick_rw_test(wmx_tick *h, int on);
/* The conference bridge.  parties >= 2: the tick's groups are n_groups / parties conferences of call legs (needs rec_per_group == 1,
 * n_groups % parties == 0, rwTest off; else WMX_EINVAL).  While on, wmx_tick_record loads the chain's output of every participant
 * into the rings of the OTHER participants of its conference (wmx_mix_load_minus with a cursor of the bridge's own, reduce 1) before
 * the zoom -- the place and the arguments of the rwTest load (src/wmix.c:716-726) -- so participant q is played everybody except
 * themself, and the echo canceller of leg q is given exactly what leg q was played.  parties == 0: off, the cursor is forgotten.
 * wmx_tick_rw_test(h, 1) while the bridge is on returns WMX_EINVAL. */
int wmx_tick_bridge(wmx_tick *h, int parties);
/* host_mask: n_groups bytes, non-zero = that participant is muted (loaded nowhere, still hears the others); NULL = nobody.  Copied
 * into a buffer the handle owns, on `stream`. */
int wmx_tick_bridge_mute(wmx_tick *h, const uint8_t *host_mask, void *stream);
/* The bridge with conferences of different sizes whose legs join and leave: the layout of wmx_mix_set_conferences over the tick's
 * groups (needs rec_per_group == 1).  Called between ticks, it replaces the layout; while one is in force wmx_tick_record calls
 * wmx_mix_load_minus_conf where wmx_tick_bridge calls wmx_mix_load_minus.  Conference identity is the index c and the handle keeps
 * (head[c], tick[c]) across the change: a conference that had 2 or more members and still has keeps its cursor, any other starts from
 * a fresh one when it next loads.  A leg's ring, FIFO row and chain state are never touched; fresh NS / AEC / AGC / VAD handles for a
 * new call in a slot are wmx_chain_reset_streams' business (wmx_tick_chain).  n_conf == 0 switches it off and forgets every cursor.
 * wmx_tick_bridge_mute works unchanged (the mask is by ring).  It excludes wmx_tick_rw_test(h, 1) and wmx_tick_bridge(h, parties > 0),
 * and each of them excludes it: WMX_EINVAL. */
int wmx_tick_bridge_conferences(wmx_tick *h, int n_conf, const int32_t *host_off, const int32_t *host_members, void *stream);
/* Talker selection in the tick (wmx_mix_select_speakers / _conf on the tick's mixer).  May be called at any time and takes effect while
 * either bridge form is on: wmx_tick_record then runs the selection on the chain's output, between the chain and the bridge load, with
 * the mask of wmx_tick_bridge_mute as the host's mute and a mask buffer of the tick's own as the load's d_mute.  max_speakers == 0
 * (the default) switches it off: the tick's launches are then what they are without it.  Switching off does not clear env; a new call
 * in a reused slot clears its own with wmx_mix_reset_speakers(wmx_tick_mix(h), ..), next to its wmx_chain_reset_streams.
 * WMX_EINVAL: max_speakers outside 0 .. WMX_MIX_MAX_PARTIES, decay_shift outside 0 .. 31.
 * wmx_tick_bridge_speaking: who was speaking in the last tick and every ring's envelope (wmx_mix_export_speakers; n_groups entries
 * each, either may be NULL; blocking). */
int wmx_tick_bridge_speakers(wmx_tick *h, int max_speakers, uint32_t floor, int decay_shift);
int wmx_tick_bridge_speaking(wmx_tick *h, uint8_t *host_speaking, uint32_t *host_env, void *stream);
/* the daemon of another platform directory: PLAT_AEC_INTERVALMS (alsa 400, hi3516 700, t31 0; plat.h:14/19) is wmx_tick_create's
 * aec_delay_ms -- the FIFO gets AEC_FIFO_PKG_NUM = aec_delay_ms / interval_ms + 2 slots (src/wmixConf.h:141) -- and PLAT_PLAY_CORRECT is
 * set here (wmx_mix_set_play_correct on the tick's rings; default platform/alsa's) */
int wmx_tick_set_play_correct(wmx_tick *h, uint32_t bytes);
int wmx_tick_package_samples(const wmx_tick *h); /* int16 elements of one package of one stream = WMIX_PKG_SIZE / 2 */
int wmx_tick_load(wmx_tick *h, const int16_t *d_src, uint32_t srcU8Len, int freq, int channels, int sample, int n_src, long group_stride,
                  long source_stride, int reduce, uint32_t *head, uint32_t *tick, void *stream);
int wmx_tick_play(wmx_tick *h, int16_t *d_play, long play_stride, void *stream);
const int16_t *wmx_tick_far(const wmx_tick *h);
int wmx_tick_record(wmx_tick *h, int16_t *d_rec, long rec_stride, int16_t *d_rec_1x8000, long out_stride, uint32_t out_capacity,
                    uint32_t *out_len, void *stream);
int wmx_tick_run(wmx_tick *h, int16_t *d_play, long play_stride, int16_t *d_rec, long rec_stride, int16_t *d_rec_1x8000, long out_stride,
                 uint32_t out_capacity, uint32_t *out_len, void *stream);
wmx_mix *wmx_tick_mix(wmx_tick *h);
wmx_chain *wmx_tick_chain(wmx_tick *h);
wmx_pkgfifo *wmx_tick_fifo(wmx_tick *h);

/* Developer / test hook: the cross-lane FFT executors of the kernels, stand-alone, one transform per wavefront, in place
 * (wmix_amd/csrc/fft_debug.hip lists the kinds: Ooura rdft 128 / 256 through the LDS executor, aec_rdft_128 through the LDS,
 * 16-lane-register and one-point-per-lane executors, the SPL fixed-point real FFT of orders 7 and 8).  The SPL kinds, on
 * [n_batch][n + 2] int16: 8 / 9 forward / inverse of order 7 and 10 / 11 of order 8 through the register executors the product
 * kernels run (spl_cfft128, spl_cfft256); 12 / 13 order 8 through the generic LDS executor spl_cfft, kept as their cross-check.
 * The inverse kinds 9, 11 and 13 write the transform's scale count to d_aux[n_batch]. */
int wmx_debug_fft(int kind, int n_batch, void *d_data, int32_t *d_aux, void *stream);
/* Developer / test hook: the fixed-point primitives of the VAD, AGC, NSX and AECM kernels (wmix_amd/csrc/spl_dev.h, spl_fx.h) on the
 * device (device pointers to n int32 each; synchronises `stream`), y[i] = f(a[i], b[i], c[i]).  The int32 operands are narrowed the
 * way the callee's parameter does (the low bits are kept); operands a kind does not take are not read and may be NULL.
 *   0 norm_w16(a)   1 norm_w32(a)   2 norm_u32(a)   3 size_in_bits(a)   4 div_w32_w16(a, b)   5 div_u32_u16(a, b)
 *   6 sqrt_floor(a)   7 spl_sqrt(a)   8 mul_rsft_round(a, b, c) with c in 1 .. 31   9 agc_scalediff32(a, b, c)   10 agc_mul32(a, b)
 *   11 spl_scalediff32(a, b, c)   12 pk_abs16(a)   13 pk_max_u16(a, b)
 * Wave reductions, d_a and d_y [n / 64][64] with n a multiple of 64, one wavefront per row, every lane storing what it holds:
 *   16 wave_sum   17 wave_max   18 wave_min   19 wave_umax   20 wave_umin
 * WMX_EINVAL: any other kind, a NULL operand the kind takes, n not a multiple of 64 for a wave kind. */
int wmx_debug_spl(int kind, const int32_t *d_a, const int32_t *d_b, const int32_t *d_c, int32_t *d_y, size_t n, void *stream);
/* Developer / test hook: the NS kernels' table-driven log (kind 0, x >= 1), exp (kind 1) and tanh (kind 2) evaluated on the host
 * from the same source (wmix_amd/csrc/libm_dev.h), for sweeping against libm without a GPU. */
int wmx_debug_ns_libm(int kind, const float *x, float *y, size_t n);
/* ... and on the device (device pointers; synchronises `stream`), with the tables in LDS as the kernels hold them.  kind 0 .. 2 as
 * above (arguments outside a routine's guard take the library routine behind it), 3: exp in double, rounded to float, 4:
 * x / pow(a, b) in double, rounded to float (d_a, d_b are read for this kind only and may be NULL otherwise), 5: sqrtf. */
int wmx_debug_ns_libm_device(int kind, const float *d_x, const float *d_a, const float *d_b, float *d_y, size_t n, void *stream);
/* ... and the double that kinds 0 .. 2 hold before they round it to float (kind 2: of |x|), on the host and on the device; NaN for an
 * argument outside the routine's guard.  Host and device run the same IEEE operations: the doubles are equal bit for bit. */
int wmx_debug_ns_libm_dbl(int kind, const float *x, double *y, size_t n);
int wmx_debug_ns_libm_dbl_device(int kind, const float *d_x, double *d_y, size_t n, void *stream);
/* Developer / test hook: the library routines of the AEC kernels on the device (device pointers; synchronises `stream`).
 * kind 0: log in double, rounded to float, 1: sqrtf. */
int wmx_debug_aec_libm_device(int kind, const float *d_x, float *d_y, size_t n, void *stream);
/* Developer / test hook: the float NS kernel's analysis window for L = 128 (8 kHz) or 256 (16 / 32 kHz) as its constants block holds
 * it, L floats to a HOST buffer; needs no device. */
int wmx_debug_ns_window(int L, float *host_window);
/* Developer / test hook: the NS kernels' division for ordinary operands (wmix_amd/csrc/libm_dev.h div_ordinary: the
 * compiler's own fp32 division sequence without its rescaling and special-case instructions) beside `a / b`, on the device
 * (device pointers) and compiled for the host. */
int wmx_debug_div(const float *d_a, const float *d_b, float *d_q_ordinary, float *d_q_ieee, size_t n, void *stream);
int wmx_debug_div_host(const float *a, const float *b, float *q, size_t n);
/* Developer / test hook: the gate of the float AEC's near kernel that settles the two decisions taken from sdSum and seSum
 * (divergeState, filter reset) from lane-parallel sums where the order of the additions cannot matter (wmix_amd/csrc/aec_gate.h).
 * sd_rows, se_rows: [n][65] floats, prev_state: [n] divergeState in front of the block, out: [n][4] int32.  On the host:
 * {decided, diverge, reset, 0} (diverge and reset mean nothing where decided is 0); on the device (device pointers; synchronises
 * `stream`), one wave per row with the kernel's reduction and, for an undecided row, its ordered sums: {1 = settled by the gate /
 * 0 = by the ordered sums, diverge, reset, 0}, final for every row. */
int wmx_debug_aec_decide(const float *sd_rows, const float *se_rows, const int32_t *prev_state, int32_t *out, size_t n);
int wmx_debug_aec_decide_device(const float *d_sd_rows, const float *d_se_rows, const int32_t *d_prev_state, int32_t *d_out, size_t n, void *stream);
/* Same for the AEC kernel's table-driven powf: y[i] = x[i] ^ e[i]. */
int wmx_debug_pow(const float *x, const float *e, float *y, size_t n);
/* ... and evaluated on the device (device pointers; synchronises `stream`) */
int wmx_debug_pow_device(const float *d_x, const float *d_e, float *d_y, size_t n, void *stream);
/* Developer / test hook: the lane-mask constants the wave-per-stream kernels test instead of comparing the lane id
 * (wmix_amd/csrc/lane_sites.h).  wmx_debug_lane_sites(): how many there are; wmx_debug_lane_site_name(site): the name of one (NULL
 * outside the list).  wmx_debug_lane_masks launches ONE workgroup of block_threads threads (a multiple of 64, at most 1024) and
 * writes d_out[site][thread] (device pointer, sites x block_threads int32; synchronises `stream`): bit 0 = the mask says the
 * thread's lane is selected, bit 1 = the arithmetic predicate of the lane id says so.  Only the lanes whose bit is set in
 * diverge_mask evaluate and store (inside a divergent branch); all ones: every lane, no branch. */
int wmx_debug_lane_sites(void);
const char *wmx_debug_lane_site_name(int site);
int wmx_debug_lane_masks(int block_threads, uint64_t diverge_mask, int32_t *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WMIX_AMD_H */
