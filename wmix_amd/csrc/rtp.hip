// rtp.hip -- the RTP / G.711 packet edge of the hot path, batched for gfx950.
//
// Egress replaces, for n streams per launch, the loop body of wmix_thread_rtp_send_pcma (src/wmixTask.c:1124-1143):
//   wmix_pcm_zoom (src/wmix.c:139-222) -> PCM2G711a (src/g711codec.c:227-247) -> header.timestamp += codes / chn ->
//   rtp_send's network-order header (src/rtp.c:35-70, layout src/rtp.h:37-75) -> header.seq++
// as ONE kernel: the PCM a stream produced is read once and what leaves is the datagram (12 + 160 bytes for the
// reference's 20 ms of 8 kHz A-law), so 172 B per stream per packet cross PCIe instead of 320 B of PCM plus a host
// encode.  Ingest replaces rtp_recv's payload-size rule + G711a2PCM (src/rtp.c:86-95, src/wmixTask.c:1278-1282).
// The zoom's float32 phase walk is data independent and runs once per call on the host (mix.hip) -- the kernel
// gathers through the list.  Integer path: bit-exact.
#include <vector>
#include "wmx_internal.h"
#include "g711_dev.h"
#include "leg_calls.h"
#include "leg_seq.h"
#include "leg_plc.h"
#include "leg_codec.h"
#include "leg_dtmf.h"
#include "leg_record.h"
#include "leg_state.h"

struct wmx_rtp {
    int device;  // the HIP device the state lives on (current device at create); every entry point switches to it
    int n_streams, law;
    wmx::SchedCache sched;  // gather list per egress format, never rewritten (see SchedCache)
    std::vector<int32_t> idx;
    wmx::LegState send;   // per stream, made by create: sequence number (low 16 bits significant), timestamp
    wmx::LegState seq;    // the sequence rule (leg_seq.h): synced, next, lost, late, dup, resync, overflow, uint32 each
    wmx::LegState codec;  // the codec rule (leg_codec.h): refused (uint32), in_codec and out_law (uint8)
    wmx::LegState plc;    // the concealment rule (leg_plc.h): hist (kPlcHist int16), concealed (uint32)
    wmx::LegState dtmf;   // the DTMF rule (leg_dtmf.h): ring (uint64), count, ts and flags (uint32 each)
    // no stream has left in_codec REFERENCE / out_law = law, so the launches are those of a handle that knows no codecs
    bool codecs_default;
    // the recording taps (leg_record.h), made once by wmx_rtp_recorders: the taps' state on the device with the store's gather list
    // behind it (one block), and the host's copy of the state, stepped beside every launch: the rule reads nothing the device computes
    wmx::LegRecord *d_rec = nullptr;
    const int32_t *d_rec_idx = nullptr;
    std::vector<wmx::LegRecord> rec;
    int rec_chn = 0, rec_freq = 0, rec_mode = 0;
    uint32_t rec_row = 0;  // the samples of a row: what the zoom writes for one package
};

namespace wmx {
namespace {

constexpr int kRtpHeader = 12;      // RTP_HEADER_SIZE, src/rtp.h:33
constexpr int kRtpG711Payload = 160;  // RTP_PCMA_PKT_SIZE, src/rtp.h:31
static_assert(kLegRow == kRtpG711Payload, "a leg's row is one datagram's payload decoded");
static_assert(kLegMaxCalls == WMX_MIX_MAX_LEG_PACKETS, "leg_calls.h and include/wmix_amd.h name one limit");

// LAW: WMX_LAW_A / WMX_LAW_U for every stream of the launch (payload type `pt`), or kLawPerStream: laws[stream] (leg_codec.h)
constexpr int kLawPerStream = 2;
template <int LAW>
__device__ __forceinline__ uint32_t enc_law(int law, int v) {
    if (LAW == WMX_LAW_A) return enc_alaw(v);
    if (LAW == WMX_LAW_U) return enc_ulaw(v);
    return law == WMX_LAW_A ? enc_alaw(v) : enc_ulaw(v);
}

// The first two words of rtp_send's network-order header (src/rtp.c:35-70) as a little-endian machine stores them: v = 2, p = x = 0,
// cc = 0 | m = 1, pt | seq, timestamp big endian on the wire.  The third word, ssrc, is 0 (src/wmixTask.c:1058).
__device__ __forceinline__ uint2 rtp_header_words(uint32_t pt, uint32_t sq, uint32_t tt) {
    return make_uint2((2u << 6) | ((0x80u | pt) << 8) | ((sq >> 8) << 16) | ((sq & 0xFFu) << 24),
                      (tt >> 24) | (((tt >> 16) & 0xFFu) << 8) | (((tt >> 8) & 0xFFu) << 16) | ((tt & 0xFFu) << 24));
}

// the four codes of one payload word decoded to four samples, the first in the low half of x
template <class Dec>
__device__ __forceinline__ uint2 dec4(uint32_t w, const Dec &dec) {
    return make_uint2(((uint32_t)dec(w & 0xFF) & 0xFFFFu) | ((uint32_t)dec((w >> 8) & 0xFF) << 16),
                      ((uint32_t)dec((w >> 16) & 0xFF) & 0xFFFFu) | ((uint32_t)dec(w >> 24) << 16));
}

template <int LAW>
__global__ void rtp_egress_kernel(const int16_t *__restrict__ pcm, long pcm_stride, const int32_t *__restrict__ idx, int n_codes,
                                  int codes_per_ts, uint32_t *seq, uint32_t *ts, uint8_t *packets, long packet_stride, int n_streams,
                                  int pt, const uint8_t *__restrict__ laws) {
    const int stream = blockIdx.y;
    if (stream >= n_streams) return;
    const int law = LAW == kLawPerStream ? (int)laws[stream] : LAW;
    if (LAW == kLawPerStream) pt = (int)leg_codec_out_pt(law);
    const int16_t *src = pcm + (size_t)stream * pcm_stride;
    uint8_t *pkt = packets + (size_t)stream * packet_stride;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_codes; i += gridDim.x * blockDim.x)
        pkt[kRtpHeader + i] = (uint8_t)enc_law<LAW>(law, src[idx[i]]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t t = ts[stream] + (uint32_t)codes_per_ts;  // timestamp += ret / chn, before the send
        const uint32_t s = seq[stream] & 0xFFFFu;
        pkt[0] = 2u << 6;                 // v = 2, p = x = 0, cc = 0
        pkt[1] = (uint8_t)(0x80u | pt);   // m = 1
        pkt[2] = (uint8_t)(s >> 8);       // htons / htonl: big endian on the wire
        pkt[3] = (uint8_t)s;
        pkt[4] = (uint8_t)(t >> 24);
        pkt[5] = (uint8_t)(t >> 16);
        pkt[6] = (uint8_t)(t >> 8);
        pkt[7] = (uint8_t)t;
        pkt[8] = pkt[9] = pkt[10] = pkt[11] = 0;  // ssrc = 0 (src/wmixTask.c:1058)
        ts[stream] = t;
        seq[stream] = (s + 1) & 0xFFFFu;  // rtpHeader.seq++ after the send (uint16 wrap)
    }
}

__global__ void rtp_ingest_kernel(const uint8_t *__restrict__ packets, long packet_stride, int16_t *pcm, long pcm_stride, uint32_t *pcm_bytes,
                                  uint16_t *seq_raw, int n_streams) {
    const int stream = blockIdx.x;
    if (stream >= n_streams) return;
    const uint8_t *pkt = packets + (size_t)stream * packet_stride;
    const int pt = pkt[1] & 0x7F;
    const int size = (pt == 8 || pt == 0) ? kRtpG711Payload : 0;  // src/rtp.c:88-95 (AAC-tagged packets: not G.711, size 0 here)
    int16_t *dst = pcm + (size_t)stream * pcm_stride;
    for (int i = threadIdx.x; i < size; i += blockDim.x) dst[i] = (int16_t)dec_alaw(pkt[kRtpHeader + i]);  // G711a2PCM whatever the pt
    if (threadIdx.x == 0) {
        if (pcm_bytes) pcm_bytes[stream] = (uint32_t)size * 2;
        if (seq_raw) seq_raw[stream] = (uint16_t)(pkt[2] | (pkt[3] << 8));  // as stored: rtp_recv does not ntohs
    }
}

// ---- the same two kernels for the layouts the hosts use: packets and PCM rows on 4 / 8-byte boundaries.  One lane takes FOUR
// codes (one 32-bit word of payload, one 8-byte store of samples; or four gathered samples, one 32-bit store of codes), and
// the lanes are dealt over (stream, word) pairs instead of one workgroup per stream: 65 536 streams were 65 536 workgroups of
// 64 / 256 lanes moving one byte each (115 us for the ingest, 40 for the egress); now 1.3 M lanes of four codes.
constexpr int kRtpWords = kRtpG711Payload / 4;
__global__ __launch_bounds__(256) void rtp_ingest_wide_kernel(const uint8_t *__restrict__ packets, long packet_stride, int16_t *pcm,
                                                               long pcm_stride, uint32_t *pcm_bytes, uint16_t *seq_raw, int n_streams) {
    const size_t total = (size_t)n_streams * kRtpWords;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int stream = (int)(t / kRtpWords), c = (int)(t - (size_t)stream * kRtpWords);
        const uint8_t *pkt = packets + (size_t)stream * packet_stride;
        const uint32_t h0 = *reinterpret_cast<const uint32_t *>(pkt);  // bytes 0..3 of the header: flags, pt, seq as stored
        const int pt = (h0 >> 8) & 0x7F;
        const bool g711 = pt == 8 || pt == 0;  // src/rtp.c:88-95 (AAC-tagged packets: not G.711, size 0 here)
        if (g711) {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(pkt + kRtpHeader + 4 * c);
            // G711a2PCM whatever the pt
            *reinterpret_cast<uint2 *>(pcm + (size_t)stream * pcm_stride + 4 * c) = dec4(w, [](uint32_t code) { return dec_alaw(code); });
        }
        if (c == 0) {
            if (pcm_bytes) pcm_bytes[stream] = g711 ? (uint32_t)kRtpG711Payload * 2 : 0u;
            if (seq_raw) seq_raw[stream] = (uint16_t)(h0 >> 16);  // pkt[2] | pkt[3] << 8, as stored: rtp_recv does not ntohs
        }
    }
}

template <int LAW>
__global__ __launch_bounds__(256) void rtp_egress_wide_kernel(const int16_t *__restrict__ pcm, long pcm_stride, const int32_t *__restrict__ idx,
                                                               int n_codes, int codes_per_ts, uint32_t *seq, uint32_t *ts, uint8_t *packets,
                                                               long packet_stride, int n_streams, int pt_all,
                                                               const uint8_t *__restrict__ laws) {
    const int words = n_codes >> 2;  // n_codes is a multiple of 4 here
    const size_t total = (size_t)n_streams * words;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int stream = (int)(t / words), j = (int)(t - (size_t)stream * words);
        const int16_t *src = pcm + (size_t)stream * pcm_stride;
        uint8_t *pkt = packets + (size_t)stream * packet_stride;
        const int4 ix = *reinterpret_cast<const int4 *>(idx + 4 * j);
        const int law = LAW == kLawPerStream ? (int)laws[stream] : LAW;
        const int pt = LAW == kLawPerStream ? (int)leg_codec_out_pt(law) : pt_all;
        auto enc = [=](int v) -> uint32_t { return enc_law<LAW>(law, v); };
        *reinterpret_cast<uint32_t *>(pkt + kRtpHeader + 4 * j) =
            (enc(src[ix.x]) & 0xFF) | ((enc(src[ix.y]) & 0xFF) << 8) | ((enc(src[ix.z]) & 0xFF) << 16) | (enc(src[ix.w]) << 24);
        if (j == 0) {
            const uint32_t tt = ts[stream] + (uint32_t)codes_per_ts;  // timestamp += ret / chn, before the send
            const uint32_t sq = seq[stream] & 0xFFFFu;
            uint32_t *hd = reinterpret_cast<uint32_t *>(pkt);
            const uint2 hw = rtp_header_words((uint32_t)pt, sq, tt);
            hd[0] = hw.x, hd[1] = hw.y, hd[2] = 0;
            ts[stream] = tt;
            seq[stream] = (sq + 1) & 0xFFFFu;  // rtpHeader.seq++ after the send (uint16 wrap)
        }
    }
}

// Ingest for legs that deliver 0 .. max_packets datagrams in a tick (wmx_rtp_ingest_legs, wmx_rtp_ingest_legs_codecs):
// rtp_ingest_wide_kernel's four codes per lane (WIDE: rows on 4 / 8-byte boundaries) or one code per lane, dealt over (leg, slot,
// piece).  A slot where nothing arrived (recv_bytes <= 0: its datagram row is not read) or that the codec rule (leg_codec.h) refuses
// made no call: len 0 and a zeroed PCM row.  Which slots make a call and with which law their payload is decoded is the leg's in_codec's
// to say.  PER_LEG false: every leg is WMX_CODEC_REFERENCE (in_codec is not read) -- a G.711 payload type makes a call, decoded as
// A-law whatever the pt (src/rtp.c:88-95).  A row's lanes all decide alike from the row's header; neighbouring rows, and so the lanes
// of one wave, may decode with different laws: both decoders are evaluated and one is selected.  COUNT: refused[leg] counts the leg's
// slots where something arrived that made no call: one atomic add by the row's first lane -- up to max_packets lanes add to one word,
// and no lane of the launch reads it.  COUNT false (no handle, wmx_rtp_ingest_legs): refused is not touched.
template <bool WIDE, bool PER_LEG, bool COUNT>
__global__ __launch_bounds__(256) void rtp_ingest_legs_codecs_kernel(const uint8_t *__restrict__ packets, long leg_stride, long packet_stride,
                                                                      const int32_t *__restrict__ recv_bytes, int16_t *pcm, long source_stride,
                                                                      long pcm_packet_stride, uint32_t *len, uint16_t *seq_raw, int max_packets,
                                                                      int n_legs, const uint8_t *__restrict__ in_codec, uint32_t *refused) {
    constexpr int kPieces = WIDE ? kRtpWords : kRtpG711Payload;
    const size_t total = (size_t)n_legs * max_packets * kPieces;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t row = t / kPieces;  // leg * max_packets + slot
        const int c = (int)(t - row * kPieces);
        const size_t leg = row / (size_t)max_packets, k = row - leg * (size_t)max_packets;
        const uint8_t *pkt = packets + leg * leg_stride + k * packet_stride;
        int16_t *dst = pcm + leg * source_stride + k * pcm_packet_stride;
        const bool there = recv_bytes[row] > 0;
        const uint32_t pt = there ? pkt[1] & 0x7Fu : 0u;
        const uint32_t what = leg_codec_slot(there, pt, PER_LEG ? (uint32_t)in_codec[leg] : kCodecReference);
        const bool call = (what & kLegCodecCall) != 0u, ulaw = PER_LEG && (what & kLegCodecUlaw) != 0u;
        auto dec = [=](uint32_t code) -> uint32_t { return (uint32_t)(PER_LEG && ulaw ? dec_ulaw(code) : dec_alaw(code)); };
        if (WIDE) {
            uint2 o = make_uint2(0u, 0u);
            if (call) o = dec4(*reinterpret_cast<const uint32_t *>(pkt + kRtpHeader + 4 * c), dec);
            *reinterpret_cast<uint2 *>(dst + 4 * c) = o;
        } else {
            dst[c] = call ? (int16_t)dec(pkt[kRtpHeader + c]) : (int16_t)0;
        }
        if (c == 0) {
            len[row] = call ? kLegRowBytes : 0u;
            if (seq_raw) seq_raw[row] = there ? (uint16_t)(pkt[2] | (pkt[3] << 8)) : (uint16_t)0;  // as stored: rtp_recv does not ntohs
            if (COUNT && (what & kLegCodecRefused)) atomicAdd(refused + leg, 1u);
        }
    }
}

// Play and send in one kernel (wmx_rtp_egress_rings): what drain_kernel (mix.hip) followed by the egress kernels above do for a ring
// of 1 x 8000, where the zoom is the identity -- the 160 samples at the ring head never pass through a PCM row in HBM.  One lane takes
// FOUR codes, dealt over (ring, word) pairs.  WIDE_IN: the head is a multiple of four samples, so (the ring's length is one too) every
// lane's four samples are one aligned 8-byte piece that does not straddle the ring's end: one load, one store of zeros (the play thread
// zeroes what it has read, src/wmix.c:1351-1352).  Otherwise sample by sample, each reduced into the ring.  WIDE_OUT: datagram rows on
// 4-byte boundaries, the codes and the header as 32-bit stores; otherwise byte by byte.
// PER_RING: law and payload type are the ring's own (laws[ring], leg_codec.h).  A wave of 64 lanes spans more than one ring (40 words per
// ring), so its lanes may hold different laws: both encoders are evaluated and one is selected per lane; which lane writes the header
// (j == 0) does not depend on the law.
template <bool WIDE_IN, bool WIDE_OUT, bool PER_RING>
__global__ __launch_bounds__(256) void rtp_egress_rings_kernel(int16_t *__restrict__ rings, uint32_t ring_samples, uint32_t head_sample, int law_all,
                                                                uint32_t *seq, uint32_t *ts, uint8_t *__restrict__ packets, long packet_stride,
                                                                int n_rings, int pt_all, const uint8_t *__restrict__ laws) {
    const size_t total = (size_t)n_rings * kRtpWords;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int ring = (int)(t / kRtpWords), j = (int)(t - (size_t)ring * kRtpWords);
        int16_t *rg = rings + (size_t)ring * ring_samples;
        uint8_t *pkt = packets + (size_t)ring * packet_stride;
        const int law = PER_RING ? (int)laws[ring] : law_all;
        const int pt = PER_RING ? (int)leg_codec_out_pt(law) : pt_all;
        uint32_t pos = head_sample + 4u * (uint32_t)j;  // head_sample < ring_samples, 4 j < 160 <= ring_samples
        pos -= pos >= ring_samples ? ring_samples : 0u;
        int v[4];
        if (WIDE_IN) {
            uint2 *p = reinterpret_cast<uint2 *>(rg + pos);
            const uint2 x = *p;
            *p = make_uint2(0u, 0u);
            v[0] = (int16_t)(x.x & 0xFFFFu), v[1] = (int16_t)(x.x >> 16), v[2] = (int16_t)(x.y & 0xFFFFu), v[3] = (int16_t)(x.y >> 16);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                uint32_t q = pos + (uint32_t)i;
                q -= q >= ring_samples ? ring_samples : 0u;
                v[i] = rg[q];
                rg[q] = 0;
            }
        }
        uint32_t c[4];
#pragma unroll
        for (int i = 0; i < 4; i++) c[i] = (uint32_t)(law == WMX_LAW_A ? enc_alaw(v[i]) : enc_ulaw(v[i])) & 0xFFu;
        if (WIDE_OUT) {
            *reinterpret_cast<uint32_t *>(pkt + kRtpHeader + 4 * j) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) pkt[kRtpHeader + 4 * j + i] = (uint8_t)c[i];
        }
        if (j == 0) {
            const uint32_t tt = ts[ring] + (uint32_t)kRtpG711Payload;  // timestamp += ret / chn, before the send
            const uint32_t sq = seq[ring] & 0xFFFFu;
            const uint2 hw = rtp_header_words((uint32_t)pt, sq, tt);
            const uint32_t h0 = hw.x, h1 = hw.y;
            if (WIDE_OUT) {
                uint32_t *hd = reinterpret_cast<uint32_t *>(pkt);
                hd[0] = h0, hd[1] = h1, hd[2] = 0;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) pkt[i] = (uint8_t)(h0 >> (8 * i)), pkt[4 + i] = (uint8_t)(h1 >> (8 * i)), pkt[8 + i] = 0;
            }
            ts[ring] = tt;
            seq[ring] = (sq + 1) & 0xFFFFu;  // rtpHeader.seq++ after the send (uint16 wrap)
        }
    }
}

// The recording taps (wmx_rtp_record_rings, leg_record.h): in front of the kernel above, what it is about to play, as PCM in the
// store's format.  One wave = one tap, no loop over taps: the state entry is read before anything is stored, so it is a wave-uniform
// (scalar) load, the rule is evaluated once on the scalar side, and a free tap's wave leaves behind its one store of -1.  The ring is
// read and NOT zeroed: the egress still has to play it.  The host has checked that the head is a multiple of 160 samples and the ring a
// multiple of 160 long, so the row's 160 samples lie in one piece from a 16-byte boundary on; a leg index read from memory never
// addresses anything as it is: it is held against n_rings, and a gather index against the package.
// MODE kRecIdentity (1 x 8000): 20 lanes move 16 bytes each.  kRecDouble (2 x 8000, the zoom's 1 -> 2 duplication): 40 lanes load four
// samples and store them twice over, 16 bytes.  kRecGather: every other format, and rows that are not on 16-byte boundaries, sample by
// sample through the store's list (zoom_gather_list).
enum { kRecGather, kRecIdentity, kRecDouble };
template <int MODE>
__global__ __launch_bounds__(256) void rtp_record_rings_kernel(const int16_t *__restrict__ rings, uint32_t ring_samples, uint32_t head_sample,
                                                                LegRecord *__restrict__ state, const int32_t *__restrict__ idx, uint32_t row_samples,
                                                                int16_t *__restrict__ rows, long row_stride, int32_t *__restrict__ legs, int n_taps,
                                                                int n_rings) {
    const uint32_t lane = threadIdx.x & 63u;
    const int tap = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    if (tap >= n_taps) return;
    LegRecord r = state[tap];
    const int32_t leg = leg_record_tick(r);
    const bool known = leg >= 0 && leg < n_rings;  // a leg the mixer does not have writes no row, and its tap runs out all the same
    if (lane == 0u) legs[tap] = known ? leg : -1;
    if (leg < 0) return;
    if (known) {
        const int16_t *src = rings + (size_t)leg * ring_samples + head_sample;  // head_sample + 160 <= ring_samples
        int16_t *dst = rows + (size_t)tap * row_stride;
        if (MODE == kRecIdentity) {
            if (lane < (uint32_t)kRecordRowIn / 8u) reinterpret_cast<uint4 *>(dst)[lane] = reinterpret_cast<const uint4 *>(src)[lane];
        } else if (MODE == kRecDouble) {
            if (lane < (uint32_t)kRecordRowIn / 4u) {
                const uint2 x = reinterpret_cast<const uint2 *>(src)[lane];
                const uint32_t a = x.x & 0xFFFFu, b = x.x >> 16, c = x.y & 0xFFFFu, d = x.y >> 16;
                reinterpret_cast<uint4 *>(dst)[lane] = make_uint4(a | (a << 16), b | (b << 16), c | (c << 16), d | (d << 16));
            }
        } else {
            for (uint32_t i = lane; i < row_samples; i += 64u) {
                const uint32_t from = (uint32_t)idx[i];
                dst[i] = src[from < (uint32_t)kRecordRowIn ? from : (uint32_t)kRecordRowIn - 1u];
            }
        }
    }
    if (lane == 0u) state[tap] = r;
}

// start, stop and reset: one tap's entry
__global__ void rtp_record_set_kernel(LegRecord *__restrict__ state, int tap, LegRecord value) {
    if (blockIdx.x == 0 && threadIdx.x == 0) state[tap] = value;
}

// What a leg was sent, as its phone's speaker plays it (wmx_rtp_decode_sent_legs): the 160 codes of the leg's outgoing datagram decoded
// with the law they were encoded in -- the leg's own out_law once a stream has left the default (laws), else the handle's.  One lane
// per sample; the far end of the leg's echo canceller (aecm.hip, aecm_legs_kernel).
__global__ __launch_bounds__(256) void rtp_decode_sent_legs_kernel(const uint8_t *__restrict__ packets, long packet_stride, int16_t *__restrict__ pcm,
                                                                    long pcm_leg_stride, int n_legs, int law_all, const uint8_t *__restrict__ laws) {
    const size_t total = (size_t)n_legs * kRtpG711Payload;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t leg = t / kRtpG711Payload;
        const int c = (int)(t - leg * kRtpG711Payload);
        const int law = laws ? (int)laws[leg] : law_all;
        const uint32_t code = packets[leg * (size_t)packet_stride + kRtpHeader + c];
        pcm[leg * (size_t)pcm_leg_stride + c] = (int16_t)(law == WMX_LAW_A ? dec_alaw(code) : dec_ulaw(code));
    }
}

// The sequence rule (leg_seq.h) for every leg, one lane per leg: the lane reads its leg's up to four slots (d_len: which are calls;
// d_seq_raw: header bytes 2..3 as stored, swapped here), sorts the candidates' keys in registers, walks them, writes the call list,
// zeroes d_len of the slots that make no call and stores the state it read.  WIDE: max_packets == 4 and d_seq_raw on an 8-byte
// boundary -- the four sequence numbers are one 8-byte load.  No lane touches another leg's words: no atomics.
template <bool WIDE>
__global__ __launch_bounds__(256) void rtp_sequence_legs_kernel(const uint16_t *__restrict__ seq_raw, uint32_t *__restrict__ len,
                                                                 uint32_t *__restrict__ calls, uint32_t *__restrict__ sq, int max_packets,
                                                                 uint32_t max_gap, int n_legs) {
    const size_t n = (size_t)n_legs;
    for (size_t leg = blockIdx.x * (size_t)blockDim.x + threadIdx.x; leg < n; leg += (size_t)gridDim.x * blockDim.x) {
        uint32_t raw[kLegMaxCalls] = {0u, 0u, 0u, 0u}, ok = 0;
        if (WIDE) {
            const uint2 w = *reinterpret_cast<const uint2 *>(seq_raw + leg * kLegMaxCalls);
            raw[0] = w.x & 0xFFFFu, raw[1] = w.x >> 16, raw[2] = w.y & 0xFFFFu, raw[3] = w.y >> 16;
        }
#pragma unroll
        for (int k = 0; k < kLegMaxCalls; k++) {
            if (k >= max_packets) continue;
            if (!WIDE) raw[k] = seq_raw[leg * (size_t)max_packets + k];
            ok |= leg_row_readable(len[leg * (size_t)max_packets + k]) << k;
        }
        if (!ok) {  // no calls, state unchanged
            calls[leg] = 0u;
            continue;
        }
        uint32_t seq[kLegMaxCalls];
#pragma unroll
        for (int k = 0; k < kLegMaxCalls; k++) seq[k] = ((raw[k] & 0xFFu) << 8) | ((raw[k] >> 8) & 0xFFu);  // ntohs
        LegSeqState st{sq[leg], sq[n + leg], sq[2 * n + leg], sq[3 * n + leg], sq[4 * n + leg], sq[5 * n + leg], sq[6 * n + leg]};
        const LegSeqState was = st;
        const LegSeqTick r = leg_seq_tick(st, seq, ok, max_gap);
        calls[leg] = r.calls;
#pragma unroll
        for (int k = 0; k < kLegMaxCalls; k++)
            if (k < max_packets && ((r.discard >> k) & 1u)) len[leg * (size_t)max_packets + k] = 0u;
        sq[leg] = st.synced;
        sq[n + leg] = st.next;
        if (st.lost != was.lost) sq[2 * n + leg] = st.lost;
        if (st.late != was.late) sq[3 * n + leg] = st.late;
        if (st.dup != was.dup) sq[4 * n + leg] = st.dup;
        if (st.resync != was.resync) sq[5 * n + leg] = st.resync;
        if (st.overflow != was.overflow) sq[6 * n + leg] = st.overflow;
    }
}

// ---- the concealment rule (leg_plc.h) for every leg: ONE WAVE PER LEG, kPlcLegsPerBlock legs per block; no wave waits for another.
// A leg whose list holds no silence call takes a wave-uniform early path: its rows are copied to the repaired rows in call order and
// the history becomes the last 320 samples emitted, registers only.  Otherwise the wave lays a TIMELINE into LDS -- the history, then
// every call's emitted row behind it -- so that the history in front of call j is timeline[160 j .. 160 j + 320) and nothing is ever
// rolled.  At the start of a run q = h0 >> 4 goes to LDS, lane l scores lag 40 + l and (l < 17) lag 104 + l with 160 multiply-adds
// each -- q[i] is one address for the wave, q[i - L] one int16 per lane, descending: no bank conflict -- and six xor steps find the
// arg-max, ties to the smaller lag.  All 64 lanes then synthesise (and blend) two samples each per pass.  Per leg 1920 + 640 bytes of
// LDS.  Samples move in pairs: WIDE (rows in and out on 4-byte boundaries) one 32-bit access per pair, otherwise two 16-bit ones; the
// handle's history and the LDS are always 32-bit.  A lane writes only its own leg's rows, history and counter: no atomics.
constexpr int kPlcLegsPerBlock = 4;
constexpr int kPlcPairs = kLegRow / 2, kPlcHistPairs = kPlcHist / 2;
constexpr int kPlcTimeline = kPlcHist + kLegMaxCalls * kLegRow;

// two samples of a row as one word (the concealment and the DTMF kernel): WIDE one 32-bit access, otherwise two 16-bit ones
template <bool WIDE>
__device__ __forceinline__ uint32_t pair_load(const int16_t *p, int pair) {
    if (WIDE) return *reinterpret_cast<const uint32_t *>(p + 2 * pair);
    return (uint32_t)(uint16_t)p[2 * pair] | ((uint32_t)(uint16_t)p[2 * pair + 1] << 16);
}
template <bool WIDE>
__device__ __forceinline__ void pair_store(int16_t *p, int pair, uint32_t v) {
    if (WIDE) {
        *reinterpret_cast<uint32_t *>(p + 2 * pair) = v;
    } else {
        p[2 * pair] = (int16_t)(v & 0xFFFFu);
        p[2 * pair + 1] = (int16_t)(v >> 16);
    }
}
__device__ __forceinline__ uint32_t pair_pack(int32_t lo, int32_t hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }

template <bool WIDE>
__global__ __launch_bounds__(64 * kPlcLegsPerBlock) void rtp_conceal_legs_kernel(const int16_t *__restrict__ pcm, long source_stride,
                                                                                  long packet_stride, const uint32_t *__restrict__ len,
                                                                                  const uint32_t *__restrict__ calls_in, int max_packets,
                                                                                  int16_t *__restrict__ pcm_out, uint32_t *__restrict__ len_out,
                                                                                  int16_t *__restrict__ hist, uint32_t *__restrict__ concealed,
                                                                                  int n_legs) {
    __shared__ __attribute__((aligned(16))) int16_t timeline[kPlcLegsPerBlock][kPlcTimeline];
    __shared__ __attribute__((aligned(16))) int16_t qs[kPlcLegsPerBlock][kPlcHist];
    const int lane = (int)(threadIdx.x & 63u);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t leg = blockIdx.x * (size_t)kPlcLegsPerBlock + (size_t)w;
    if (leg >= (size_t)n_legs) return;  // the whole wave
    const uint32_t calls = (uint32_t)__builtin_amdgcn_readfirstlane((int)calls_in[leg]);
    const LegWalk walk = leg_calls_walk(len + leg * (size_t)max_packets, true, calls, max_packets);
    const uint32_t count = walk.count;
    // sil bit j: call j is filled from the history
    const uint32_t sil = ~(uint32_t)__builtin_amdgcn_readfirstlane((int)walk.data) & ((1u << count) - 1u);
    if (lane < kLegMaxCalls) len_out[leg * kLegMaxCalls + lane] = (uint32_t)lane < count ? kLegRowBytes : 0u;
    if (count == 0u) return;  // no calls: the state stays
    const int16_t *src = pcm + leg * source_stride;
    int16_t *dst = pcm_out + leg * (size_t)(kLegMaxCalls * kLegRow);
    int16_t *hs = hist + leg * (size_t)kPlcHist;
    const bool second = lane < kPlcPairs - 64;  // a row is 80 pairs: every lane one, the first 16 another

    if (sil == 0u) {  // data calls only
        if (count == 1u) {  // the older half of the history is its newer half; read and written by disjoint pairs
            const uint32_t a = pair_load<true>(hs, kPlcPairs + lane), b = second ? pair_load<true>(hs, kPlcPairs + 64 + lane) : 0u;
            pair_store<true>(hs, lane, a);
            if (second) pair_store<true>(hs, 64 + lane, b);
        }
        for (uint32_t j = 0; j < count; j++) {
            const int16_t *row = src + leg_calls_slot(calls, j) * packet_stride;
            const uint32_t a = pair_load<WIDE>(row, lane), b = second ? pair_load<WIDE>(row, 64 + lane) : 0u;
            pair_store<WIDE>(dst + j * kLegRow, lane, a);
            if (second) pair_store<WIDE>(dst + j * kLegRow, 64 + lane, b);
            if (j + 2u >= count) {  // one of the last two: it stays in the history
                int16_t *hrow = hs + (j + 2u - count) * kLegRow;
                pair_store<true>(hrow, lane, a);
                if (second) pair_store<true>(hrow, 64 + lane, b);
            }
        }
        return;
    }

    int16_t *tl = timeline[w], *q = qs[w];
    for (int p = lane; p < kPlcHistPairs; p += 64) pair_store<true>(tl, p, pair_load<true>(hs, p));
    const int16_t *h0 = tl;
    int32_t lag = kPlcLagMin, run = 0;
    uint32_t made = 0;
    for (uint32_t j = 0; j < count; j++) {
        int16_t *y = tl + kPlcHist + j * kLegRow, *out = dst + j * kLegRow;
        if ((sil >> j) & 1u) {
            if (run == 0) {
                h0 = tl + j * kLegRow;
                wave_sync();  // what the calls in front of this one appended
                for (int p = lane; p < kPlcHistPairs; p += 64) {
                    const uint32_t v = pair_load<true>(h0, p);
                    pair_store<true>(q, p, pair_pack(leg_plc_q((int16_t)(v & 0xFFFFu)), leg_plc_q((int16_t)(v >> 16))));
                }
                wave_sync();
                int32_t L = kPlcLagMin + lane, c = leg_plc_score(q, L);
                if (lane <= kPlcLagMax - kPlcLagMin - 64) {
                    const int32_t L2 = kPlcLagMin + 64 + lane, c2 = leg_plc_score(q, L2);
                    if (leg_plc_better(c2, L2, c, L)) c = c2, L = L2;
                }
                for (int o = 32; o > 0; o >>= 1) {
                    const int32_t c2 = __shfl_xor(c, o, 64), L2 = __shfl_xor(L, o, 64);
                    if (leg_plc_better(c2, L2, c, L)) c = c2, L = L2;
                }
                lag = __builtin_amdgcn_readfirstlane(L);
            }
            for (int p = lane; p < kPlcPairs; p += 64) {
                const int32_t k = run * kLegRow + 2 * p;
                const uint32_t v = pair_pack(leg_plc_synth(h0[leg_plc_index(k, lag)], k), leg_plc_synth(h0[leg_plc_index(k + 1, lag)], k + 1));
                pair_store<true>(y, p, v);
                pair_store<WIDE>(out, p, v);
            }
            run++;
            made++;
        } else {
            const int16_t *row = src + leg_calls_slot(calls, j) * packet_stride;
            for (int p = lane; p < kPlcPairs; p += 64) {
                uint32_t v = pair_load<WIDE>(row, p);
                if (run > 0 && 2 * p < kPlcBlend) {
                    const int32_t i = 2 * p, k = run * kLegRow + i;
                    v = pair_pack(leg_plc_blend((int16_t)(v & 0xFFFFu), leg_plc_synth(h0[leg_plc_index(k, lag)], k), i),
                                 leg_plc_blend((int16_t)(v >> 16), leg_plc_synth(h0[leg_plc_index(k + 1, lag)], k + 1), i + 1));
                }
                pair_store<true>(y, p, v);
                pair_store<WIDE>(out, p, v);
            }
            run = 0;
        }
    }
    wave_sync();
    const int16_t *last = tl + count * kLegRow;  // the last 320 samples emitted
    for (int p = lane; p < kPlcHistPairs; p += 64) pair_store<true>(hs, p, pair_load<true>(last, p));
    if (lane == 0) concealed[leg] += made;
}

// ---- the DTMF rule (leg_dtmf.h) for every leg: HALF A WAVE PER LEG, kDtmfLegsPerBlock legs per block; no lane waits for a lane of
// another wave.  A leg's up to four blocks times eight frequencies are 32 chains, one per lane: lane l of the leg's 32 runs frequency
// l & 7 over block l >> 3.  The leg's 32 lanes stage its readable rows into LDS pair by pair (WIDE: rows on 4-byte boundaries, one
// 32-bit load per pair; otherwise two 16-bit ones), then every chain walks its row two samples per 32-bit LDS read: the eight lanes
// of a block read one address (a broadcast), and rows are kDtmfLdsRow = 164 samples = 82 words apart, so the four blocks of a leg
// stand on banks 0, 18, 4 and 22 -- no two on one.  Every lane also sums the energy of the row it walks.  The eight powers of a block
// reach each of its lanes by cross-lane moves, each lane takes the header's decision, and the four decisions reach the leg's lanes
// the same way.  With suppress the leg's lanes zero the rows of the blocks that are tones.  The leg's first lane then reads the event
// packets' header bytes and walks the debounce over the decisions -- a short serial tail -- and stores the state it changed.  A lane
// writes only its own leg's rows and state: no atomics.  Per block of legs 8 x 4 x 328 bytes of LDS.
constexpr int kDtmfLegsPerBlock = 8;
constexpr int kDtmfLdsRow = 164;
constexpr int kDtmfPairs = kLegRow / 2;

__device__ __forceinline__ int64_t dtmf_shfl64(int64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v & 0xFFFFFFFFu), src, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), src, 64);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

template <bool WIDE>
__global__ __launch_bounds__(32 * kDtmfLegsPerBlock) void rtp_detect_dtmf_legs_kernel(const uint8_t *__restrict__ packets, long leg_stride,
                                                                                       long packet_stride, const int32_t *__restrict__ recv,
                                                                                       int16_t *pcm, long source_stride, long pcm_packet_stride,
                                                                                       const uint32_t *__restrict__ len,
                                                                                       const uint32_t *__restrict__ calls_in, int max_packets,
                                                                                       uint32_t event_pt, int suppress, uint64_t *ring,
                                                                                       uint32_t *count, uint32_t *ts, uint32_t *flags, int n_legs) {
    __shared__ __attribute__((aligned(16))) int16_t staged[kDtmfLegsPerBlock][kLegMaxCalls][kDtmfLdsRow];
    const int hl = (int)(threadIdx.x & 31u), half = (int)(threadIdx.x >> 5);
    const int wave_lane = (int)(threadIdx.x & 63u);
    const size_t leg = blockIdx.x * (size_t)kDtmfLegsPerBlock + (size_t)half;
    const bool live = leg < (size_t)n_legs;
    uint32_t list = 0, blocks = 0, quiet = (1u << kLegMaxCalls) - 1u;  // quiet bit j: block j is none, or not to be read
    if (live) {
        const LegWalk walk = leg_calls_walk_leg(len, calls_in, leg, max_packets);
        list = walk.list, blocks = walk.count, quiet &= ~walk.data;
    }
    int16_t *rows = pcm + (live ? leg : 0) * (size_t)source_stride;
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)kLegMaxCalls; j++) {
        if ((quiet >> j) & 1u) continue;
        const int16_t *row = rows + leg_calls_slot(list, j) * pcm_packet_stride;
        for (int p = hl; p < kDtmfPairs; p += 32) pair_store<true>(staged[half][j], p, pair_load<WIDE>(row, p));
    }
    wave_sync();  // a leg's lanes are lanes of one wave

    const int j = hl >> 3, f = hl & 7;
    const bool mine = !((quiet >> j) & 1u);
    int64_t power = 0, energy = 0;
    if (mine) {
        const int32_t coef = leg_dtmf_coef(f);
        const int16_t *x = staged[half][j];
        int32_t s1 = 0, s2 = 0;
        for (int p = 0; p < kDtmfPairs; p++) {
            const uint32_t v = pair_load<true>(x, p);
            const int32_t a = (int16_t)(v & 0xFFFFu), b = (int16_t)(v >> 16);
            leg_dtmf_step(s1, s2, coef, a);
            leg_dtmf_step(s1, s2, coef, b);
            energy = leg_dtmf_energy(leg_dtmf_energy(energy, a), b);
        }
        power = leg_dtmf_power(s1, s2, coef);
    }
    int64_t p8[kDtmfFreqs];
#pragma unroll
    for (int i = 0; i < kDtmfFreqs; i++) p8[i] = dtmf_shfl64(power, (wave_lane & ~7) + i);
    const int32_t digit = mine ? leg_dtmf_decide(p8, energy) : kDtmfNone;
    int32_t d[kLegMaxCalls];
#pragma unroll
    for (int i = 0; i < kLegMaxCalls; i++) d[i] = __shfl(digit, (wave_lane & 32) + 8 * i, 64);

    if (suppress) {
#pragma unroll
        for (uint32_t i = 0; i < (uint32_t)kLegMaxCalls; i++) {
            if (d[i] == kDtmfNone) continue;  // a tone: the leg is live and the block has a row
            int16_t *row = rows + leg_calls_slot(list, i) * pcm_packet_stride;
            for (int p = hl; p < kDtmfPairs; p += 32) pair_store<WIDE>(row, p, 0u);
        }
    }
    if (!live || hl != 0) return;
    LegDtmfState st{count[leg], ring[leg], ts[leg], flags[leg]};
    const LegDtmfState was = st;
#pragma unroll
    for (int k = 0; k < kLegMaxCalls; k++) {
        if (k >= max_packets) continue;
        const int32_t got = recv[leg * (size_t)max_packets + k];
        if (got < (int32_t)kDtmfMinEventBytes) continue;  // the row is read only where enough arrived
        const uint8_t *pkt = packets + leg * (size_t)leg_stride + (size_t)k * packet_stride;
        leg_dtmf_packet(st, got, pkt[1], pkt[12], leg_dtmf_word(pkt + 4), event_pt);
    }
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)kLegMaxCalls; i++)
        if (i < blocks) leg_dtmf_debounce(st, d[i]);
    if (st.count != was.count) count[leg] = st.count, ring[leg] = st.ring;
    if (st.ts != was.ts) ts[leg] = st.ts;
    if (st.flags != was.flags) flags[leg] = st.flags;
}

inline bool aligned_to(const void *p, long stride_bytes, int a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0 && stride_bytes % a == 0; }

}  // namespace
}  // namespace wmx

using namespace wmx;

// conf.hip's question in front of a tick: has it a tap that writes a row?  (the host's copy of leg_record.h's state: no download)
bool wmx::rtp_record_running(const wmx_rtp *h) { return h->d_rec && leg_record_any(h->rec.data(), (int)h->rec.size()); }

extern "C" {

int wmx_rtp_create(wmx_rtp **out, int n_streams, int law) {
    if (!out || n_streams < 1 || (law != WMX_LAW_A && law != WMX_LAW_U)) {
        set_error("wmx_rtp_create: n_streams %d, law %d", n_streams, law);
        return WMX_EINVAL;
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) {
        set_error("wmx_rtp_create: no HIP device");
        return WMX_ENODEV;
    }
    wmx_rtp *h = new wmx_rtp();
    if ((h->device = wmx::current_device()) < 0) {
        delete h;
        return WMX_ENODEV;
    }
    h->n_streams = n_streams;
    h->law = law;
    h->codecs_default = true;
    // the tables.  Every fresh value is zero (unsynced, counters 0, an empty history, no key down) but the codecs'
    h->send = LegState("wmx_rtp_create: hipMalloc/hipMemset", "handle", n_streams, kLegSendColumns);
    h->seq = LegState("hipMemset(sequence state)", "handle", n_streams, kLegSeqColumns);
    h->codec = LegState("hipMemset(codec state)", "handle", n_streams, leg_codec_columns(law));
    h->plc = LegState("hipMemset(concealment state)", "handle", n_streams, kLegPlcColumns);
    h->dtmf = LegState("hipMemset(DTMF state)", "handle", n_streams, kLegDtmfColumns);
    const int rc = h->send.make();
    if (rc) {
        wmx_rtp_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

int wmx_rtp_destroy(wmx_rtp *h) {
    WMX_ON_DEVICE(h);
    if (!h) return 0;
    for (LegState *st : {&h->send, &h->seq, &h->codec, &h->plc, &h->dtmf}) st->destroy();
    if (h->d_rec) (void)hipFree(h->d_rec);  // the gather list lies behind it
    delete h;
    return 0;
}

int wmx_rtp_egress(wmx_rtp *h, int in_chn, int in_freq, const int16_t *d_pcm, uint32_t in_bytes, long pcm_stride, int out_chn,
                   int out_freq, uint8_t *d_packets, long packet_stride, uint32_t *packet_bytes, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h || !d_pcm || !d_packets || in_chn < 1 || in_chn > 2 || out_chn < 1 || out_chn > 2 || in_freq < 1 || out_freq < 1 ||
        in_bytes == 0 || (h->n_streams > 1 && pcm_stride < (long)(in_bytes / 2))) {
        set_error("wmx_rtp_egress: bad arguments");
        return WMX_EINVAL;
    }
    const uint64_t k0 = ((uint64_t)in_chn << 56) | ((uint64_t)out_chn << 48) | ((uint64_t)(uint32_t)in_freq << 24) | (uint32_t)out_freq;
    SchedCache::Entry *ent = h->sched.find(k0, in_bytes);
    if (!ent) {
        zoom_gather_list(in_chn, in_freq, in_bytes, out_chn, out_freq, h->idx);
        const int rc = h->sched.add(k0, in_bytes, h->idx.data(), h->idx.size() * sizeof(int32_t), h->idx.size(), &ent);
        if (rc) return rc;
    }
    const int32_t *d_idx = (const int32_t *)ent->p;
    const int n_codes = (int)ent->n;  // PCM2G711x returns DataLen / 2 codes
    if (packet_stride < kRtpHeader + n_codes) {
        set_error("wmx_rtp_egress: packet_stride %ld < %d", packet_stride, kRtpHeader + n_codes);
        return WMX_EINVAL;
    }
    if (packet_bytes) *packet_bytes = (uint32_t)(kRtpHeader + n_codes);
    const dim3 block(256), grid((unsigned)((n_codes + 255) / 256 > 0 ? (n_codes + 255) / 256 : 1), (unsigned)h->n_streams);
    const int pt = h->law == WMX_LAW_A ? 8 : 0;  // RTP_PAYLOAD_TYPE_PCMA / PCMU, src/rtp.h:21-24
    // per stream once a stream has left the default (leg_codec.h)
    const uint8_t *laws = h->codecs_default ? nullptr : h->codec.at<uint8_t>(kCodecOutLaw);
    uint32_t *d_seq = h->send.at<uint32_t>(kSendSeq), *d_ts = h->send.at<uint32_t>(kSendTs);
    if (n_codes >= 4 && n_codes % 4 == 0 && aligned_to(d_packets, packet_stride, 4)) {  // four codes per lane (the gather list is 16-byte aligned)
        const unsigned wgrid = wmx::stream_grid((size_t)h->n_streams * (n_codes / 4), 256);
        auto kernel = laws ? rtp_egress_wide_kernel<kLawPerStream>
                           : (h->law == WMX_LAW_A ? rtp_egress_wide_kernel<WMX_LAW_A> : rtp_egress_wide_kernel<WMX_LAW_U>);
        hipLaunchKernelGGL(kernel, dim3(wgrid), block, 0, as_stream(stream), d_pcm, pcm_stride, d_idx, n_codes, n_codes / out_chn, d_seq,
                           d_ts, d_packets, packet_stride, h->n_streams, pt, laws);
    } else {
        auto kernel = laws ? rtp_egress_kernel<kLawPerStream> : (h->law == WMX_LAW_A ? rtp_egress_kernel<WMX_LAW_A> : rtp_egress_kernel<WMX_LAW_U>);
        hipLaunchKernelGGL(kernel, grid, block, 0, as_stream(stream), d_pcm, pcm_stride, d_idx, n_codes, n_codes / out_chn, d_seq, d_ts,
                           d_packets, packet_stride, h->n_streams, pt, laws);
    }
    WMX_LAUNCH_CHECK();
    return h->sched.used(ent, as_stream(stream));
}

int wmx_rtp_ingest(int n_streams, const uint8_t *d_packets, long packet_stride, int16_t *d_pcm, long pcm_stride, uint32_t *d_pcm_bytes,
                   uint16_t *d_seq_raw, void *stream) {
    if (n_streams < 0 || !d_packets || !d_pcm || packet_stride < kRtpHeader + kRtpG711Payload || (n_streams > 1 && pcm_stride < kRtpG711Payload)) {
        set_error("wmx_rtp_ingest: bad arguments");
        return WMX_EINVAL;
    }
    if (n_streams == 0) return 0;
    if (aligned_to(d_packets, packet_stride, 4) && aligned_to(d_pcm, pcm_stride * 2, 8))
        hipLaunchKernelGGL(rtp_ingest_wide_kernel, dim3(wmx::stream_grid((size_t)n_streams * kRtpWords, 256)), dim3(256), 0, as_stream(stream),
                           d_packets, packet_stride, d_pcm, pcm_stride, d_pcm_bytes, d_seq_raw, n_streams);
    else
        hipLaunchKernelGGL(rtp_ingest_kernel, dim3((unsigned)n_streams), dim3(64), 0, as_stream(stream), d_packets, packet_stride, d_pcm,
                           pcm_stride, d_pcm_bytes, d_seq_raw, n_streams);
    WMX_LAUNCH_CHECK();
    return 0;
}

// what wmx_rtp_ingest_legs and wmx_rtp_ingest_legs_codecs share: the argument check, and the launch (d_refused NULL: no count;
// d_in_codec NULL: every leg is WMX_CODEC_REFERENCE)
static int ingest_legs_check(const char *who, int n_legs, int max_packets, const uint8_t *d_packets, long leg_stride, long packet_stride,
                             const int32_t *d_recv_bytes, const int16_t *d_pcm, long source_stride, long pcm_packet_stride,
                             const uint32_t *d_len) {
    if (n_legs < 0 || max_packets < 1 || max_packets > 4 || !d_packets || !d_recv_bytes || !d_pcm || !d_len ||
        packet_stride < kRtpHeader + kRtpG711Payload || pcm_packet_stride < kRtpG711Payload ||
        (n_legs > 1 && (leg_stride < packet_stride * max_packets || source_stride < pcm_packet_stride * max_packets))) {
        set_error("%s: bad arguments", who);
        return WMX_EINVAL;
    }
    return 0;
}

static int ingest_legs_launch(int n_legs, int max_packets, const uint8_t *d_packets, long leg_stride, long packet_stride,
                              const int32_t *d_recv_bytes, int16_t *d_pcm, long source_stride, long pcm_packet_stride, uint32_t *d_len,
                              uint16_t *d_seq_raw, const uint8_t *d_in_codec, uint32_t *d_refused, void *stream) {
    if (n_legs == 0) return 0;
    const size_t rows = (size_t)n_legs * max_packets;
    const bool wide = aligned_to(d_packets, packet_stride, 4) && leg_stride % 4 == 0 && aligned_to(d_pcm, pcm_packet_stride * 2, 8) &&
                      (source_stride * 2) % 8 == 0;
    auto kernel = !d_refused   ? (wide ? rtp_ingest_legs_codecs_kernel<true, false, false> : rtp_ingest_legs_codecs_kernel<false, false, false>)
                  : d_in_codec ? (wide ? rtp_ingest_legs_codecs_kernel<true, true, true> : rtp_ingest_legs_codecs_kernel<false, true, true>)
                               : (wide ? rtp_ingest_legs_codecs_kernel<true, false, true> : rtp_ingest_legs_codecs_kernel<false, false, true>);
    hipLaunchKernelGGL(kernel, dim3(wmx::stream_grid(rows * (wide ? kRtpWords : kRtpG711Payload), 256)), dim3(256), 0, as_stream(stream), d_packets,
                       leg_stride, packet_stride, d_recv_bytes, d_pcm, source_stride, pcm_packet_stride, d_len, d_seq_raw, max_packets, n_legs,
                       d_in_codec, d_refused);
    WMX_LAUNCH_CHECK();
    return 0;
}

int wmx_rtp_ingest_legs(int n_legs, int max_packets, const uint8_t *d_packets, long leg_stride, long packet_stride, const int32_t *d_recv_bytes,
                        int16_t *d_pcm, long source_stride, long pcm_packet_stride, uint32_t *d_len, uint16_t *d_seq_raw, void *stream) {
    const int rc = ingest_legs_check("wmx_rtp_ingest_legs", n_legs, max_packets, d_packets, leg_stride, packet_stride, d_recv_bytes, d_pcm,
                                     source_stride, pcm_packet_stride, d_len);
    return rc ? rc
              : ingest_legs_launch(n_legs, max_packets, d_packets, leg_stride, packet_stride, d_recv_bytes, d_pcm, source_stride, pcm_packet_stride,
                                   d_len, d_seq_raw, nullptr, nullptr, stream);
}

// Play and send in one launch: wmx_mix_drain(320 bytes) followed by wmx_rtp_egress(1, 8000 -> 1, 8000), byte for byte, for a mixer of
// 1 x 8000 rings and as many senders as it has rings.
int wmx_rtp_egress_rings(wmx_rtp *h, wmx_mix *m, uint8_t *d_packets, long packet_stride, uint32_t *packet_bytes, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h || !m || !d_packets) {
        set_error("wmx_rtp_egress_rings: bad arguments");
        return WMX_EINVAL;
    }
    const MixPlayView v = mix_play_view(m);
    if (v.chn != 1 || v.freq != kRtpG711Payload * 50) {
        set_error("wmx_rtp_egress_rings: rings of %d x %d, not 1 x 8000 (wmx_mix_drain + wmx_rtp_egress convert)", v.chn, v.freq);
        return WMX_EINVAL;
    }
    if (v.n_groups != h->n_streams) {
        set_error("wmx_rtp_egress_rings: %d rings, %d senders", v.n_groups, h->n_streams);
        return WMX_EINVAL;
    }
    if (v.device != h->device) {
        set_error("wmx_rtp_egress_rings: the mixer is on device %d, the senders on %d", v.device, h->device);
        return WMX_EINVAL;
    }
    if (packet_stride < kRtpHeader + kRtpG711Payload) {
        set_error("wmx_rtp_egress_rings: packet_stride %ld < %d", packet_stride, kRtpHeader + kRtpG711Payload);
        return WMX_EINVAL;
    }
    const uint32_t ring_samples = v.ring_bytes / 2, head_sample = (v.head_off / 2) % ring_samples;
    const bool wide_in = head_sample % 4 == 0 && ring_samples % 4 == 0 && reinterpret_cast<uintptr_t>(v.d_rings) % 8 == 0;
    const bool wide_out = aligned_to(d_packets, packet_stride, 4);
    // per ring once a stream has left the default (leg_codec.h)
    const uint8_t *laws = h->codecs_default ? nullptr : h->codec.at<uint8_t>(kCodecOutLaw);
    auto kernel = wide_in ? (wide_out ? rtp_egress_rings_kernel<true, true, false> : rtp_egress_rings_kernel<true, false, false>)
                          : (wide_out ? rtp_egress_rings_kernel<false, true, false> : rtp_egress_rings_kernel<false, false, false>);
    if (laws)
        kernel = wide_in ? (wide_out ? rtp_egress_rings_kernel<true, true, true> : rtp_egress_rings_kernel<true, false, true>)
                         : (wide_out ? rtp_egress_rings_kernel<false, true, true> : rtp_egress_rings_kernel<false, false, true>);
    const int pt = h->law == WMX_LAW_A ? 8 : 0;  // RTP_PAYLOAD_TYPE_PCMA / PCMU, src/rtp.h:21-24
    hipLaunchKernelGGL(kernel, dim3(wmx::stream_grid((size_t)h->n_streams * kRtpWords, 256)), dim3(256), 0, as_stream(stream), v.d_rings,
                       ring_samples, head_sample, h->law, h->send.at<uint32_t>(kSendSeq), h->send.at<uint32_t>(kSendTs), d_packets, packet_stride,
                       h->n_streams, pt, laws);
    WMX_LAUNCH_CHECK();
    mix_played(m, 2u * kRtpG711Payload);
    if (packet_bytes) *packet_bytes = (uint32_t)(kRtpHeader + kRtpG711Payload);
    return 0;
}

// The payload of each leg's outgoing datagram decoded with that leg's outgoing law (include/wmix_amd.h): the far end of its canceller
int wmx_rtp_decode_sent_legs(wmx_rtp *h, const uint8_t *d_packets, long packet_stride, int16_t *d_pcm, long pcm_leg_stride, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h || !d_packets || !d_pcm || packet_stride < kRtpHeader + kRtpG711Payload || (h->n_streams > 1 && pcm_leg_stride < kRtpG711Payload) ||
        reinterpret_cast<uintptr_t>(d_pcm) % sizeof(int16_t) != 0) {
        set_error("wmx_rtp_decode_sent_legs: bad arguments (packet_stride %ld >= %d, pcm_leg_stride %ld >= %d, d_pcm on a 2-byte boundary)",
                  packet_stride, kRtpHeader + kRtpG711Payload, pcm_leg_stride, kRtpG711Payload);
        return WMX_EINVAL;
    }
    const uint8_t *laws = h->codecs_default ? nullptr : h->codec.at<uint8_t>(kCodecOutLaw);
    hipLaunchKernelGGL(rtp_decode_sent_legs_kernel, dim3(wmx::stream_grid((size_t)h->n_streams * kRtpG711Payload, 256)), dim3(256), 0,
                       as_stream(stream), d_packets, packet_stride, d_pcm, pcm_leg_stride, h->n_streams, h->law, laws);
    WMX_LAUNCH_CHECK();
    return 0;
}

// seq = timestamp = 0 for the listed senders (NULL = all), on `stream`: what wmix_thread_rtp_send_pcma starts a call from
// (src/wmixTask.c:1058)
int wmx_rtp_reset_streams(wmx_rtp *h, const int32_t *host_idx, int n, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    return h->send.reset("wmx_rtp_reset_streams: sender", host_idx, n, as_stream(stream));
}

// ---- the sequence rule per leg (include/wmix_amd.h, leg_seq.h)
int wmx_rtp_sequence_legs(wmx_rtp *h, int max_packets, int max_gap, const uint16_t *d_seq_raw, uint32_t *d_len, uint32_t *d_calls,
                          void *stream) {
    WMX_ON_DEVICE(h);
    if (!h || !d_seq_raw || !d_len || !d_calls || max_packets < 1 || max_packets > kLegMaxCalls || max_gap < 0 || max_gap > kLegMaxCalls - 1) {
        set_error("wmx_rtp_sequence_legs: max_packets=%d must be 1 .. %d, max_gap=%d 0 .. %d, and no pointer NULL", max_packets, kLegMaxCalls,
                  max_gap, kLegMaxCalls - 1);
        return WMX_EINVAL;
    }
    const int rcs = h->seq.make();
    if (rcs) return rcs;
    const bool wide = max_packets == kLegMaxCalls && reinterpret_cast<uintptr_t>(d_seq_raw) % 8 == 0;
    hipLaunchKernelGGL(wide ? rtp_sequence_legs_kernel<true> : rtp_sequence_legs_kernel<false>, dim3(wmx::stream_grid((size_t)h->n_streams, 256)),
                       dim3(256), 0, as_stream(stream), d_seq_raw, d_len, d_calls, h->seq.at<uint32_t>(kSeqSynced), max_packets, (uint32_t)max_gap,
                       h->n_streams);
    WMX_LAUNCH_CHECK();
    return 0;
}

// unsynced and counters 0 (the refused count of the codec rule among them) for the listed legs (NULL = all), on `stream`: a new call
// may start at any sequence number
int wmx_rtp_reset_sequence(wmx_rtp *h, const int32_t *host_idx, int n, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    hipStream_t s = as_stream(stream);
    const int rc = h->seq.reset("wmx_rtp_reset_sequence: leg", host_idx, n, s);
    if (rc || !h->codec.p) return rc;  // no codec state: its counter is fresh
    // the receive side's other counter (leg_codec.h); the leg's codec stays
    return h->codec.reset("wmx_rtp_reset_sequence: leg", host_idx, n, s, kCodecRefused, kCodecRefused + 1);
}

// next (uint16), synced (uint8) and the five counters (uint32) of every leg as the work queued on `stream` leaves them; any pointer may
// be NULL; blocking
int wmx_rtp_export_sequence(wmx_rtp *h, uint16_t *next, uint8_t *synced, uint32_t *lost, uint32_t *late, uint32_t *dup, uint32_t *resync,
                            uint32_t *overflow, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    const size_t n = (size_t)h->n_streams;
    std::vector<uint32_t> w(2 * n);  // synced and next as the device holds them: a word each
    const int rc = h->seq.export_to({synced ? w.data() : nullptr, next ? w.data() + n : nullptr, lost, late, dup, resync, overflow},
                                    as_stream(stream));
    for (size_t r = 0; rc == 0 && r < n; r++) {
        if (synced) synced[r] = (uint8_t)(w[r] != 0);
        if (next) next[r] = (uint16_t)w[n + r];
    }
    return rc;
}

// ---- the concealment rule per leg (include/wmix_amd.h, leg_plc.h)
int wmx_rtp_conceal_legs(wmx_rtp *h, int max_packets, const int16_t *d_pcm, long source_stride, long pcm_packet_stride, const uint32_t *d_len,
                         const uint32_t *d_calls, int16_t *d_pcm_out, uint32_t *d_len_out, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h || !d_pcm || !d_len || !d_calls || !d_pcm_out || !d_len_out || max_packets < 1 || max_packets > kLegMaxCalls) {
        set_error("wmx_rtp_conceal_legs: max_packets=%d must be 1 .. %d, and no pointer NULL", max_packets, kLegMaxCalls);
        return WMX_EINVAL;
    }
    const size_t n = (size_t)h->n_streams;
    if (pcm_packet_stride < kLegRow || (n > 1 && source_stride < pcm_packet_stride * max_packets)) {
        set_error("wmx_rtp_conceal_legs: rows that overlap (pcm_packet_stride %ld < %d, or source_stride %ld shorter than %d rows)",
                  pcm_packet_stride, kLegRow, source_stride, max_packets);
        return WMX_EINVAL;
    }
    const int16_t *in_end = d_pcm + (n - 1) * (size_t)source_stride + (size_t)(max_packets - 1) * pcm_packet_stride + kLegRow;
    const int16_t *out_end = d_pcm_out + n * (size_t)(kLegMaxCalls * kLegRow);
    if (reinterpret_cast<uintptr_t>(d_pcm) < reinterpret_cast<uintptr_t>(out_end) &&
        reinterpret_cast<uintptr_t>(d_pcm_out) < reinterpret_cast<uintptr_t>(in_end)) {
        set_error("wmx_rtp_conceal_legs: the repaired rows overlap the rows they are made from");
        return WMX_EINVAL;
    }
    const int rcs = h->plc.make();
    if (rcs) return rcs;
    const bool wide = aligned_to(d_pcm, pcm_packet_stride * 2, 4) && (source_stride * 2) % 4 == 0 && reinterpret_cast<uintptr_t>(d_pcm_out) % 4 == 0;
    hipLaunchKernelGGL(wide ? rtp_conceal_legs_kernel<true> : rtp_conceal_legs_kernel<false>,
                       dim3((unsigned)((n + kPlcLegsPerBlock - 1) / kPlcLegsPerBlock)), dim3(64 * kPlcLegsPerBlock), 0, as_stream(stream), d_pcm,
                       source_stride, pcm_packet_stride, d_len, d_calls, max_packets, d_pcm_out, d_len_out, h->plc.at<int16_t>(kPlcColHist),
                       h->plc.at<uint32_t>(kPlcColConcealed), h->n_streams);
    WMX_LAUNCH_CHECK();
    return 0;
}

// a fresh history and concealed = 0 for the listed legs (NULL = all), on `stream`: a new call does not repeat the old call's voice
int wmx_rtp_reset_conceal(wmx_rtp *h, const int32_t *host_idx, int n, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    return h->plc.reset("wmx_rtp_reset_conceal: leg", host_idx, n, as_stream(stream));
}

// hist (n_streams x 320 int16, newest last) and concealed (uint32) of every leg as the work queued on `stream` leaves them; any pointer
// may be NULL; blocking
int wmx_rtp_export_conceal(wmx_rtp *h, int16_t *hist, uint32_t *concealed, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    return h->plc.export_to({hist, concealed}, as_stream(stream));
}

// ---- the DTMF rule per leg (include/wmix_amd.h, leg_dtmf.h)
int wmx_rtp_detect_dtmf_legs(wmx_rtp *h, int max_packets, const uint8_t *d_in, long leg_stride, long packet_stride, const int32_t *d_recv,
                             int16_t *d_pcm, long source_stride, long pcm_packet_stride, const uint32_t *d_len, const uint32_t *d_calls,
                             int event_pt, int suppress, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h || !d_in || !d_recv || !d_pcm || !d_len || max_packets < 1 || max_packets > kLegMaxCalls || event_pt < 96 || event_pt > 127) {
        set_error("wmx_rtp_detect_dtmf_legs: max_packets=%d must be 1 .. %d, event_pt=%d 96 .. 127, and no pointer but d_calls NULL", max_packets,
                  kLegMaxCalls, event_pt);
        return WMX_EINVAL;
    }
    const size_t n = (size_t)h->n_streams;
    if (packet_stride < kRtpHeader + kRtpG711Payload || pcm_packet_stride < kLegRow ||
        (n > 1 && (leg_stride < packet_stride * max_packets || source_stride < pcm_packet_stride * max_packets))) {
        set_error("wmx_rtp_detect_dtmf_legs: rows that overlap (packet_stride %ld < %d, pcm_packet_stride %ld < %d, or a leg stride shorter than %d rows)",
                  packet_stride, kRtpHeader + kRtpG711Payload, pcm_packet_stride, kLegRow, max_packets);
        return WMX_EINVAL;
    }
    const int rcs = h->dtmf.make();
    if (rcs) return rcs;
    const bool wide = aligned_to(d_pcm, pcm_packet_stride * 2, 4) && (source_stride * 2) % 4 == 0;
    hipLaunchKernelGGL(wide ? rtp_detect_dtmf_legs_kernel<true> : rtp_detect_dtmf_legs_kernel<false>,
                       dim3((unsigned)((n + kDtmfLegsPerBlock - 1) / kDtmfLegsPerBlock)), dim3(32 * kDtmfLegsPerBlock), 0, as_stream(stream), d_in,
                       leg_stride, packet_stride, d_recv, d_pcm, source_stride, pcm_packet_stride, d_len, d_calls, max_packets, (uint32_t)event_pt,
                       suppress ? 1 : 0, h->dtmf.at<uint64_t>(kDtmfRing), h->dtmf.at<uint32_t>(kDtmfCount), h->dtmf.at<uint32_t>(kDtmfTs),
                       h->dtmf.at<uint32_t>(kDtmfFlags), h->n_streams);
    WMX_LAUNCH_CHECK();
    return 0;
}

// nothing reported, no key down and no event timestamp for the listed legs (NULL = all), on `stream`: a new call does not inherit half a
// key press
int wmx_rtp_reset_dtmf(wmx_rtp *h, const int32_t *host_idx, int n, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    return h->dtmf.reset("wmx_rtp_reset_dtmf: leg", host_idx, n, as_stream(stream));
}

// count (uint32) and ring (n_streams x 8 uint8) of every leg as the work queued on `stream` leaves them; either pointer may be NULL;
// blocking
int wmx_rtp_export_dtmf(wmx_rtp *h, uint32_t *count, uint8_t *ring, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    return h->dtmf.export_to({ring, count}, as_stream(stream));
}

// ---- the recording taps (include/wmix_amd.h, leg_record.h)
// the store, once and blocking: max_taps taps of one format, chn x freq
int wmx_rtp_recorders(wmx_rtp *h, int max_taps, int chn, int freq) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    if (h->d_rec) {
        set_error("wmx_rtp_recorders: the senders have their store already (%zu taps of %d x %d)", h->rec.size(), h->rec_chn, h->rec_freq);
        return WMX_ESTATE;
    }
    if (max_taps < 1 || max_taps > (1 << 20) || chn < 1 || chn > 2 || freq < 1 || freq > kRecordMaxFreq) {
        set_error("wmx_rtp_recorders: max_taps=%d (1 .. 2^20) chn=%d (1, 2) freq=%d (1 .. %d)", max_taps, chn, freq, kRecordMaxFreq);
        return WMX_EINVAL;
    }
    zoom_gather_list(1, kRtpG711Payload * 50, 2u * kRecordRowIn, chn, freq, h->idx);
    const size_t row = h->idx.size(), state_bytes = (size_t)max_taps * sizeof(LegRecord);
    if (row == 0) {
        set_error("wmx_rtp_recorders: wmix_pcm_zoom writes nothing for a package of 1 x 8000 -> %d x %d", chn, freq);
        return WMX_EINVAL;
    }
    bool identity = row == (size_t)kRecordRowIn, twice = row == 2u * kRecordRowIn;
    for (size_t i = 0; i < row; i++) {
        if (h->idx[i] < 0 || h->idx[i] >= kRecordRowIn) {
            set_error("wmx_rtp_recorders: the zoom's list reads sample %d of a package of %d", (int)h->idx[i], kRecordRowIn);
            return WMX_EINVAL;
        }
        identity = identity && h->idx[i] == (int32_t)i;
        twice = twice && h->idx[i] == (int32_t)(i / 2);
    }
    void *p = nullptr;
    WMX_HIP(hipMalloc(&p, state_bytes + row * sizeof(int32_t)));
    const std::vector<LegRecord> fresh((size_t)max_taps, leg_record_free(0u));
    hipError_t e = hipMemcpy(p, fresh.data(), state_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(static_cast<uint8_t *>(p) + state_bytes, h->idx.data(), row * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)hipFree(p);
        return hip_fail(e, "hipMemcpy(recording taps)", __FILE__, __LINE__);
    }
    h->d_rec = static_cast<LegRecord *>(p);
    h->d_rec_idx = reinterpret_cast<const int32_t *>(h->d_rec + max_taps);
    h->rec = fresh;
    h->rec_chn = chn, h->rec_freq = freq;
    h->rec_row = (uint32_t)row;
    h->rec_mode = identity ? kRecIdentity : (twice ? kRecDouble : kRecGather);
    return 0;
}

int wmx_rtp_record_row_bytes(const wmx_rtp *h) { return h ? (int)(h->rec_row * sizeof(int16_t)) : WMX_EINVAL; }

// tap `k` takes `value` on the host and, ordered on `s`, on the device
static int record_set(wmx_rtp *h, size_t k, const LegRecord &value, hipStream_t s) {
    hipLaunchKernelGGL(rtp_record_set_kernel, dim3(1), dim3(64), 0, s, h->d_rec, (int)k, value);
    WMX_LAUNCH_CHECK();
    h->rec[k] = value;
    return 0;
}

static int record_store(const wmx_rtp *h, const char *who) {
    if (h->d_rec) return 0;
    set_error("%s: no store (wmx_rtp_recorders)", who);
    return WMX_ESTATE;
}

// the n listed legs start: a leg that has a tap in place, the others at the lowest free taps; ticks rows each, 0 = until stopped.
// host_taps_out (n int32, or NULL) takes the taps.  Too few free taps: WMX_ESTATE and nothing started.
int wmx_rtp_record(wmx_rtp *h, const int32_t *host_idx, int n, int ticks, int32_t *host_taps_out, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h || !host_idx || n < 0 || ticks < 0) {
        set_error("wmx_rtp_record: a list of n >= 0 legs and ticks >= 0 (0: until stopped)");
        return WMX_EINVAL;
    }
    const int rcs = record_store(h, "wmx_rtp_record");
    if (rcs) return rcs;
    if (idx_check(host_idx, n, h->n_streams, "wmx_rtp_record: leg", "handle")) return WMX_EINVAL;
    std::vector<int32_t> taps((size_t)n);
    if (!leg_record_assign(h->rec.data(), (int)h->rec.size(), host_idx, n, taps.data())) {
        set_error("wmx_rtp_record: %d legs and fewer free taps among the store's %zu; nothing started", n, h->rec.size());
        return WMX_ESTATE;
    }
    for (int i = 0; i < n; i++) {
        const int rc = record_set(h, (size_t)taps[(size_t)i], leg_record_start(host_idx[i], (uint32_t)ticks), as_stream(stream));
        if (rc) return rc;
        if (host_taps_out) host_taps_out[i] = taps[(size_t)i];
    }
    return 0;
}

// the taps of the n listed legs (NULL = every tap) are free from the next tick on: keep_written: a stop; otherwise the leg's reset
static int record_end(wmx_rtp *h, const char *who, const int32_t *host_idx, int n, bool keep_written, void *stream) {
    if ((host_idx && n < 0) || idx_check(host_idx, n, h->n_streams, who, "handle")) return WMX_EINVAL;
    for (size_t k = 0; k < h->rec.size(); k++) {
        const LegRecord was = h->rec[k];
        bool listed = !host_idx;
        for (int i = 0; host_idx && was.leg >= 0 && i < n && !listed; i++) listed = was.leg == host_idx[i];
        if (!listed) continue;
        const LegRecord now = keep_written ? leg_record_stop(was) : leg_record_reset();
        if (now.leg == was.leg && now.left == was.left && now.written == was.written) continue;  // a free tap, as it is already
        const int rc = record_set(h, k, now, as_stream(stream));
        if (rc) return rc;
    }
    return 0;
}

int wmx_rtp_record_stop(wmx_rtp *h, const int32_t *host_idx, int n, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    const int rcs = record_store(h, "wmx_rtp_record_stop");
    return rcs ? rcs : record_end(h, "wmx_rtp_record_stop: leg", host_idx, n, true, stream);
}

// what a new call in a used slot needs: the leg's recording ends, as wmix_reset ends the daemon's record threads.  No store: nothing.
int wmx_rtp_reset_record(wmx_rtp *h, const int32_t *host_idx, int n, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    if (!h->d_rec) return (host_idx && n < 0) || idx_check(host_idx, n, h->n_streams, "wmx_rtp_reset_record: leg", "handle") ? WMX_EINVAL : 0;
    return record_end(h, "wmx_rtp_reset_record: leg", host_idx, n, false, stream);
}

// leg (int32, -1: free), left and written (uint32) of every tap as the work queued on `stream` leaves them; any pointer may be NULL;
// blocking
int wmx_rtp_export_record(wmx_rtp *h, int32_t *leg, uint32_t *left, uint32_t *written, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    const int rcs = record_store(h, "wmx_rtp_export_record");
    if (rcs) return rcs;
    std::vector<LegRecord> st(h->rec.size());
    WMX_HIP(hipStreamSynchronize(as_stream(stream)));
    WMX_HIP(hipMemcpy(st.data(), h->d_rec, st.size() * sizeof(LegRecord), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < st.size(); k++) {
        if (leg) leg[k] = st[k].leg;
        if (left) left[k] = st[k].left;
        if (written) written[k] = st[k].written;
    }
    return 0;
}

// One tick of every tap, in front of wmx_rtp_egress_rings on the same mixer: a running tap's row -- ring `leg` from the play head on,
// through the store's zoom -- into d_rows + tap * row_stride (int16 elements), its leg into d_legs[tap]; a free tap: -1 and no row.
int wmx_rtp_record_rings(wmx_rtp *h, wmx_mix *m, int16_t *d_rows, long row_stride, int32_t *d_legs, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h || !m || !d_rows || !d_legs) {
        set_error("wmx_rtp_record_rings: bad arguments");
        return WMX_EINVAL;
    }
    const int rcs = record_store(h, "wmx_rtp_record_rings");
    if (rcs) return rcs;
    const MixPlayView v = mix_play_view(m);
    if (v.chn != 1 || v.freq != kRtpG711Payload * 50 || v.n_groups != h->n_streams || v.device != h->device) {
        set_error("wmx_rtp_record_rings: a mixer of %d rings of %d x %d on device %d; the senders are %d on device %d and tap rings of 1 x 8000",
                  v.n_groups, v.chn, v.freq, v.device, h->n_streams, h->device);
        return WMX_EINVAL;
    }
    const uint32_t ring_samples = v.ring_bytes / 2, head_sample = (v.head_off / 2) % ring_samples;
    // the conference handle's mixer: it is drained a package at a time, so a row never straddles the ring's end
    if (v.head_off % (2u * kRecordRowIn) != 0 || ring_samples % (uint32_t)kRecordRowIn != 0 || reinterpret_cast<uintptr_t>(v.d_rings) % 16 != 0) {
        set_error("wmx_rtp_record_rings: the play head (byte %u of %u) is not on a package of %d bytes: this mixer has been drained otherwise",
                  v.head_off, v.ring_bytes, 2 * kRecordRowIn);
        return WMX_EINVAL;
    }
    const size_t n_taps = h->rec.size();
    if (row_stride < (long)h->rec_row && n_taps > 1) {
        set_error("wmx_rtp_record_rings: rows that overlap (row_stride %ld < %u samples)", row_stride, h->rec_row);
        return WMX_EINVAL;
    }
    if (reinterpret_cast<uintptr_t>(d_rows) % sizeof(int16_t) != 0 || reinterpret_cast<uintptr_t>(d_legs) % sizeof(int32_t) != 0) {
        set_error("wmx_rtp_record_rings: d_rows on a 2-byte and d_legs on a 4-byte boundary");
        return WMX_EINVAL;
    }
    const int mode = aligned_to(d_rows, row_stride * 2, 16) ? h->rec_mode : kRecGather;
    auto kernel = mode == kRecIdentity ? rtp_record_rings_kernel<kRecIdentity>
                                       : (mode == kRecDouble ? rtp_record_rings_kernel<kRecDouble> : rtp_record_rings_kernel<kRecGather>);
    const unsigned waves = 4, grid = ((unsigned)n_taps + waves - 1) / waves;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), 0, as_stream(stream), (const int16_t *)v.d_rings, ring_samples, head_sample, h->d_rec,
                       h->d_rec_idx, h->rec_row, d_rows, row_stride, d_legs, (int)n_taps, h->n_streams);
    WMX_LAUNCH_CHECK();
    for (LegRecord &r : h->rec) (void)leg_record_tick(r);  // behind the check: a launch that failed has moved no tap
    return 0;
}

// ---- the codec rule per stream (include/wmix_amd.h, leg_codec.h): fresh is refused 0, in_codec REFERENCE, out_law the law of create
// in_codec (WMX_CODEC_*) and out_law (WMX_LAW_*) of the listed streams (NULL = all), on `stream`; the refused counts stay
int wmx_rtp_set_codecs(wmx_rtp *h, const int32_t *host_idx, int n, int in_codec, int out_law, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h || (host_idx && n < 0)) return WMX_EINVAL;
    if (!leg_codec_valid(in_codec) || !leg_law_valid(out_law)) {
        set_error("wmx_rtp_set_codecs: in_codec %d must be WMX_CODEC_REFERENCE .. WMX_CODEC_BY_PT and out_law %d WMX_LAW_A or WMX_LAW_U", in_codec,
                  out_law);
        return WMX_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    int rc = h->codec.set("wmx_rtp_set_codecs: stream", kCodecIn, in_codec, host_idx, n, s);
    if (rc == 0) rc = h->codec.set("wmx_rtp_set_codecs: stream", kCodecOutLaw, out_law, host_idx, n, s);
    if (rc) return rc;
    const bool is_default = in_codec == WMX_CODEC_REFERENCE && out_law == h->law;
    if (!host_idx)
        h->codecs_default = is_default;
    else if (n > 0 && !is_default)
        h->codecs_default = false;
    return 0;
}

// in_codec, out_law (uint8) and refused (uint32) of every stream as the work queued on `stream` leaves them; any pointer may be NULL;
// blocking
int wmx_rtp_export_codecs(wmx_rtp *h, uint8_t *in_codec, uint8_t *out_law, uint32_t *refused, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    return h->codec.export_to({refused, in_codec, out_law}, as_stream(stream));
}

// wmx_rtp_ingest_legs for the handle's streams as legs, with the codec rule per leg
int wmx_rtp_ingest_legs_codecs(wmx_rtp *h, int max_packets, const uint8_t *d_packets, long leg_stride, long packet_stride,
                               const int32_t *d_recv_bytes, int16_t *d_pcm, long source_stride, long pcm_packet_stride, uint32_t *d_len,
                               uint16_t *d_seq_raw, void *stream) {
    WMX_ON_DEVICE(h);
    const int rcc = ingest_legs_check("wmx_rtp_ingest_legs_codecs", h ? h->n_streams : -1, max_packets, d_packets, leg_stride, packet_stride,
                                      d_recv_bytes, d_pcm, source_stride, pcm_packet_stride, d_len);
    if (rcc) return rcc;
    const int rcs = h->codec.make();
    if (rcs) return rcs;
    return ingest_legs_launch(h->n_streams, max_packets, d_packets, leg_stride, packet_stride, d_recv_bytes, d_pcm, source_stride,
                              pcm_packet_stride, d_len, d_seq_raw, h->codecs_default ? nullptr : h->codec.at<uint8_t>(kCodecIn),
                              h->codec.at<uint32_t>(kCodecRefused), stream);
}

int wmx_rtp_export(wmx_rtp *h, int stream_index, uint16_t *seq, uint32_t *timestamp) {
    WMX_ON_DEVICE(h);
    if (!h || stream_index < 0 || stream_index >= h->n_streams) return WMX_EINVAL;
    uint32_t s = 0, t = 0;
    WMX_HIP(hipDeviceSynchronize());
    WMX_HIP(hipMemcpy(&s, h->send.at<uint32_t>(kSendSeq) + stream_index, 4, hipMemcpyDeviceToHost));
    WMX_HIP(hipMemcpy(&t, h->send.at<uint32_t>(kSendTs) + stream_index, 4, hipMemcpyDeviceToHost));
    if (seq) *seq = (uint16_t)s;
    if (timestamp) *timestamp = t;
    return 0;
}

}  // extern "C"
