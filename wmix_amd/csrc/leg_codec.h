// leg_codec.h -- the codec rule of one RTP leg (wmx_rtp_ingest_legs_codecs, wmx_rtp_egress*, rtp.hip): which datagram slots of a leg
// make a wmix_load_data call, with which G.711 law their payload is decoded, and which law and payload type the leg is sent.
//
// The reference's receive thread accepts payload types 8 (PCMA) and 0 (PCMU) alike (rtp_recv, src/rtp.c:88-95) and decodes both with
// G711a2PCM (src/wmixTask.c:1282): a leg that negotiated PCMU is mixed in as noise.  A leg's in_codec says what the leg negotiated:
//
//   arrived = recvfrom returned > 0 for the slot; pt = header byte 1 & 0x7F; g711 = arrived && (pt == 8 || pt == 0)
//
//   in_codec                 the slot makes a call when    decoded as
//   WMX_CODEC_REFERENCE 0    g711                          A-law, whatever the pt (the default: the reference's behaviour)
//   WMX_CODEC_PCMA      1    g711 && pt == 8               A-law
//   WMX_CODEC_PCMU      2    g711 && pt == 0               mu-law
//   WMX_CODEC_BY_PT     3    g711                          mu-law if pt == 0, else A-law
//
//   refused = arrived && !call, in every mode: telephone-event packets, the AAC tag, the other law on a strict leg.
//
// A refused slot is what a slot of another payload type has always been: d_len = 0 and a zeroed PCM row (d_seq_raw is still written
// where something arrived).  Everything downstream goes by d_len, so a refused packet is invisible to the sequence rule (leg_seq.h:
// it is not late, not a duplicate, does not sync a leg and, having consumed a sequence number, shows up there as a gap), to talker
// selection (a zeroed row has no level) and to the load (no call: the leg's cursor does not move).
//
// Send side: out_law WMX_LAW_A is payload type 8 and PCM2G711a, WMX_LAW_U payload type 0 and PCM2G711u (src/rtp.h:21-24).
//
// Plain C++ without HIP types: rtp.hip includes it for the device, tests/test_leg_codec_host.py compiles it with g++ beside a model
// written from the table above.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define WMX_CODEC_FN __host__ __device__ inline
#else
#define WMX_CODEC_FN inline
#endif

namespace wmx {

constexpr uint32_t kCodecReference = 0, kCodecPcma = 1, kCodecPcmu = 2, kCodecByPt = 3;  // WMX_CODEC_* (include/wmix_amd.h)
constexpr uint32_t kLegCodecCall = 1u, kLegCodecUlaw = 2u, kLegCodecRefused = 4u;        // leg_codec_slot's answer
constexpr int kLawA = 0, kLawU = 1;                                                       // WMX_LAW_*

WMX_CODEC_FN bool leg_codec_valid(int in_codec) { return in_codec >= 0 && in_codec <= (int)kCodecByPt; }
WMX_CODEC_FN bool leg_law_valid(int law) { return law == kLawA || law == kLawU; }

// One datagram slot.  pt is read only where something arrived.  -> kLegCodecCall | kLegCodecUlaw (a call only) | kLegCodecRefused
WMX_CODEC_FN uint32_t leg_codec_slot(bool arrived, uint32_t pt, uint32_t in_codec) {
    const bool g711 = arrived && (pt == 8u || pt == 0u);  // src/rtp.c:88-95
    const bool call = g711 && (in_codec == kCodecPcma ? pt == 8u : (in_codec == kCodecPcmu ? pt == 0u : true));
    const bool ulaw = call && pt == 0u && (in_codec == kCodecPcmu || in_codec == kCodecByPt);
    return (call ? kLegCodecCall : 0u) | (ulaw ? kLegCodecUlaw : 0u) | (arrived && !call ? kLegCodecRefused : 0u);
}

// RTP_PAYLOAD_TYPE_PCMA / PCMU of what a leg is sent
WMX_CODEC_FN uint32_t leg_codec_out_pt(int out_law) { return out_law == kLawA ? 8u : 0u; }

}  // namespace wmx
