// speakers.h -- the rule behind wmx_mix_select_speakers / wmx_mix_select_speakers_conf (mix.hip) and wmx_tick_bridge_speakers
// (tick.hip): of the legs of a conference, only the loudest `max_speakers` are loaded into the others' rings.
//
// Integer and exact.  Per ring r the mixer keeps one uint32 envelope env[r], zero at first.  One call with max_speakers in
// 1 .. WMX_MIX_MAX_PARTIES, floor and decay_shift in 0 .. 31 does, for the member at list position p (ring r) of a conference of at
// least 2 members:
//   level    = sum of |x| over the srcU8Len / 2 int16 elements of the leg's source row as they lie there (all channels, before the
//              resampling and the reduce division); |-32768| = 32768; uint32, which kSpeakersMaxElements elements cannot overflow
//   env'     = max(level, env - (env >> decay_shift)), stored for every member, the host-muted ones too (a leg that is unmuted in
//              the middle of a sentence is selected at once); shift 0 holds nothing
//   eligible = !host_mute[r] && env' >= floor
//   rank     = the number of eligible members s of the same conference with env'[s] > env'[p], or env'[s] == env'[p] and s < p:
//              a tie goes to the earlier LIST position, not to the lower ring index
//   speaking = eligible && rank < max_speakers;   mute_out = !speaking
// Every other ring -- in no conference, or in one of 0 or 1 members -- gets speaking = 0, mute_out = 1 and keeps its env.
//
// Plain C++ without HIP types: mix.hip includes it for the kernel (which calls the element functions below from its lanes),
// tests/test_speakers_host.py compiles it with g++ and compares speakers_conference with a numpy model (tests/speakers_model.py).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define WMX_SPK_FN __host__ __device__ inline
#else
#define WMX_SPK_FN inline
#endif

namespace wmx {

constexpr int kSpeakersMaxParties = 32;  // WMX_MIX_MAX_PARTIES (include/wmix_amd.h)
// the longest row whose level fits uint32 when every element is -32768
constexpr uint32_t kSpeakersMaxElements = UINT32_MAX / 32768u;

WMX_SPK_FN bool speakers_params_ok(int max_speakers, int decay_shift) {
    return max_speakers >= 1 && max_speakers <= kSpeakersMaxParties && decay_shift >= 0 && decay_shift <= 31;
}
WMX_SPK_FN bool speakers_len_ok(uint32_t srcU8Len) { return srcU8Len / 2 <= kSpeakersMaxElements; }

WMX_SPK_FN uint32_t speakers_abs16(int16_t x) { return x < 0 ? (uint32_t)(-(int32_t)x) : (uint32_t)x; }

WMX_SPK_FN uint32_t speakers_level(const int16_t *row, uint32_t n_elements) {
    uint32_t level = 0;
    for (uint32_t i = 0; i < n_elements; i++) level += speakers_abs16(row[i]);
    return level;
}

WMX_SPK_FN uint32_t speakers_env_next(uint32_t env, uint32_t level, int decay_shift) {
    const uint32_t held = env - (env >> decay_shift);
    return level > held ? level : held;
}

WMX_SPK_FN bool speakers_eligible(bool host_muted, uint32_t env_next, uint32_t floor) { return !host_muted && env_next >= floor; }

// does member s (envelope env_s) come before member p in the ranking?  s and p are list positions
WMX_SPK_FN bool speakers_outranks(uint32_t env_s, int s, uint32_t env_p, int p) { return env_s > env_p || (env_s == env_p && s < p); }

// One conference of n members (2 .. kSpeakersMaxParties), position by position: level[p] and host_muted[p] in, env[p] in and out,
// speaking[p] out.  What the kernel's lanes compute side by side.
WMX_SPK_FN void speakers_conference(int n, const uint32_t *level, const uint8_t *host_muted, uint32_t *env, int max_speakers, uint32_t floor,
                                    int decay_shift, uint8_t *speaking) {
    for (int p = 0; p < n; p++) env[p] = speakers_env_next(env[p], level[p], decay_shift);
    for (int p = 0; p < n; p++) {
        int rank = 0;
        for (int s = 0; s < n; s++)
            if (speakers_eligible(host_muted[s] != 0, env[s], floor) && speakers_outranks(env[s], s, env[p], p)) rank++;
        speaking[p] = speakers_eligible(host_muted[p] != 0, env[p], floor) && rank < max_speakers;
    }
}

// One whole call over a layout (bridge_layout.h: conference c = members[off[c] .. off[c + 1]), ring indices; at most
// kSpeakersMaxParties each), sequentially: the source row of ring r at rows + r * row_stride, host_mute NULL or by ring, env in and
// out, speaking and mute_out out (all by ring, n_groups entries).  The reference the device is compared with.
inline void speakers_step(int n_groups, int n_conf, const int32_t *off, const int32_t *members, const int16_t *rows, long row_stride,
                          uint32_t n_elements, const uint8_t *host_mute, int max_speakers, uint32_t floor, int decay_shift, uint32_t *env,
                          uint8_t *speaking, uint8_t *mute_out) {
    for (int r = 0; r < n_groups; r++) speaking[r] = 0, mute_out[r] = 1;
    for (int c = 0; c < n_conf; c++) {
        const int n = off[c + 1] - off[c];
        if (n < 2 || n > kSpeakersMaxParties) continue;
        const int32_t *mem = members + off[c];
        uint32_t level[kSpeakersMaxParties], e[kSpeakersMaxParties];
        uint8_t muted[kSpeakersMaxParties], sp[kSpeakersMaxParties];
        for (int p = 0; p < n; p++) {
            level[p] = speakers_level(rows + (long)mem[p] * row_stride, n_elements);
            e[p] = env[mem[p]];
            muted[p] = host_mute && host_mute[mem[p]];
        }
        speakers_conference(n, level, muted, e, max_speakers, floor, decay_shift, sp);
        for (int p = 0; p < n; p++) env[mem[p]] = e[p], speaking[mem[p]] = sp[p], mute_out[mem[p]] = !sp[p];
    }
}

// ---- legs that deliver 0 .. max_packets packets in a tick (wmx_mix_select_speakers_legs, in front of wmx_mix_load_minus_legs)
// The rule above with one change: slot k of a leg is a call if and only if len[k] == srcU8Len, and
//   level = the maximum, over the slots of the leg that are calls, of speakers_level(row of that slot); no call this tick: 0
// so a leg whose slot 0 is a hole and whose packet sits in a later slot is as loud as its packet.  `rows`: the leg's slot 0, slot k
// packet_stride int16 elements behind it; `len`: the leg's max_packets entries.
constexpr int kSpeakersMaxLegPackets = 4;  // WMX_MIX_MAX_LEG_PACKETS (include/wmix_amd.h)

WMX_SPK_FN uint32_t speakers_level_legs(const int16_t *rows, long packet_stride, int max_packets, const uint32_t *len, uint32_t srcU8Len) {
    uint32_t level = 0;
    for (int k = 0; k < max_packets; k++) {
        if (len[k] != srcU8Len) continue;
        const uint32_t l = speakers_level(rows + (long)k * packet_stride, srcU8Len / 2);
        level = l > level ? l : level;
    }
    return level;
}

// speakers_step for such legs: slot k of ring r at rows + r * source_stride + k * packet_stride, len[r * max_packets + k]
inline void speakers_step_legs(int n_groups, int n_conf, const int32_t *off, const int32_t *members, const int16_t *rows, long source_stride,
                               long packet_stride, int max_packets, const uint32_t *len, uint32_t srcU8Len, const uint8_t *host_mute,
                               int max_speakers, uint32_t floor, int decay_shift, uint32_t *env, uint8_t *speaking, uint8_t *mute_out) {
    for (int r = 0; r < n_groups; r++) speaking[r] = 0, mute_out[r] = 1;
    for (int c = 0; c < n_conf; c++) {
        const int n = off[c + 1] - off[c];
        if (n < 2 || n > kSpeakersMaxParties) continue;
        const int32_t *mem = members + off[c];
        uint32_t level[kSpeakersMaxParties], e[kSpeakersMaxParties];
        uint8_t muted[kSpeakersMaxParties], sp[kSpeakersMaxParties];
        for (int p = 0; p < n; p++) {
            level[p] = speakers_level_legs(rows + (long)mem[p] * source_stride, packet_stride, max_packets, len + (long)mem[p] * max_packets, srcU8Len);
            e[p] = env[mem[p]];
            muted[p] = host_mute && host_mute[mem[p]];
        }
        speakers_conference(n, level, muted, e, max_speakers, floor, decay_shift, sp);
        for (int p = 0; p < n; p++) env[mem[p]] = e[p], speaking[mem[p]] = sp[p], mute_out[mem[p]] = !sp[p];
    }
}

}  // namespace wmx
