// mix.hip -- wmix's resample + saturating-mix arithmetic, batched for gfx950.
//
// Replaces wmix_pcm_zoom / wmix_len_of_out / wmix_len_of_in (src/wmix.c:49-222) and the arithmetic of
// wmix_load_data + volumeAdd (src/wmix.c:1617-1957) for many independent mix groups per launch.
//
// Both reference routines drive their source/destination cursors with a float32 phase accumulator
// (`divStep += div; if ((int)divStep > 0) ... divStep -= 1.0`, `divCount += divPow; if (divCount >= 1.0)`)
// that depends only on the two rates and the length, never on the samples.  The host therefore runs the
// SAME float recurrence once per call and emits a gather schedule (one entry per destination sample);
// the kernels are pure HBM-streaming gathers: zoom = copy through the schedule, load = gather (+ the
// reference's linear "repair" fill when up-sampling) / reduce, then volumeAdd (a saturating add) into the
// group's 1 s ring.  All sources of a group are applied by the same thread in call order, so the
// order-dependent saturation (src/wmix.c:1617-1636) is reproduced without atomics.  Bit-exact.
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>
#include "legacy_stage.h"
#include "../../include/wmix_compat.h"
#include "mix_sched.h"
#include "mix_minus.h"
#include "bridge_layout.h"
#include "speakers.h"
#include "leg_cursor.h"
#include "leg_prompt.h"
#include "leg_state.h"

namespace wmx {
namespace {

static_assert(kLegMaxCalls == WMX_MIX_MAX_LEG_PACKETS, "leg_calls.h and include/wmix_amd.h name one limit");

// ---------------------------------------------------------------- kernels
__global__ __launch_bounds__(256) void zoom_kernel(const int16_t *__restrict__ in, int16_t *__restrict__ out,
                                                   const int32_t *__restrict__ idx, uint32_t n_out, long in_stride, long out_stride,
                                                   int n_streams) {
    const size_t total = (size_t)n_out * n_streams;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const uint32_t i = (uint32_t)(t % n_out);
        const size_t s = t / n_out;
        out[s * out_stride + i] = in[s * in_stride + idx[i]];
    }
}

__device__ __forceinline__ int16_t volume_add(int16_t a, int16_t b) {  // src/wmix.c:1617-1636
    if (a == 0) return b;
    if (b == 0) return a;
    const int32_t s = (int32_t)a + b;
    return (int16_t)(s < -32768 ? -32768 : (s > 32767 ? 32767 : s));
}

// one schedule entry evaluated for one source: the sample itself, or the reference's linear "repair" fill when up-sampling
__device__ __forceinline__ int16_t load_entry_value(const int16_t *__restrict__ p, const LoadEntry e, int rdce) {
    int16_t v;
    if (e.k < 0) {
        v = p[e.src];
    } else {
        // repairBuff[k] = prev + (k+1 times accumulated) step, float adds in the reference's order
        const int16_t prev = p[e.src - e.step];
        const float st = (float)((int)p[e.src] - (int)prev) / (float)e.n2;
        float sum = st;
        for (int j = 0; j < e.k; j++) sum += st;
        v = (int16_t)((float)prev + sum);
    }
    return (int16_t)(v / rdce);
}

// one thread = one ring sample of one group; all `n_src` sources are accumulated in order
__global__ __launch_bounds__(256) void load_kernel(int16_t *__restrict__ rings, uint32_t ring_samples, const int16_t *__restrict__ src,
                                                   const LoadEntry *__restrict__ sch, uint32_t n_out, uint32_t head_sample, int n_src,
                                                   long group_stride, long source_stride, int rdce, int n_groups) {
    const size_t total = (size_t)n_out * n_groups;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const uint32_t i = (uint32_t)(t % n_out);
        const size_t g = t / n_out;
        const LoadEntry e = sch[i];
        uint32_t pos = head_sample + i;
        pos -= (pos >= ring_samples) ? ring_samples * (pos / ring_samples) : 0;
        int16_t *dst = rings + g * (size_t)ring_samples + pos;
        int16_t acc = *dst;
        const int16_t *sg = src + g * group_stride;
        for (int s = 0; s < n_src; s++) acc = volume_add(acc, load_entry_value(sg + (size_t)s * source_stride, e, rdce));
        *dst = acc;
    }
}

__global__ __launch_bounds__(256) void drain_kernel(int16_t *__restrict__ rings, uint32_t ring_samples, int16_t *__restrict__ out,
                                                    uint32_t n, uint32_t head_sample, long out_stride, int n_groups) {
    const size_t total = (size_t)n * n_groups;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const uint32_t i = (uint32_t)(t % n);
        const size_t g = t / n;
        uint32_t pos = head_sample + i;
        pos -= (pos >= ring_samples) ? ring_samples * (pos / ring_samples) : 0;
        int16_t *src = rings + g * (size_t)ring_samples + pos;
        out[g * out_stride + i] = *src;
        *src = 0;  // the play thread zeroes what it has read (src/wmix.c:1351-1352)
    }
}

// The two sweeps of the bridge load (mix_minus.h) over one ring-sample column of a conference of n members: the same sample position
// in the members' rings.  Every source is evaluated ONCE.  Forward sweep: y[q] = F_q(ring_q) with the running prefix map; backward
// sweep: ring_q = G_q(y[q]) with the running suffix map.  PMAX is the compile-time bound that keeps c[] and y[] in registers (fully
// unrolled, `q < n` predicates): no scratch.  load_minus_conf_kernel keeps a copy of the sweeps (see there).  ring(q): the address of member q's sample in this column.  value(q, c): sets c to what
// source q adds and returns true, or returns false and leaves the 0 -- a muted source, or one that does not cover the column, adds 0,
// which is what not calling wmix_load_data for it leaves.  SKIP_EMPTY: a column for which every value() returned false is not written.
// DUCK: member q with bit q of `ducked` set is not written -- its ring is duck_fold_kernel's this tick (leg_prompt.h, REDUCE); its
// source counts for everybody else as ever.
// The kernels' closures capture BY VALUE and are taken by reference here: with reference captures the compiler no longer hoists the
// schedule entry's per-column arithmetic out of the sweep (5 % more instructions, 2 % more time on 65 536 conferences of 8).
template <int PMAX, bool SKIP_EMPTY, bool DUCK = false, class Ring, class Value>
__device__ __forceinline__ void minus_sweeps(int n, const Ring &ring, const Value &value, uint32_t ducked = 0u) {
    int c[PMAX], y[PMAX];
    bool any = false;
    ClampMap f = clamp_map_identity();
#pragma unroll
    for (int q = 0; q < PMAX; q++) {
        c[q] = 0;
        y[q] = 0;
        if (q < n) {
            any |= value(q, c[q]);
            y[q] = clamp_map_apply(f, *ring(q));
            f = clamp_map_then_add(f, (int16_t)c[q]);
        }
    }
    if (SKIP_EMPTY && !any) return;
    ClampMap g = clamp_map_identity();
#pragma unroll
    for (int q = PMAX - 1; q >= 0; q--) {
        if (q < n) {
            if (!DUCK || !((ducked >> q) & 1u)) *ring(q) = clamp_map_apply(g, (int16_t)y[q]);
            g = clamp_map_add_then((int16_t)c[q], g);
        }
    }
}

// The bridge load: one thread = one ring-sample column of one conference, the `parties` consecutive rings of that conference.
template <int PMAX>
__global__ __launch_bounds__(256) void load_minus_kernel(int16_t *__restrict__ rings, uint32_t ring_samples, const int16_t *__restrict__ src,
                                                         const LoadEntry *__restrict__ sch, uint32_t n_out, uint32_t head_sample, int parties,
                                                         long conf_stride, long source_stride, const uint8_t *__restrict__ mute, int rdce,
                                                         int n_conf) {
    const size_t total = (size_t)n_out * n_conf;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const uint32_t i = (uint32_t)(t % n_out);
        const size_t conf = t / n_out;
        const LoadEntry e = sch[i];
        uint32_t pos = head_sample + i;
        pos -= (pos >= ring_samples) ? ring_samples * (pos / ring_samples) : 0;
        int16_t *col = rings + conf * (size_t)parties * ring_samples + pos;
        const int16_t *sc = src + conf * conf_stride;
        const uint8_t *mc = mute ? mute + conf * (size_t)parties : nullptr;
        minus_sweeps<PMAX, false>(
            parties, [=](int q) { return col + (size_t)q * ring_samples; },
            [=](int q, int &c) {
                if (mc && mc[q]) return false;
                c = load_entry_value(sc + (size_t)q * source_stride, e, rdce);
                return true;
            });
    }
}

// The bridge load over a layout (bridge_layout.h): the ring and source addresses are taken from the member list.  One thread = one
// ring-sample column of one conference of this size class (`tab`: {offset into members, size} per slot;
// `lead`: the slot's start column relative to base_sample).  A slot's columns are dealt out in whole waves (n_pad = n_out rounded up to
// the wave, the lanes past n_out idle), so the slot is wave-uniform: the table entry, the member indices and the mute bytes are scalar
// loads and the ring / source bases scalar arithmetic.  The members of a conference are distinct rings and a ring is in one conference
// only (bridge_layout_build), so no two threads touch the same ring sample.
// This kernel writes minus_sweeps' two sweeps out itself: through the shared function its 32-wide instantiation compiled to 86 VGPRs
// for 84 and measured 0.6 - 0.9 % slower on 16 384 conferences of 32 (DESIGN_HISTORY.md); the other two kernels lose nothing.
template <int PMAX>
__global__ __launch_bounds__(256) void load_minus_conf_kernel(int16_t *__restrict__ rings, uint32_t ring_samples, const int16_t *__restrict__ src,
                                                              const LoadEntry *__restrict__ sch, uint32_t n_out, uint32_t n_pad,
                                                              uint32_t base_sample, const int32_t *__restrict__ tab,
                                                              const uint32_t *__restrict__ lead, const int32_t *__restrict__ members,
                                                              long source_stride, const uint8_t *__restrict__ mute, int rdce, int n_slots) {
    const size_t total = (size_t)n_pad * n_slots;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const uint32_t i = (uint32_t)(t % n_pad);
        // n_pad, the block and the grid's stride are multiples of the wave: every lane of a wave computes the same slot
        const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t / n_pad));
        if (i >= n_out) continue;
        const LoadEntry e = sch[i];
        uint32_t pos = base_sample + lead[slot] + i;  // each of the three < ring_samples
        pos -= (pos >= ring_samples) ? ring_samples * (pos / ring_samples) : 0;
        const int32_t *mem = members + tab[2 * (size_t)slot];
        const int n = tab[2 * (size_t)slot + 1];
        int c[PMAX], y[PMAX];
        ClampMap f = clamp_map_identity();
#pragma unroll
        for (int q = 0; q < PMAX; q++) {
            c[q] = 0;
            y[q] = 0;
            if (q < n) {
                const size_t r = (size_t)mem[q];
                if (!mute || !mute[r]) c[q] = load_entry_value(src + r * source_stride, e, rdce);
                y[q] = clamp_map_apply(f, rings[r * ring_samples + pos]);
                f = clamp_map_then_add(f, (int16_t)c[q]);
            }
        }
        ClampMap g = clamp_map_identity();
#pragma unroll
        for (int q = PMAX - 1; q >= 0; q--) {
            if (q < n) {
                rings[(size_t)mem[q] * ring_samples + pos] = clamp_map_apply(g, (int16_t)y[q]);
                g = clamp_map_add_then((int16_t)c[q], g);
            }
        }
    }
}

// ---- talker selection (speakers.h)
__device__ __forceinline__ uint32_t abs_sum_pair(uint32_t w) { return speakers_abs16((int16_t)(w & 0xffffu)) + speakers_abs16((int16_t)(w >> 16)); }

// the rings the selection kernel does not visit: nobody speaks there
__global__ __launch_bounds__(256) void speakers_clear_kernel(uint8_t *__restrict__ speaking, uint8_t *__restrict__ mute_out, int n_groups) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n_groups; r += gridDim.x * blockDim.x) {
        speaking[r] = 0;
        mute_out[r] = 1;
    }
}

// the part of a row's level that lane `sub` of the L lanes dealt to the row sums: the elements in front of the first
// 16-byte boundary and behind the last one singly, the rest as 16-byte loads, so a row that is not aligned (source_stride is the
// caller's) is read the same way, and every element once over the L lanes
__device__ __forceinline__ uint32_t abs_sum_part(const int16_t *__restrict__ row, uint32_t n_el, uint32_t sub, uint32_t L) {
    uint32_t sum = 0;
    uint32_t head = (8u - (uint32_t)(((uintptr_t)row & 15u) >> 1)) & 7u;  // elements in front of the 16-byte boundary
    if (head > n_el) head = n_el;
    const uint32_t body = (n_el - head) / 8;  // whole 16-byte pieces, none past the row's end
    for (uint32_t i = sub; i < head; i += L) sum += speakers_abs16(row[i]);
    const uint4 *v = reinterpret_cast<const uint4 *>(row + head);
    for (uint32_t c = sub; c < body; c += L) {
        const uint4 x = v[c];
        sum += abs_sum_pair(x.x) + abs_sum_pair(x.y) + abs_sum_pair(x.z) + abs_sum_pair(x.w);
    }
    for (uint32_t i = head + body * 8 + sub; i < n_el; i += L) sum += speakers_abs16(row[i]);
    return sum;
}

// Lane p = member p, for the whole wave outside every divergent branch (a ballot and lane reads): the member's env' from its level
// (speakers.h), the rank from the n envelopes read lane by lane, and the three stores to ring r.  A lane that is no member brings
// nothing and stores nothing.
template <class RingOf>
__device__ __forceinline__ void speakers_rank_store(bool member, const RingOf &ring_of, uint32_t level, int n, int lane, const uint8_t *__restrict__ mute,
                                                    int max_speakers, uint32_t floor, int decay_shift, uint32_t *__restrict__ env,
                                                    uint8_t *__restrict__ speaking, uint8_t *__restrict__ mute_out) {
    size_t r = 0;
    uint32_t e = 0;
    bool eligible = false;
    if (member) {
        r = ring_of();
        e = speakers_env_next(env[r], level, decay_shift);
        eligible = speakers_eligible(mute && mute[r], e, floor);
    }
    const unsigned long long eligible_lanes = __ballot(eligible);
    int rank = 0;
    for (int s = 0; s < n; s++) {  // s is wave-uniform: a lane read, no LDS traffic
        const uint32_t es = (uint32_t)__builtin_amdgcn_readlane((int)e, s);
        rank += ((eligible_lanes >> s) & 1ull) && speakers_outranks(es, s, e, lane);
    }
    if (member) {
        const bool sp = eligible && rank < max_speakers;
        env[r] = e;
        speaking[r] = sp ? 1 : 0;
        mute_out[r] = sp ? 0 : 1;
    }
}

// One wave = one conference (a slot of the layout when `tab` is given, else `parties` consecutive rings), the workgroup's waves on
// conferences of their own.  The wave's lanes are dealt out to the members, L = the largest power of two with n * L <= 64 lanes each
// (32 for a two-party call, 2 for 32 legs): the L lanes of a member stride its source row (abs_sum_part) and an xor-shuffle over the
// L lanes gives the row's level.  Then lane p is member p (speakers_rank_store).  No LDS, no atomics.
__global__ __launch_bounds__(256) void select_speakers_kernel(const int16_t *__restrict__ src, uint32_t n_el, int parties, long conf_stride,
                                                              long source_stride, const int32_t *__restrict__ tab,
                                                              const int32_t *__restrict__ members, const uint8_t *__restrict__ mute,
                                                              int max_speakers, uint32_t floor, int decay_shift, uint32_t *__restrict__ env,
                                                              uint8_t *__restrict__ speaking, uint8_t *__restrict__ mute_out, int n_slots) {
    const int lane = (int)(threadIdx.x & 63u), waves = (int)(blockDim.x >> 6);
    for (int w = (int)blockIdx.x * waves + (int)(threadIdx.x >> 6); w < n_slots; w += (int)gridDim.x * waves) {
        const int slot = __builtin_amdgcn_readfirstlane(w);  // the conference is wave-uniform: the table entry is a scalar load
        const int32_t *mem = tab ? members + tab[2 * (size_t)slot] : nullptr;
        const int n = tab ? tab[2 * (size_t)slot + 1] : parties;  // 2 .. 32
        int shift = 5;  // log2 of L
        while ((n << shift) > 64) shift--;
        const int L = 1 << shift, q = lane >> shift, sub = lane & (L - 1);
        uint32_t sum = 0;
        if (q < n) {
            const int16_t *row = mem ? src + (size_t)mem[q] * source_stride : src + (size_t)slot * conf_stride + (size_t)q * source_stride;
            sum = abs_sum_part(row, n_el, (uint32_t)sub, (uint32_t)L);
        }
        for (int o = L >> 1; o > 0; o >>= 1) sum += (uint32_t)__shfl_xor((int)sum, o);
        // lane p = member p
        const uint32_t level = (uint32_t)__shfl((int)sum, (lane << shift) & 63);
        const bool member = lane < n;
        speakers_rank_store(member, [=] { return mem ? (size_t)mem[lane] : (size_t)slot * parties + lane; }, level, n, lane, mute, max_speakers,
                            floor, decay_shift, env, speaking, mute_out);
    }
}

// Talker selection over leg packets (speakers.h: speakers_level_legs): select_speakers_kernel's dealing -- one wave = one conference
// of the layout, L lanes per member -- with the level taken over the leg's slots.  The L lanes of a member read which of its slots are
// calls (len == srcU8Len; the same words in every lane of the member), stride the rows of those slots only, and an xor-shuffle per
// slot gives that slot's level; the largest is the leg's.  The shuffles run outside every branch: a lane whose slot is no call brings
// 0.  Then lane p is member p, as there.  Rings outside every conference of two or more members are the clear kernel's.
__global__ __launch_bounds__(256) void select_speakers_legs_kernel(const int16_t *__restrict__ src, uint32_t n_el, uint32_t srcU8Len,
                                                                   long source_stride, long packet_stride, int max_packets,
                                                                   const uint32_t *__restrict__ len, const int32_t *__restrict__ tab,
                                                                   const int32_t *__restrict__ members, const uint8_t *__restrict__ mute,
                                                                   int max_speakers, uint32_t floor, int decay_shift, uint32_t *__restrict__ env,
                                                                   uint8_t *__restrict__ speaking, uint8_t *__restrict__ mute_out, int n_groups,
                                                                   int n_slots) {
    const int lane = (int)(threadIdx.x & 63u), waves = (int)(blockDim.x >> 6);
    for (int w = (int)blockIdx.x * waves + (int)(threadIdx.x >> 6); w < n_slots; w += (int)gridDim.x * waves) {
        const int slot = __builtin_amdgcn_readfirstlane(w);
        const int32_t *mem = members + tab[2 * (size_t)slot];
        int n = tab[2 * (size_t)slot + 1];  // 2 .. 32
        n = n < 0 ? 0 : (n > kBridgeMaxParties ? kBridgeMaxParties : n);
        int shift = 5;  // log2 of L
        while ((n << shift) > 64) shift--;
        const int L = 1 << shift, q = lane >> shift, sub = lane & (L - 1);
        uint32_t sum[kLegMaxCalls];
#pragma unroll
        for (int k = 0; k < kLegMaxCalls; k++) sum[k] = 0;
        if (q < n) {
            const int32_t ri = mem[q];
            if (ri >= 0 && ri < n_groups) {
                const int16_t *rows = src + (size_t)ri * source_stride;
#pragma unroll
                for (int k = 0; k < kLegMaxCalls; k++)
                    if (k < max_packets && len[(size_t)ri * max_packets + k] == srcU8Len)
                        sum[k] = abs_sum_part(rows + (size_t)k * packet_stride, n_el, (uint32_t)sub, (uint32_t)L);
            }
        }
        uint32_t best = 0;
#pragma unroll
        for (int k = 0; k < kLegMaxCalls; k++) {
            uint32_t s = sum[k];
            for (int o = L >> 1; o > 0; o >>= 1) s += (uint32_t)__shfl_xor((int)s, o);
            best = s > best ? s : best;
        }
        // lane p = member p
        const uint32_t level = (uint32_t)__shfl((int)best, (lane << shift) & 63);
        const int32_t rl = lane < n ? mem[lane] : -1;
        const bool member = rl >= 0 && rl < n_groups;
        speakers_rank_store(member, [=] { return (size_t)rl; }, level, n, lane, mute, max_speakers, floor, decay_shift, env, speaking,
                            mute_out);
    }
}

// ---- a cursor per leg (leg_cursor.h)
// What the cursor kernel leaves for the load kernels.  Per ring: where the calls its leg makes in this launch start (a ring sample,
// reduced into the ring), how many ring samples they cover (0: none, or muted), and the slot each came from.  Per layout slot: the
// conference's window, from the earliest start to the latest end among its members, relative to the play head.
struct LegSpanEntry {
    uint32_t start, len, slots, pad;
};

// One wave = one conference of the layout, lane p = member p (select_speakers_kernel's dealing).  The lane reads which of its leg's
// slots are calls (d_len), applies the rule (at most WMX_MIX_MAX_LEG_PACKETS steps) and writes the span, the new cursor and the drop
// count; an xor-shuffle over the wave gives the window.  Rings outside every conference of two or more members are not visited:
// their cursors stay.  A cursor read from memory never indexes anything as it is: the span's start is reduced into the ring here.
// CALLS (wmx_mix_load_minus_legs_calls): the leg's calls are those of its call list (leg_calls.h), in list order, instead of its valid
// slots in slot order; a data call that names a slot that is not readable (d_len) is made with zeros, and the span's pad carries the
// silence mask of the calls made.
template <bool CALLS>
__global__ __launch_bounds__(256) void leg_cursor_kernel(const int32_t *__restrict__ tab, const int32_t *__restrict__ members,
                                                         const uint32_t *__restrict__ len, uint32_t srcU8Len, int max_packets,
                                                         const uint8_t *__restrict__ mute, LegMixState ms, uint32_t n_out,
                                                         uint32_t *__restrict__ head, uint32_t *__restrict__ tick,
                                                         uint32_t *__restrict__ dropped, LegSpanEntry *__restrict__ span,
                                                         uint2 *__restrict__ win, int n_groups, int n_slots,
                                                         const uint32_t *__restrict__ calls) {
    const int lane = (int)(threadIdx.x & 63u), waves = (int)(blockDim.x >> 6);
    const uint32_t ring_samples = ms.ring_bytes / 2, head_sample = (ms.head_off / 2) % ring_samples;
    for (int w = (int)blockIdx.x * waves + (int)(threadIdx.x >> 6); w < n_slots; w += (int)gridDim.x * waves) {
        const int slot = __builtin_amdgcn_readfirstlane(w);
        const int32_t *mem = members + tab[2 * (size_t)slot];
        int n = tab[2 * (size_t)slot + 1];
        n = n < 0 ? 0 : (n > kBridgeMaxParties ? kBridgeMaxParties : n);
        uint32_t lo = UINT32_MAX, hi = 0;  // the window in samples behind the play head: [lo, hi)
        if (lane < n) {
            const int32_t r = mem[lane];
            if (r >= 0 && r < n_groups) {
                uint32_t valid = 0;
                for (int k = 0; k < kLegMaxCalls; k++)
                    if (k < max_packets && len[(size_t)r * max_packets + k] == srcU8Len) valid |= 1u << k;
                uint32_t list = 0, silence = 0;
                if (CALLS) {
                    list = calls[r];
                    const uint32_t n_calls = leg_calls_walked(list);
                    for (uint32_t j = 0; j < n_calls; j++)  // a data call whose slot's row is not readable: a call with zeros
                        if (!((valid >> leg_calls_slot(list, j)) & 1u)) list = leg_calls_set_silence(list, j);
                    valid = n_calls;
                }
                if (valid) {
                    LegSpan s;
                    if (CALLS) {
                        const LegSpanCalls sc = leg_cursor_span_calls(ms, n_out, LegCursor{head[r], tick[r]}, list);
                        s = sc.span;
                        silence = sc.silence;
                    } else {
                        s = leg_cursor_span(ms, n_out, LegCursor{head[r], tick[r]}, valid, max_packets);
                    }
                    head[r] = s.after.head;
                    tick[r] = s.after.tick;
                    if (s.dropped) dropped[r] += s.dropped;
                    LegSpanEntry e{(s.start / 2) % ring_samples, (mute && mute[r]) ? 0u : s.count * n_out, s.slots, silence};
                    span[r] = e;
                    if (e.len) {
                        lo = e.start >= head_sample ? e.start - head_sample : e.start + ring_samples - head_sample;
                        hi = lo + e.len;
                    }
                } else {
                    span[r] = LegSpanEntry{0u, 0u, 0u, 0u};
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t l2 = (uint32_t)__shfl_xor((int)lo, o), h2 = (uint32_t)__shfl_xor((int)hi, o);
            lo = l2 < lo ? l2 : lo;
            hi = h2 > hi ? h2 : hi;
        }
        if (lane == 0) {
            uint32_t wlen = hi > lo ? hi - lo : 0u;
            if (wlen > ring_samples) wlen = ring_samples;  // every ring column once
            uint32_t wstart = wlen ? head_sample + lo : 0u;
            wstart -= wstart >= ring_samples ? ring_samples : 0u;
            win[slot] = make_uint2(wstart, wlen);
        }
    }
}

// The bridge load with a cursor per leg: load_minus_conf_kernel's addressing, with each source's value looked up through its
// span.  One thread = one ring column of one conference of this size class; the columns are those of the conference's window.  A
// slot is dealt n_pad columns (whole waves, so the slot is wave-uniform and its table entry, window, member indices and spans are
// scalar loads); a window longer than that is walked in strides of n_pad, a wave whose first column lies behind the window's end
// exits.  A source whose span does not cover the column adds 0, which is what not calling wmix_load_data leaves; a column no
// source covers is not written.  A leg's span covers no ring sample twice (leg_cursor.h), a ring is in one conference only and a
// column is one thread's: no two threads touch the same ring sample.  CALLS: a call whose bit in the span's silence mask (pad) is set
// adds 0 like a source that does not cover the column.  DUCK (a tick in which a ring can be ducked under its prompt): the members in the
// slot's mask `duck` are not written here; duck_fold_kernel, in front of this launch, has filled their rings.  Without DUCK `duck` is
// not read.
template <int PMAX, bool CALLS, bool DUCK>
__global__ __launch_bounds__(256) void load_minus_legs_kernel(int16_t *__restrict__ rings, uint32_t ring_samples, const int16_t *__restrict__ src,
                                                              const LoadEntry *__restrict__ sch, uint32_t n_out, uint32_t n_pad,
                                                              const int32_t *__restrict__ tab, const uint2 *__restrict__ win,
                                                              const LegSpanEntry *__restrict__ span, const int32_t *__restrict__ members,
                                                              long source_stride, long packet_stride, int rdce, int n_groups, int n_slots,
                                                              const uint32_t *__restrict__ duck) {
    const size_t total = (size_t)n_pad * n_slots;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t / n_pad));
        const uint32_t ducked = DUCK ? duck[slot] : 0u;
        const uint2 w = win[slot];
        const uint32_t wstart = w.x < ring_samples ? w.x : 0u, wlen = w.y < ring_samples ? w.y : ring_samples;
        const int32_t *mem = members + tab[2 * (size_t)slot];
        int n = tab[2 * (size_t)slot + 1];
        n = n > PMAX ? PMAX : n;
        for (uint32_t col = (uint32_t)(t % n_pad); col < wlen; col += n_pad) {
            uint32_t pos = wstart + col;  // both < ring_samples
            pos -= pos >= ring_samples ? ring_samples : 0u;
            // a member index read from memory never addresses anything as it is
            auto ring_of = [=](int q) {
                const int32_t ri = mem[q];
                return (size_t)(ri >= 0 && ri < n_groups ? ri : 0);
            };
            minus_sweeps<PMAX, true, DUCK>(
                n, [=](int q) { return rings + ring_of(q) * ring_samples + pos; },
                [=](int q, int &c) {
                    const size_t r = ring_of(q);
                    const LegSpanEntry e = span[r];
                    const uint32_t st = e.start < ring_samples ? e.start : 0u;
                    const uint32_t d = pos >= st ? pos - st : pos + ring_samples - st;
                    if (d >= e.len || d >= (uint32_t)kLegMaxCalls * n_out) return false;
                    const uint32_t j = (d >= n_out) + (d >= 2 * n_out) + (d >= 3 * n_out);  // the call, 0 .. 3, and its sample
                    if (CALLS && ((e.pad >> j) & 1u)) return false;
                    const uint32_t k = (e.slots >> (2u * j)) & 3u;
                    c = load_entry_value(src + r * source_stride + (size_t)k * packet_stride, sch[d - j * n_out], rdce);
                    return true;
                },
                ducked);
        }
    }
}

// ---- a prompt per leg (leg_prompt.h)
// One wave = one leg, no loop over legs: the state entry is read before anything is stored, so it and the clip's table entry are
// wave-uniform (scalar) loads, and an idle leg's wave exits after the one load.  The rule's inputs are all wave-uniform, so the wave
// evaluates it once, on the scalar side; the lanes take the call's up to 160 ring samples -- ring[pos] = volumeAdd(ring[pos], clip[i]),
// with the ring's wrap -- and lane 0 writes the state back.  A clip index, an offset, a length or a cursor read from memory never
// addresses anything as it is: the index is held against the table, offset and length against the arena (a clip that does not fit has
// no samples, and the rule sets its leg idle), the call's start is reduced into the ring.  Ring g is touched by wave g alone.
// the clip a state entry names, held against the table and the arena: a clip that does not fit has no samples
__device__ __forceinline__ PromptClip prompt_clip_of(int32_t clip, const PromptClip *__restrict__ table, uint32_t n_clips, uint32_t arena_samples) {
    const bool known = clip >= 0 && (uint32_t)clip < n_clips;
    const PromptClip c = table[known ? (uint32_t)clip : 0u];
    const uint32_t off = c.off < arena_samples ? c.off : 0u;
    return PromptClip{off, known && c.off < arena_samples && c.samples <= arena_samples - off ? c.samples : 0u};
}

__global__ __launch_bounds__(256) void prompt_kernel(int16_t *__restrict__ rings, uint32_t ring_samples, LegPrompt *__restrict__ state,
                                                     const PromptClip *__restrict__ table, uint32_t n_clips,
                                                     const int16_t *__restrict__ arena, uint32_t arena_samples, LegMixState ms, int n_groups) {
    const uint32_t lane = threadIdx.x & 63u;
    const int g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    if (g >= n_groups) return;
    LegPrompt p = state[g];
    if (p.clip < 0) return;
    const PromptClip c = prompt_clip_of(p.clip, table, n_clips, arena_samples);
    const uint32_t off = c.off, samples = c.samples;
    const PromptCall call = leg_prompt_tick(ms, samples, p);
    const uint32_t start = (call.start / 2u) % ring_samples;
    const uint32_t n = call.n < (uint32_t)kLegRow ? call.n : (uint32_t)kLegRow;  // from + n <= samples (leg_prompt_tick)
    int16_t *ring = rings + (size_t)g * ring_samples;
    const int16_t *src = arena + off + call.from;
    for (uint32_t i = lane; i < n; i += 64u) {
        uint32_t pos = start + i;  // both < ring_samples
        pos -= pos >= ring_samples ? ring_samples : 0u;
        ring[pos] = volume_add(ring[pos], src[i]);
    }
    if (lane == 0u) state[g] = p;
}

// ---- the duck: the conference under a leg's prompt (leg_prompt.h, REDUCE)
// Launched in front of the DUCK form of load_minus_legs_kernel, behind leg_cursor_kernel, and only in a tick in which the host knows
// that some ring can be ducked.  One block of four waves = one conference of the layout, no loop over conferences.  First, in every
// wave, lane p = member p (leg_cursor_kernel's dealing) reads its leg's prompt entry and evaluates leg_prompt_ducks on it -- the state as
// the tick finds it: the prompts' step comes behind the load -- and a ballot makes the slot's mask of ducked members, which the first
// lane of the block leaves in duck[slot] for the sweeps, which then do not write those rings.  The mask is wave-uniform; a wave whose
// mask is empty exits there.  Otherwise a scalar loop runs over the ducked members g, the block's threads take the columns of the
// conference's window (a fold is a chain of dependent loads, so the columns are spread over the waves rather than walked by one), and
// per column a scalar loop runs over the members other than g in list order with the sweeps' own span / slot / silence-mask lookup:
//   x = ring_g[pos];  x = volumeAdd(x, c_s / rdce) for every s != g that covers the column;  ring_g[pos] = x, once, if any did
// with rdce = (reduce == D) ? 1 : D, the load's line (src/wmix.c:1675-1676) on a daemon whose reduceMode the play task holds at D.
// The divisor comes out of leg_prompt_divisor, 1 .. 16 whatever the entry holds; member and clip indices are held against n_groups and
// the table as everywhere.  Ring g's column is one lane's, ring g is in this conference only and the sweeps leave it alone: no two
// threads touch one ring sample.
__global__ __launch_bounds__(256) void duck_fold_kernel(int16_t *__restrict__ rings, uint32_t ring_samples, const int16_t *__restrict__ src,
                                                        const LoadEntry *__restrict__ sch, uint32_t n_out, const int32_t *__restrict__ tab,
                                                        const uint2 *__restrict__ win, const LegSpanEntry *__restrict__ span,
                                                        const int32_t *__restrict__ members, long source_stride, long packet_stride, int reduce,
                                                        const LegPrompt *__restrict__ state, const PromptClip *__restrict__ table,
                                                        uint32_t n_clips, uint32_t arena_samples, uint32_t *__restrict__ duck, int n_groups,
                                                        int n_slots) {
    const uint32_t lane = threadIdx.x & 63u;
    const int slot = (int)blockIdx.x;
    if (slot >= n_slots) return;
    const int32_t *mem = members + tab[2 * (size_t)slot];
    int n = tab[2 * (size_t)slot + 1];
    n = n < 0 ? 0 : (n > kBridgeMaxParties ? kBridgeMaxParties : n);
    uint32_t div = 1u;
    if ((int)lane < n) {
        const int32_t r = mem[lane];
        if (r >= 0 && r < n_groups) {
            const LegPrompt p = state[r];
            div = leg_prompt_ducks(p, prompt_clip_of(p.clip, table, n_clips, arena_samples).samples);
        }
    }
    const uint32_t mask = (uint32_t)__ballot(div > 1u);  // n <= 32: the lanes behind it bring 1
    if (threadIdx.x == 0u) duck[slot] = mask;
    if (!mask) return;
    const uint2 w = win[slot];
    const uint32_t wstart = w.x < ring_samples ? w.x : 0u, wlen = w.y < ring_samples ? w.y : ring_samples;
    // a member index read from memory never addresses anything as it is
    auto ring_of = [=](int q) {
        const int32_t ri = mem[q];
        return (size_t)(ri >= 0 && ri < n_groups ? ri : 0);
    };
    for (uint32_t rest = mask; rest; rest &= rest - 1u) {
        const int g = __builtin_ctz(rest);  // < n
        uint32_t D = (uint32_t)__builtin_amdgcn_readlane((int)div, g);
        D = D < 1u ? 1u : (D > kPromptMaxReduce + 1u ? kPromptMaxReduce + 1u : D);
        const int rdce = reduce == (int)D ? 1 : (int)D;
        int16_t *ring = rings + ring_of(g) * ring_samples;
        for (uint32_t col = threadIdx.x; col < wlen; col += blockDim.x) {
            uint32_t pos = wstart + col;  // both < ring_samples
            pos -= pos >= ring_samples ? ring_samples : 0u;
            int16_t x = ring[pos];
            bool any = false;
            for (int q = 0; q < n; q++) {
                if (q == g) continue;
                const size_t r = ring_of(q);
                const LegSpanEntry e = span[r];
                const uint32_t st = e.start < ring_samples ? e.start : 0u;
                const uint32_t d = pos >= st ? pos - st : pos + ring_samples - st;
                if (d >= e.len || d >= (uint32_t)kLegMaxCalls * n_out) continue;
                const uint32_t j = (d >= n_out) + (d >= 2 * n_out) + (d >= 3 * n_out);  // the call, 0 .. 3, and its sample
                if ((e.pad >> j) & 1u) continue;  // a silence call; without call lists the mask is 0
                const uint32_t k = (e.slots >> (2u * j)) & 3u;
                x = volume_add(x, load_entry_value(src + r * source_stride + (size_t)k * packet_stride, sch[d - j * n_out], rdce));
                any = true;
            }
            if (any) ring[pos] = x;
        }
    }
}

// play, stop and reset: `value` for the listed legs (NULL: every leg); keep_done: the leg's done count stays
__global__ __launch_bounds__(256) void prompt_set_kernel(LegPrompt *__restrict__ state, const int32_t *__restrict__ idx, int n, int n_groups,
                                                         LegPrompt value, int keep_done) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int r = idx ? idx[i] : i;
        if (r < 0 || r >= n_groups) continue;
        LegPrompt v = value;
        if (keep_done) v.done = state[r].done;
        state[r] = v;
    }
}

constexpr size_t kMappedMaxBytes = 64 * 1024;  // legacy staging (legacy_stage.h): above this the DMA engines win, the call is copied

}  // namespace

void zoom_gather_list(int inChn, int inFreq, uint32_t inLen, int outChn, int outFreq, std::vector<int32_t> &idx) {
    if (inChn == outChn && inFreq == outFreq) {
        idx.resize(inLen / 2);
        for (size_t i = 0; i < idx.size(); i++) idx[i] = (int32_t)i;
        return;
    }
    zoom_schedule((uint8_t)inChn, (uint16_t)inFreq, inLen, (uint8_t)outChn, (uint16_t)outFreq, idx);
}
}  // namespace wmx

struct wmx_mix {
    int device;  // the HIP device the state lives on (current device at create); every entry point switches to it
    int n_groups, chn, freq;
    uint32_t ring_bytes, head_off, tick, play_correct;
    uint8_t reduce_mode;
    int16_t *d_rings;
    uint8_t *h_rings = nullptr;  // set when the rings are pinned host memory mapped into the device (the legacy adapter's one ring)
    wmx::SchedCache sched;  // load schedules per source format, never rewritten (see SchedCache)
    std::vector<wmx::LoadEntry> sch;
    // wmx_mix_set_conferences: the layout, what the device holds of it (the member list, {offset, size} per slot, the leads), and
    // the host copies an upload in flight reads
    wmx::BridgeLayout conf;
    wmx::BridgeLeads conf_leads;
    std::vector<uint32_t> conf_next, h_conf_lead;
    int32_t *d_conf_members = nullptr, *d_conf_tab = nullptr;
    uint32_t *d_conf_lead = nullptr;
    size_t conf_cap_members = 0, conf_cap_slots = 0;
    // talker selection (speakers.h): one envelope and one speaking flag per ring, and a cursor per leg (leg_cursor.h): head, tick and the
    // drop count of every ring -- two tables (leg_state.h), each made by the first call that needs it
    wmx::LegState talkers, cursors;
    // what leg_cursor_kernel rewrites every tick for the load kernels, scratch and not state: the span table and the windows (one
    // zeroed block, made with the cursors)
    wmx::LegSpanEntry *d_leg_span = nullptr;
    uint2 *d_leg_win = nullptr;
    // the index list of prompt_set
    int32_t *d_prompt_idx = nullptr;
    size_t prompt_idx_cap = 0;
    // a prompt per leg (leg_prompt.h), made once by wmx_mix_prompts: one block -- the state entries in front, the clip table behind
    // them, the arena behind that -- and what the host knows of it
    wmx::LegPrompt *d_prompt = nullptr;
    wmx::PromptClip *d_clip_tab = nullptr;
    int16_t *d_clip_arena = nullptr;
    std::vector<wmx::PromptClip> clips;  // the clips added so far
    size_t clip_cap = 0, arena_cap = 0, arena_used = 0;  // clips; samples
    // Which launch of wmx_mix_load_prompts (counted in prompt_now) is the first that finds ring r idle for certain: an upper bound the
    // host keeps from what play, stop and reset were given (UINT64_MAX: an endless play).  A tick in which no ring can still be
    // playing launches nothing.
    std::vector<uint64_t> prompt_end;
    uint64_t prompt_now = 0, prompt_last = 0;  // prompt_last: the largest of prompt_end
    // The duck (leg_prompt.h, REDUCE): whether ring r's play was started with reduce > 0, and the largest prompt_end among those that
    // were.  Only a tick in front of it can find a ring ducked; every other tick's load of the legs is the plain one.  d_duck: the
    // mask of ducked members per layout slot, duck_fold_kernel's word to the sweeps; part of the store's block.
    std::vector<uint8_t> prompt_ducks;
    uint64_t duck_last = 0;
    uint32_t *d_duck = nullptr;
};

// rtp.hip's view of the mixer (wmx_rtp_egress_rings plays the rings itself) and wmx_mix_drain's bookkeeping for it
wmx::MixPlayView wmx::mix_play_view(const wmx_mix *m) {
    return MixPlayView{m->device, m->n_groups, m->chn, m->freq, m->ring_bytes, m->head_off, m->d_rings};
}
void wmx::mix_played(wmx_mix *m, uint32_t bytes) {
    m->head_off = (m->head_off + bytes) % m->ring_bytes;
    m->tick += bytes;
}

static wmx::BridgeMixState cursor_state(const wmx_mix *m) { return wmx::BridgeMixState{m->head_off, m->tick, m->play_correct, m->ring_bytes}; }

// The schedule of a source format, from the handle's cache or made and uploaded here, and wmx_mix_load's refusals.
static int load_sched(wmx_mix *m, const char *who, uint32_t srcU8Len, int freq, int channels, int sample, wmx::SchedCache::Entry **out) {
    using namespace wmx;
    const uint64_t k0 = ((uint64_t)srcU8Len << 32) | (uint32_t)freq, k1 = ((uint64_t)(uint8_t)channels << 8) | (uint8_t)sample;
    SchedCache::Entry *ent = m->sched.find(k0, k1);
    if (!ent) {
        if (!load_schedule(m->chn, m->freq, srcU8Len, (uint16_t)freq, (uint8_t)channels, (uint8_t)sample, m->sch)) {
            set_error("%s: rate ratio needs more than 64 fill samples (the reference overruns repairBuff here)", who);
            return WMX_EINVAL;
        }
        // More than one ring of output would make two threads of the launch read-modify-write the same ring sample (the
        // reference adds them one after the other); nothing in the daemon loads more than a few packets per call.
        if (m->sch.size() > m->ring_bytes / 2) {
            set_error("%s: %zu output samples do not fit the %u-sample ring in one call", who, m->sch.size(), m->ring_bytes / 2);
            return WMX_EINVAL;
        }
        const int rc = m->sched.add(k0, k1, m->sch.data(), m->sch.size() * sizeof(LoadEntry), m->sch.size(), &ent);
        if (rc) return rc;
    }
    *out = ent;
    return 0;
}

// What wmx_mix_load and wmx_mix_load_minus share on the host: where the call starts (mix_cursor.h) and the
// schedule of its source format; and the cursor the call ends with.
static int load_begin(wmx_mix *m, const char *who, uint32_t srcU8Len, int freq, int channels, int sample, uint32_t &head_off, uint32_t &tk,
                      wmx::SchedCache::Entry **out) {
    wmx::mix_cursor_begin(cursor_state(m), head_off, tk);
    return load_sched(m, who, srcU8Len, freq, channels, sample, out);
}

static void load_end(const wmx_mix *m, uint32_t n_out, uint32_t head_off, uint32_t tk, uint32_t *head, uint32_t *tick) {
    wmx::mix_cursor_end(cursor_state(m), n_out, head_off, tk);
    *head = head_off;
    *tick = tk;
}

// The instantiation of a bridge load kernel for size class cls (bridge_layout.h).  `of` is handed the class's bound PMAX as a
// compile-time constant and names the kernel:
//     auto kernel = kernel_of_class(cls, [](auto pmax) { return load_minus_kernel<decltype(pmax)::value>; });
template <class Of>
static auto kernel_of_class(int cls, Of of) {
    using std::integral_constant;
    return cls == 0 ? of(integral_constant<int, 4>()) : cls == 1 ? of(integral_constant<int, 8>()) : cls == 2 ? of(integral_constant<int, 16>())
                                                                                                           : of(integral_constant<int, 32>());
}

extern "C" {

// ---- src/wmix.h:113-121: pure index arithmetic, identical loops to the reference
uint32_t wmix_len_of_out(uint8_t inChn, uint16_t inFreq, uint32_t inLen, uint8_t outChn, uint16_t outFreq) {
    if (inFreq == outFreq && inChn == outChn) return inLen;
    return wmx::len_walk(inChn, inFreq, outChn, outFreq, inLen, true, false);
}
uint32_t wmix_len_of_in(uint8_t inChn, uint16_t inFreq, uint8_t outChn, uint16_t outFreq, uint32_t outLen) {
    if (inFreq == outFreq && inChn == outChn) return outLen;
    return wmx::len_walk(inChn, inFreq, outChn, outFreq, outLen, false, true);
}

// batched wmix_pcm_zoom: n_streams buffers of the same format and length.  Strides in int16 elements.  out_capacity =
// bytes available per output row: a conversion that needs more fails with WMX_EINVAL (and *out_len = what it needs)
// instead of overrunning the row -- the reference has no such check, its callers size `out` by wmix_len_of_out.
int wmx_pcm_zoom(int inChn, int inFreq, const int16_t *d_in, uint32_t inLen, int outChn, int outFreq, int16_t *d_out, uint32_t out_capacity,
                 long in_stride, long out_stride, int n_streams, uint32_t *out_len, void *stream) {
    using namespace wmx;
    if (!d_in || !d_out || n_streams < 1 || inChn < 1 || outChn < 1 || inFreq < 1 || outFreq < 1) {
        set_error("wmx_pcm_zoom: bad argument");
        return WMX_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    if (inFreq == outFreq && inChn == outChn) {  // memcpy branch, src/wmix.c:154-158
        if (out_len) *out_len = inLen;
        if (inLen > out_capacity) {
            set_error("wmx_pcm_zoom: %u output bytes per row, capacity %u", inLen, out_capacity);
            return WMX_EINVAL;
        }
        if (inLen == 0) return 0;
        if (n_streams == 1)
            WMX_HIP(hipMemcpyAsync(d_out, d_in, inLen, hipMemcpyDeviceToDevice, s));
        else
            WMX_HIP(hipMemcpy2DAsync(d_out, out_stride * 2, d_in, in_stride * 2, inLen, n_streams, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    // the gather list depends on the format only: built and uploaded once per format and thread
    static thread_local std::vector<int32_t> idx;
    static thread_local SchedCache cache;
    const uint64_t k0 = ((uint64_t)inChn << 56) | ((uint64_t)outChn << 48) | ((uint64_t)(uint32_t)inFreq << 24) | (uint32_t)outFreq;
    const uint64_t k1 = ((uint64_t)(uint32_t)current_device() << 32) | inLen;
    SchedCache::Entry *ent = cache.find(k0, k1);
    if (!ent) {
        zoom_schedule((uint8_t)inChn, (uint16_t)inFreq, inLen, (uint8_t)outChn, (uint16_t)outFreq, idx);
        const int rc = cache.add(k0, k1, idx.data(), idx.size() * sizeof(int32_t), idx.size(), &ent);
        if (rc) return rc;
    }
    if (out_len) *out_len = (uint32_t)(ent->n * 2);
    if (ent->n * 2 > out_capacity) {
        set_error("wmx_pcm_zoom: %zu output bytes per row, capacity %u", ent->n * 2, out_capacity);
        return WMX_EINVAL;
    }
    if (ent->n == 0) return 0;
    const unsigned grid = stream_grid(ent->n * (size_t)n_streams, 256);
    hipLaunchKernelGGL(zoom_kernel, dim3(grid), dim3(256), 0, s, d_in, d_out, (const int32_t *)ent->p, (uint32_t)ent->n, in_stride,
                       out_stride, n_streams);
    WMX_LAUNCH_CHECK();
    return cache.used(ent, s);
}

// legacy host form, src/wmix.h:122-127
uint32_t wmix_pcm_zoom(uint8_t inChn, uint16_t inFreq, uint8_t *in, uint32_t inLen, uint8_t outChn, uint16_t outFreq, uint8_t *out) {
    using namespace wmx;
    static thread_local Stage st;  // region 0: in, region 1: out
    if (inLen == 0 || !in || !out || !inFreq || !outFreq || !inChn || !outChn) return 0;
    const uint32_t need = wmix_len_of_out(inChn, inFreq, inLen, outChn, outFreq);  // what the reference's callers size `out` by
    uint32_t n = 0;
    // the calling thread's own non-blocking stream, and only that one is waited for (wmx_internal.h: thread_stream)
    hipStream_t ts = thread_stream();
    if (st.begin((size_t)inLen + need, kMappedMaxBytes, {(size_t)inLen + 16, (size_t)need + 16})) return 0;
    const bool ok = st.put(0, in, inLen, ts) == 0 &&
                    wmx_pcm_zoom(inChn, inFreq, st.dev<const int16_t>(0), inLen, outChn, outFreq, st.dev<int16_t>(1), need + 16, 0, 0, 1, &n, ts) == 0;
    if (ok) st.get(1, out, n);
    return st.finish(ts) == 0 && ok ? n : 0;
}

int wmx_mix_destroy(wmx_mix *m) {
    WMX_ON_DEVICE(m);
    if (!m) return 0;
    if (m->h_rings)
        (void)hipHostFree(m->h_rings);
    else if (m->d_rings)
        (void)hipFree(m->d_rings);
    if (m->d_conf_members) (void)hipFree(m->d_conf_members);
    if (m->d_conf_tab) (void)hipFree(m->d_conf_tab);
    if (m->d_conf_lead) (void)hipFree(m->d_conf_lead);
    m->talkers.destroy();
    m->cursors.destroy();
    if (m->d_prompt_idx) (void)hipFree(m->d_prompt_idx);
    if (m->d_leg_span) (void)hipFree(m->d_leg_span);
    if (m->d_prompt) (void)hipFree(m->d_prompt);
    delete m;
    return 0;
}

// n_groups rings of 1 s each in the ring format (the reference's compile-time WMIX_CHN / WMIX_FREQ)
int wmx_mix_create(wmx_mix **out, int n_groups, int ring_chn, int ring_freq) {
    using namespace wmx;
    if (!out) return WMX_EINVAL;
    *out = nullptr;
    if (n_groups < 1 || (ring_chn != 1 && ring_chn != 2) || ring_freq < 1000 || ring_freq > 96000) {
        set_error("wmx_mix_create: unsupported n_groups=%d chn=%d freq=%d", n_groups, ring_chn, ring_freq);
        return WMX_EINVAL;
    }
    wmx_mix *m = new wmx_mix();
    if ((m->device = wmx::current_device()) < 0) {
        delete m;
        return WMX_ENODEV;
    }
    m->n_groups = n_groups;
    m->cursors = LegState("hipMemset(leg cursors)", "mixer", n_groups, kLegCursorColumns);
    m->talkers = LegState("hipMemset(speakers)", "mixer", n_groups, kLegTalkerColumns);
    m->chn = ring_chn;
    m->freq = ring_freq;
    m->ring_bytes = (uint32_t)(ring_chn * 2) * (uint32_t)ring_freq;  // WMIX_BUFF_SIZE, src/wmixConf.h:124
    m->head_off = 0;
    m->tick = 0;
    m->reduce_mode = 1;
    m->play_correct = (uint32_t)(ring_chn * ring_freq * 16 / 8 / 5);  // PLAT_PLAY_CORRECT, platform/alsa/plat.h:54
    m->d_rings = nullptr;
    hipError_t e = hipMalloc(&m->d_rings, (size_t)m->ring_bytes * n_groups);
    if (e == hipSuccess) e = hipMemset(m->d_rings, 0, (size_t)m->ring_bytes * n_groups);
    if (e != hipSuccess) {
        const int rc = hip_fail(e, "hipMalloc/hipMemset(rings)", __FILE__, __LINE__);
        wmx_mix_destroy(m);
        return rc;
    }
    *out = m;
    return 0;
}

int wmx_mix_set(wmx_mix *m, uint32_t head_off, uint32_t tick, int reduce_mode) {
    WMX_ON_DEVICE(m);
    if (!m || head_off >= m->ring_bytes || reduce_mode < 1 || reduce_mode > 255) return WMX_EINVAL;
    m->head_off = head_off;
    m->tick = tick;
    m->reduce_mode = (uint8_t)reduce_mode;
    return 0;
}

// VIEW_PLAY_CORRECT (src/wmixPlat.h:20, src/wmix.c:1668-1669): how far in front of the play head a source without a cursor of its
// own starts.  A compile-time constant of the reference's platform directory: 200 ms of ring in platform/alsa (the default of
// wmx_mix_create), 0 in platform/hi3516 and platform/t31 (plat.h:16).
int wmx_mix_set_play_correct(wmx_mix *m, uint32_t bytes) {
    if (!m || bytes >= m->ring_bytes || bytes % (uint32_t)(m->chn * 2)) {
        wmx::set_error("wmx_mix_set_play_correct: %u bytes is not a whole frame inside the ring", bytes);
        return WMX_EINVAL;
    }
    m->play_correct = bytes;
    return 0;
}

int wmx_mix_ring_bytes(const wmx_mix *m) { return m ? (int)m->ring_bytes : WMX_EINVAL; }

// wmix_load_data for every group: n_src sources per group (source s of group g at d_src + g*group_stride +
// s*source_stride, int16 elements), all in the same format, all starting from the cursor (*head, *tick) like
// N task threads that begin together (head == UINT32_MAX is the reference's NULL head); they are added in
// index order.  On return *head / *tick hold the cursor every one of those sources ends with.
// NOTE: like the reference (src/wmix.c:1857,1914) the up-sampling fill reads one source frame past
// srcU8Len; the caller's buffers must make that frame readable.
int wmx_mix_load(wmx_mix *m, const int16_t *d_src, uint32_t srcU8Len, int freq, int channels, int sample, int n_src, long group_stride,
                 long source_stride, int reduce, uint32_t *head, uint32_t *tick, void *stream) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    if (!m || !head || !tick || n_src < 1) {
        set_error("wmx_mix_load: bad argument");
        return WMX_EINVAL;
    }
    if (!d_src || srcU8Len < 1) return 0;  // reference returns the head unchanged (src/wmix.c:1663-1664)
    uint32_t head_off = *head, tk = *tick;
    SchedCache::Entry *ent = nullptr;
    const int rcb = load_begin(m, "wmx_mix_load", srcU8Len, freq, channels, sample, head_off, tk, &ent);
    if (rcb) return rcb;
    const uint32_t n_out = (uint32_t)ent->n;
    const int rdce = (reduce == m->reduce_mode) ? 1 : m->reduce_mode;  // src/wmix.c:1675-1676
    hipStream_t s = as_stream(stream);
    if (n_out) {
        const unsigned grid = stream_grid((size_t)n_out * m->n_groups, 256);
        hipLaunchKernelGGL(load_kernel, dim3(grid), dim3(256), 0, s, m->d_rings, m->ring_bytes / 2, d_src, (const LoadEntry *)ent->p,
                           n_out, head_off / 2, n_src, group_stride, source_stride, rdce, m->n_groups);
        WMX_LAUNCH_CHECK();
        const int rcu = m->sched.used(ent, s);
        if (rcu) return rcu;
    }
    load_end(m, n_out, head_off, tk, head, tick);
    return 0;
}

// The bridge load (include/wmix_amd.h): the mixer's rings read as n_groups / parties conferences of `parties` consecutive rings.
// One launch; every source is read once (load_minus_kernel, mix_minus.h).
int wmx_mix_load_minus(wmx_mix *m, int parties, const int16_t *d_src, uint32_t srcU8Len, int freq, int channels, int sample, long conf_stride,
                       long source_stride, const uint8_t *d_mute, int reduce, uint32_t *head, uint32_t *tick, void *stream) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    if (!m || !head || !tick) {
        set_error("wmx_mix_load_minus: bad argument");
        return WMX_EINVAL;
    }
    if (parties < 2 || parties > WMX_MIX_MAX_PARTIES || m->n_groups % parties != 0) {
        set_error("wmx_mix_load_minus: parties=%d must be 2 .. %d and divide the mixer's %d rings", parties, WMX_MIX_MAX_PARTIES, m->n_groups);
        return WMX_EINVAL;
    }
    if (!d_src || srcU8Len < 1) return 0;  // like wmx_mix_load
    uint32_t head_off = *head, tk = *tick;
    SchedCache::Entry *ent = nullptr;
    const int rcb = load_begin(m, "wmx_mix_load_minus", srcU8Len, freq, channels, sample, head_off, tk, &ent);
    if (rcb) return rcb;
    const uint32_t n_out = (uint32_t)ent->n;
    const int rdce = (reduce == m->reduce_mode) ? 1 : m->reduce_mode;  // src/wmix.c:1675-1676
    hipStream_t s = as_stream(stream);
    if (n_out) {
        const int n_conf = m->n_groups / parties;
        const unsigned grid = stream_grid((size_t)n_out * n_conf, 256);
        auto kernel = kernel_of_class(bridge_size_class(parties), [](auto pmax) { return load_minus_kernel<decltype(pmax)::value>; });
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, m->d_rings, m->ring_bytes / 2, d_src, (const LoadEntry *)ent->p, n_out,
                           head_off / 2, parties, conf_stride, source_stride, d_mute, rdce, n_conf);
        WMX_LAUNCH_CHECK();
        const int rcu = m->sched.used(ent, s);
        if (rcu) return rcu;
    }
    load_end(m, n_out, head_off, tk, head, tick);
    return 0;
}

// The layout of the bridge load below (include/wmix_amd.h, bridge_layout.h).  Validated and sorted into the size classes on the host;
// the member list and the {offset, size} table go to buffers the handle owns.  A refusal leaves the layout in force as it is.
int wmx_mix_set_conferences(wmx_mix *m, int n_conf, const int32_t *host_off, const int32_t *host_members, void *stream) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    if (!m) return WMX_EINVAL;
    BridgeLayout l;
    if (const char *why = bridge_layout_build(l, m->n_groups, n_conf, host_off, host_members)) {
        set_error("wmx_mix_set_conferences: %s (n_conf=%d, %d rings, at most %d members each)", why, n_conf, m->n_groups, WMX_MIX_MAX_PARTIES);
        return WMX_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    // the uploads' sources are pageable memory of the handle, and a launch in flight may still read the buffers that grow here
    WMX_HIP(hipStreamSynchronize(s));
    if (l.members.size() > m->conf_cap_members) {
        if (m->d_conf_members) (void)hipFree(m->d_conf_members);
        m->d_conf_members = nullptr, m->conf_cap_members = 0;
        WMX_HIP(hipMalloc(&m->d_conf_members, l.members.size() * sizeof(int32_t)));
        m->conf_cap_members = l.members.size();
    }
    if ((size_t)l.slots() > m->conf_cap_slots) {
        if (m->d_conf_tab) (void)hipFree(m->d_conf_tab);
        if (m->d_conf_lead) (void)hipFree(m->d_conf_lead);
        m->d_conf_tab = nullptr, m->d_conf_lead = nullptr, m->conf_cap_slots = 0;
        WMX_HIP(hipMalloc(&m->d_conf_tab, (size_t)l.slots() * 2 * sizeof(int32_t)));
        WMX_HIP(hipMalloc(&m->d_conf_lead, (size_t)l.slots() * sizeof(uint32_t)));
        m->conf_cap_slots = (size_t)l.slots();
    }
    m->conf = std::move(l);
    m->conf_leads.valid = false;  // the slots are other conferences now
    if (!m->conf.members.empty())
        WMX_HIP(hipMemcpyAsync(m->d_conf_members, m->conf.members.data(), m->conf.members.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (!m->conf.tab.empty())
        WMX_HIP(hipMemcpyAsync(m->d_conf_tab, m->conf.tab.data(), m->conf.tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    return 0;
}

int wmx_mix_conferences(const wmx_mix *m) { return m ? m->conf.n_conf : WMX_EINVAL; }

// The bridge load over the layout: at most one launch per non-empty size class.  The cursor rule runs on the host once per distinct
// start value (bridge_plan_load); a call after which every lead is what the device already holds uploads nothing.
int wmx_mix_load_minus_conf(wmx_mix *m, const int16_t *d_src, uint32_t srcU8Len, int freq, int channels, int sample, long source_stride,
                            const uint8_t *d_mute, int reduce, uint32_t *head, uint32_t *tick, void *stream) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    if (!m || !head || !tick) {
        set_error("wmx_mix_load_minus_conf: bad argument");
        return WMX_EINVAL;
    }
    if (m->conf.n_conf < 1) {
        set_error("wmx_mix_load_minus_conf: no layout (wmx_mix_set_conferences)");
        return WMX_EINVAL;
    }
    if (!d_src || srcU8Len < 1) return 0;  // like wmx_mix_load
    SchedCache::Entry *ent = nullptr;
    const int rcb = load_sched(m, "wmx_mix_load_minus_conf", srcU8Len, freq, channels, sample, &ent);
    if (rcb) return rcb;
    const uint32_t n_out = (uint32_t)ent->n;
    const int rdce = (reduce == m->reduce_mode) ? 1 : m->reduce_mode;  // src/wmix.c:1675-1676
    hipStream_t s = as_stream(stream);
    const BridgePlan plan = bridge_plan_load(m->conf, cursor_state(m), n_out, head, tick, m->conf_leads, m->conf_next);
    if (plan.upload) {
        WMX_HIP(hipStreamSynchronize(s));  // the previous upload must have left h_conf_lead before it is rewritten
        m->h_conf_lead = m->conf_leads.lead;
        WMX_HIP(hipMemcpyAsync(m->d_conf_lead, m->h_conf_lead.data(), m->h_conf_lead.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    }
    for (int k = 0; k < kBridgeClasses && n_out; k++) {
        const int first = m->conf.class_begin[k], n_slots = m->conf.class_begin[k + 1] - first;
        if (!n_slots) continue;
        const uint32_t n_pad = (n_out + 63) / 64 * 64;  // whole waves per conference: the slot is wave-uniform
        const unsigned grid = stream_grid((size_t)n_pad * n_slots, 256);
        auto kernel = kernel_of_class(k, [](auto pmax) { return load_minus_conf_kernel<decltype(pmax)::value>; });
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, m->d_rings, m->ring_bytes / 2, d_src, (const LoadEntry *)ent->p, n_out,
                           n_pad, plan.base_sample, (const int32_t *)m->d_conf_tab + 2 * (size_t)first, (const uint32_t *)m->d_conf_lead + first,
                           (const int32_t *)m->d_conf_members, source_stride, d_mute, rdce, n_slots);
        WMX_LAUNCH_CHECK();
    }
    return n_out && m->conf.slots() ? m->sched.used(ent, s) : 0;
}

// ---- a cursor per leg (include/wmix_amd.h, leg_cursor.h)
// the cursors (fresh) and the drop counts (zero), and the scratch of the span table and the windows (the 16-byte span entries in
// front), from the first call that needs them on.  A layout has at most n_groups / 2 conferences that load.
static int legs_state(wmx_mix *m) {
    using namespace wmx;
    const int rc = m->cursors.make();
    if (rc || m->d_leg_span) return rc;
    const size_t n = (size_t)m->n_groups;
    void *p = nullptr;
    const int rcb = zeroed_block(&p, n * sizeof(LegSpanEntry) + (n / 2 + 1) * sizeof(uint2), "hipMemset(leg spans)");
    if (rcb) return rcb;
    m->d_leg_span = static_cast<LegSpanEntry *>(p);
    m->d_leg_win = reinterpret_cast<uint2 *>(m->d_leg_span + n);
    return 0;
}

// The bridge load with a cursor per leg: the cursor kernel (one wave per conference), then at most one load launch per non-empty size
// class.  Which slots are calls is known on the device only, so nothing of the cursors passes through the host.  d_calls: NULL for
// wmx_mix_load_minus_legs (the valid slots in slot order), the call lists for wmx_mix_load_minus_legs_calls.
static int load_minus_legs_any(const char *who, wmx_mix *m, const int16_t *d_src, uint32_t srcU8Len, int freq, int channels, int sample,
                               long source_stride, long packet_stride, int max_packets, const uint32_t *d_len, const uint32_t *d_calls,
                               bool with_calls, const uint8_t *d_mute, int reduce, void *stream) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    if (!m || !d_src || !d_len || (with_calls && !d_calls)) {
        set_error("%s: bad argument", who);
        return WMX_EINVAL;
    }
    if (m->conf.n_conf < 1) {
        set_error("%s: no layout (wmx_mix_set_conferences)", who);
        return WMX_EINVAL;
    }
    if (max_packets < 1 || max_packets > WMX_MIX_MAX_LEG_PACKETS) {
        set_error("%s: max_packets=%d must be 1 .. %d", who, max_packets, WMX_MIX_MAX_LEG_PACKETS);
        return WMX_EINVAL;
    }
    if (srcU8Len < 1) return 0;  // like wmx_mix_load
    SchedCache::Entry *ent = nullptr;
    const int rcb = load_sched(m, who, srcU8Len, freq, channels, sample, &ent);
    if (rcb) return rcb;
    const uint32_t n_out = (uint32_t)ent->n;
    // a call list holds up to WMX_MIX_MAX_LEG_PACKETS calls whatever max_packets is: silence calls need no slot
    const int span_calls = with_calls ? WMX_MIX_MAX_LEG_PACKETS : max_packets;
    if ((uint64_t)n_out * (uint32_t)span_calls > m->ring_bytes / 2) {
        set_error("%s: %d packets of %u output samples do not fit the %u-sample ring in one call", who, span_calls, n_out, m->ring_bytes / 2);
        return WMX_EINVAL;
    }
    const int rcs = legs_state(m);
    if (rcs) return rcs;
    const int n_slots = m->conf.slots();
    if (!n_out || !n_slots) return 0;
    const int rdce = (reduce == m->reduce_mode) ? 1 : m->reduce_mode;  // src/wmix.c:1675-1676
    // The duck (leg_prompt.h, REDUCE): only while a play with reduce > 0 can still be making calls, and only on a mixer whose own
    // reduce_mode is 1, the mode the play task takes.  Every other tick launches what it launched before there were prompts.
    const bool duck = m->d_prompt && m->reduce_mode == 1 && m->duck_last > m->prompt_now;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(with_calls ? leg_cursor_kernel<true> : leg_cursor_kernel<false>, dim3(stream_grid((size_t)n_slots * 64, 256)), dim3(256), 0,
                       s, (const int32_t *)m->d_conf_tab, (const int32_t *)m->d_conf_members, d_len, srcU8Len, max_packets, d_mute, cursor_state(m), n_out,
                       m->cursors.at<uint32_t>(kCursorHead), m->cursors.at<uint32_t>(kCursorTick), m->cursors.at<uint32_t>(kCursorDropped), m->d_leg_span,
                       m->d_leg_win, m->n_groups, n_slots, d_calls);
    WMX_LAUNCH_CHECK();
    // whole waves per conference, enough for the longest window of legs that write side by side; a longer one is walked in strides
    const uint32_t n_pad = (n_out * (uint32_t)span_calls + 63) / 64 * 64;
    if (duck) {  // one block per conference: the ducked members' rings, and the slot's mask for the sweeps
        hipLaunchKernelGGL(duck_fold_kernel, dim3((unsigned)n_slots), dim3(256), 0, s, m->d_rings, m->ring_bytes / 2, d_src, (const LoadEntry *)ent->p,
                           n_out, (const int32_t *)m->d_conf_tab, (const uint2 *)m->d_leg_win, (const LegSpanEntry *)m->d_leg_span,
                           (const int32_t *)m->d_conf_members, source_stride, packet_stride, reduce, (const LegPrompt *)m->d_prompt,
                           (const PromptClip *)m->d_clip_tab, (uint32_t)m->clips.size(), (uint32_t)m->arena_cap, m->d_duck, m->n_groups, n_slots);
        WMX_LAUNCH_CHECK();
    }
    for (int k = 0; k < kBridgeClasses; k++) {
        const int first = m->conf.class_begin[k], n_class = m->conf.class_begin[k + 1] - first;
        if (!n_class) continue;
        const unsigned grid = stream_grid((size_t)n_pad * n_class, 256);
        auto plain = with_calls ? kernel_of_class(k, [](auto pmax) { return load_minus_legs_kernel<decltype(pmax)::value, true, false>; })
                                : kernel_of_class(k, [](auto pmax) { return load_minus_legs_kernel<decltype(pmax)::value, false, false>; });
        auto ducking = with_calls ? kernel_of_class(k, [](auto pmax) { return load_minus_legs_kernel<decltype(pmax)::value, true, true>; })
                                  : kernel_of_class(k, [](auto pmax) { return load_minus_legs_kernel<decltype(pmax)::value, false, true>; });
        hipLaunchKernelGGL(duck ? ducking : plain, dim3(grid), dim3(256), 0, s, m->d_rings, m->ring_bytes / 2, d_src, (const LoadEntry *)ent->p,
                           n_out, n_pad, (const int32_t *)m->d_conf_tab + 2 * (size_t)first, (const uint2 *)m->d_leg_win + first,
                           (const LegSpanEntry *)m->d_leg_span, (const int32_t *)m->d_conf_members, source_stride, packet_stride, rdce,
                           m->n_groups, n_class, duck ? (const uint32_t *)m->d_duck + first : (const uint32_t *)nullptr);
        WMX_LAUNCH_CHECK();
    }
    return m->sched.used(ent, s);
}

int wmx_mix_load_minus_legs(wmx_mix *m, const int16_t *d_src, uint32_t srcU8Len, int freq, int channels, int sample, long source_stride,
                            long packet_stride, int max_packets, const uint32_t *d_len, const uint8_t *d_mute, int reduce, void *stream) {
    return load_minus_legs_any("wmx_mix_load_minus_legs", m, d_src, srcU8Len, freq, channels, sample, source_stride, packet_stride, max_packets,
                               d_len, nullptr, false, d_mute, reduce, stream);
}

// The same with a call list per leg (wmx_rtp_sequence_legs): calls in list order, a silence call moves the cursor and adds nothing.
int wmx_mix_load_minus_legs_calls(wmx_mix *m, const int16_t *d_src, uint32_t srcU8Len, int freq, int channels, int sample, long source_stride,
                                  long packet_stride, int max_packets, const uint32_t *d_len, const uint32_t *d_calls, const uint8_t *d_mute,
                                  int reduce, void *stream) {
    return load_minus_legs_any("wmx_mix_load_minus_legs_calls", m, d_src, srcU8Len, freq, channels, sample, source_stride, packet_stride,
                               max_packets, d_len, d_calls, true, d_mute, reduce, stream);
}

int wmx_mix_reset_leg_cursors(wmx_mix *m, const int32_t *host_idx, int n, void *stream) {
    WMX_ON_DEVICE(m);
    if (!m) return WMX_EINVAL;
    const int rc = m->cursors.reset("wmx_mix_reset_leg_cursors: ring", host_idx, n, wmx::as_stream(stream));
    return rc ? rc : legs_state(m);  // the first call makes the scratch too: no load allocates behind it
}

int wmx_mix_export_leg_cursors(const wmx_mix *m, uint32_t *host_head, uint32_t *host_tick, uint32_t *host_dropped, void *stream) {
    WMX_ON_DEVICE(m);
    if (!m) return WMX_EINVAL;
    return m->cursors.export_to({host_head, host_tick, host_dropped}, wmx::as_stream(stream));
}

// ---- a prompt per leg (include/wmix_amd.h, leg_prompt.h)
// The store: made once, blocking.  Clips are in the ring's own format, so only a mixer of 1 x 8000 rings has one.
int wmx_mix_prompts(wmx_mix *m, int max_clips, long max_samples) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    if (!m) return WMX_EINVAL;
    if (m->d_prompt) {
        set_error("wmx_mix_prompts: the mixer has its store already (%zu clips, %zu samples)", m->clip_cap, m->arena_cap);
        return WMX_ESTATE;
    }
    if (m->chn != 1 || m->freq != 8000 || max_clips < 1 || max_clips > (1 << 20) || max_samples < 1 || max_samples > (1L << 30)) {
        set_error("wmx_mix_prompts: max_clips=%d (1 .. 2^20) max_samples=%ld (1 .. 2^30), and rings of 1 x 8000 (these: %d x %d)", max_clips,
                  max_samples, m->chn, m->freq);
        return WMX_EINVAL;
    }
    const size_t n = (size_t)m->n_groups, state_bytes = n * sizeof(LegPrompt), tab_bytes = (size_t)max_clips * sizeof(PromptClip);
    const size_t duck_bytes = (n / 2 + 1) * sizeof(uint32_t);  // a layout has at most n_groups / 2 conferences that load
    void *p = nullptr;
    const int rc = zeroed_block(&p, state_bytes + tab_bytes + duck_bytes + (size_t)max_samples * sizeof(int16_t), "hipMemset(prompts)");
    if (rc) return rc;
    const std::vector<LegPrompt> idle(n, leg_prompt_idle(0u));
    const hipError_t e = hipMemcpy(p, idle.data(), state_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return hip_fail(e, "hipMemcpy(prompt states)", __FILE__, __LINE__);
    }
    m->d_prompt = static_cast<LegPrompt *>(p);
    m->d_clip_tab = reinterpret_cast<PromptClip *>(m->d_prompt + n);
    m->d_duck = reinterpret_cast<uint32_t *>(m->d_clip_tab + max_clips);
    m->d_clip_arena = reinterpret_cast<int16_t *>(m->d_duck + (n / 2 + 1));
    m->clip_cap = (size_t)max_clips;
    m->arena_cap = (size_t)max_samples;
    m->arena_used = 0;
    m->clips.clear();
    m->clips.reserve(m->clip_cap);
    m->prompt_end.assign(n, 0);
    m->prompt_now = m->prompt_last = 0;
    m->prompt_ducks.assign(n, 0);
    m->duck_last = 0;
    return 0;
}

// One more clip behind the last: a blocking copy into arena and table entries that no leg refers to yet, so nothing in flight reads them.
int wmx_mix_add_clip(wmx_mix *m, const int16_t *host_pcm, long samples, int *clip) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    if (!m) return WMX_EINVAL;
    if (!m->d_prompt) {
        set_error("wmx_mix_add_clip: no store (wmx_mix_prompts)");
        return WMX_ESTATE;
    }
    if (!host_pcm || samples < 1 || m->clips.size() >= m->clip_cap || (size_t)samples > m->arena_cap - m->arena_used) {
        set_error("wmx_mix_add_clip: %ld samples (at least 1) into a store with %zu of %zu clips and %zu of %zu samples used", samples,
                  m->clips.size(), m->clip_cap, m->arena_used, m->arena_cap);
        return WMX_EINVAL;
    }
    const PromptClip c{(uint32_t)m->arena_used, (uint32_t)samples};
    WMX_HIP(hipMemcpy(m->d_clip_arena + m->arena_used, host_pcm, (size_t)samples * sizeof(int16_t), hipMemcpyHostToDevice));
    WMX_HIP(hipMemcpy(m->d_clip_tab + m->clips.size(), &c, sizeof(c), hipMemcpyHostToDevice));
    if (clip) *clip = (int)m->clips.size();
    m->clips.push_back(c);
    m->arena_used += (size_t)samples;
    return 0;
}

// `value` into the listed legs' state entries (NULL = every leg), ordered on `stream`; ticks: the launches of wmx_mix_load_prompts
// after which such a leg is idle again for certain (0: it is idle now; UINT64_MAX: an endless play); ducks: a play with reduce > 0
static int prompt_set(wmx_mix *m, const char *who, const int32_t *host_idx, int n, const wmx::LegPrompt &value, bool keep_done, uint64_t ticks,
                      bool ducks, void *stream) {
    using namespace wmx;
    if (host_idx && n < 0) return WMX_EINVAL;
    if (idx_check(host_idx, n, m->n_groups, who, "mixer")) return WMX_EINVAL;
    if (host_idx && n == 0) return 0;
    hipStream_t s = as_stream(stream);
    const int count = host_idx ? n : m->n_groups;
    if (host_idx) {
        const int rcu = upload_idx(m->d_prompt_idx, m->prompt_idx_cap, host_idx, n, s);
        if (rcu) return rcu;
    }
    hipLaunchKernelGGL(prompt_set_kernel, dim3(stream_grid((size_t)count, 256)), dim3(256), 0, s, m->d_prompt,
                       host_idx ? (const int32_t *)m->d_prompt_idx : (const int32_t *)nullptr, count, m->n_groups, value, keep_done ? 1 : 0);
    WMX_LAUNCH_CHECK();
    const uint64_t end = ticks == UINT64_MAX ? UINT64_MAX : m->prompt_now + ticks;
    for (int i = 0; i < count; i++) {
        const size_t r = (size_t)(host_idx ? host_idx[i] : i);
        m->prompt_end[r] = end;
        m->prompt_ducks[r] = ducks ? 1 : 0;
    }
    m->prompt_last = m->duck_last = 0;
    for (size_t r = 0; r < m->prompt_end.size(); r++) {
        const uint64_t e = m->prompt_end[r];
        m->prompt_last = e > m->prompt_last ? e : m->prompt_last;
        if (m->prompt_ducks[r]) m->duck_last = e > m->duck_last ? e : m->duck_last;
    }
    return 0;
}

// reduce: the reference's argument of every play call, 0 .. 15 -- while the prompt makes calls the others are loaded into the ring
// divided by reduce + 1 (leg_prompt.h, REDUCE)
static int play_any(const char *who, wmx_mix *m, const int32_t *host_idx, int n, int clip, int repeat, int gap_ticks, int reduce, void *stream) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    if (!m) return WMX_EINVAL;
    if (!m->d_prompt) {
        set_error("%s: no store (wmx_mix_prompts)", who);
        return WMX_ESTATE;
    }
    if (clip < 0 || (size_t)clip >= m->clips.size() || repeat < 0 || gap_ticks < 0 || (uint32_t)gap_ticks > kPromptMaxGap || reduce < 0 ||
        (uint32_t)reduce > kPromptMaxReduce) {
        set_error("%s: clip=%d (the store holds %zu) repeat=%d (0 = until stopped) gap_ticks=%d (0 .. %u) reduce=%d (0 .. %u)", who, clip,
                  m->clips.size(), repeat, gap_ticks, kPromptMaxGap, reduce, kPromptMaxReduce);
        return WMX_EINVAL;
    }
    // a pass is one call per started 160 samples; between two passes lie gap_ticks ticks without one (leg_prompt.h)
    const uint64_t per_pass = ((uint64_t)m->clips[(size_t)clip].samples + kLegRow - 1) / kLegRow;
    const uint64_t ticks = repeat == 0 ? UINT64_MAX : (uint64_t)repeat * per_pass + (uint64_t)(repeat - 1) * (uint64_t)gap_ticks;
    return prompt_set(m, who, host_idx, n, leg_prompt_play(clip, (uint32_t)repeat, (uint32_t)gap_ticks, 0u, (uint32_t)reduce), true, ticks,
                      reduce > 0, stream);
}

int wmx_mix_play(wmx_mix *m, const int32_t *host_idx, int n, int clip, int repeat, int gap_ticks, void *stream) {
    return play_any("wmx_mix_play: ring", m, host_idx, n, clip, repeat, gap_ticks, 0, stream);
}

int wmx_mix_play_duck(wmx_mix *m, const int32_t *host_idx, int n, int clip, int repeat, int gap_ticks, int reduce, void *stream) {
    return play_any("wmx_mix_play_duck: ring", m, host_idx, n, clip, repeat, gap_ticks, reduce, stream);
}

int wmx_mix_stop(wmx_mix *m, const int32_t *host_idx, int n, void *stream) {
    WMX_ON_DEVICE(m);
    if (!m) return WMX_EINVAL;
    if (!m->d_prompt) {
        wmx::set_error("wmx_mix_stop: no store (wmx_mix_prompts)");
        return WMX_ESTATE;
    }
    return prompt_set(m, "wmx_mix_stop: ring", host_idx, n, wmx::leg_prompt_idle(0u), true, 0, false, stream);
}

// a new call in a reused slot: idle, done = 0; a mixer without a store has nothing to reset
int wmx_mix_reset_prompts(wmx_mix *m, const int32_t *host_idx, int n, void *stream) {
    WMX_ON_DEVICE(m);
    if (!m || (host_idx && n < 0)) return WMX_EINVAL;
    if (wmx::idx_check(host_idx, n, m->n_groups, "wmx_mix_reset_prompts: ring", "mixer")) return WMX_EINVAL;
    if (!m->d_prompt) return 0;
    return prompt_set(m, "wmx_mix_reset_prompts: ring", host_idx, n, wmx::leg_prompt_idle(0u), false, 0, false, stream);
}

int wmx_mix_export_prompts(const wmx_mix *m, int32_t *host_clip, uint32_t *host_pos, uint32_t *host_left, uint32_t *host_done, void *stream) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    if (!m) return WMX_EINVAL;
    const size_t n = (size_t)m->n_groups;
    std::vector<LegPrompt> st(n, leg_prompt_idle(0u));  // no store: every leg idle
    if (m->d_prompt) {
        WMX_HIP(hipStreamSynchronize(as_stream(stream)));
        WMX_HIP(hipMemcpy(st.data(), m->d_prompt, n * sizeof(LegPrompt), hipMemcpyDeviceToHost));
    }
    for (size_t r = 0; r < n; r++) {
        if (host_clip) host_clip[r] = st[r].clip < 0 ? -1 : st[r].clip;
        if (host_pos) host_pos[r] = st[r].pos;
        if (host_left) host_left[r] = st[r].left;
        if (host_done) host_done[r] = st[r].done;
    }
    return 0;
}

// Per ring the divisor the next load of the legs applies to what the others add there (1: none): leg_prompt_ducks on the states as the
// work queued on `stream` leaves them.  Without a store, and on a mixer whose reduce_mode is not 1, nothing ducks.
int wmx_mix_export_duck(const wmx_mix *m, uint8_t *host_divisor, void *stream) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    if (!m || !host_divisor) return WMX_EINVAL;
    const size_t n = (size_t)m->n_groups;
    memset(host_divisor, 1, n);
    if (!m->d_prompt || m->reduce_mode != 1) return 0;
    std::vector<LegPrompt> st(n);
    WMX_HIP(hipStreamSynchronize(as_stream(stream)));
    WMX_HIP(hipMemcpy(st.data(), m->d_prompt, n * sizeof(LegPrompt), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < n; r++) {
        const int32_t c = st[r].clip;
        const uint32_t samples = c >= 0 && (size_t)c < m->clips.size() ? m->clips[(size_t)c].samples : 0u;
        host_divisor[r] = (uint8_t)leg_prompt_ducks(st[r], samples);
    }
    return 0;
}

// One tick of every leg's prompt: one launch, one wave per ring, behind the tick's load and in front of its drain.  No store, or no
// ring that can still be playing (prompt_end): no launch.
int wmx_mix_load_prompts(wmx_mix *m, void *stream) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    if (!m) return WMX_EINVAL;
    if (!m->d_prompt || m->prompt_last <= m->prompt_now) return 0;
    const unsigned waves = 4, grid = ((unsigned)m->n_groups + waves - 1) / waves;
    hipLaunchKernelGGL(prompt_kernel, dim3(grid), dim3(64 * waves), 0, as_stream(stream), m->d_rings, m->ring_bytes / 2, m->d_prompt,
                       (const PromptClip *)m->d_clip_tab, (uint32_t)m->clips.size(), (const int16_t *)m->d_clip_arena, (uint32_t)m->arena_cap,
                       cursor_state(m), m->n_groups);
    WMX_LAUNCH_CHECK();
    m->prompt_now++;  // behind the check: a launch that failed has moved no leg
    return 0;
}

// ---- talker selection (include/wmix_amd.h, speakers.h)
static int speakers_check(const char *who, const void *m, const void *d_src, uint32_t srcU8Len, int max_speakers, int decay_shift,
                          const void *d_mute_out) {
    using namespace wmx;
    if (!m || !d_src || !d_mute_out) {
        set_error("%s: bad argument", who);
        return WMX_EINVAL;
    }
    if (!speakers_params_ok(max_speakers, decay_shift)) {
        set_error("%s: max_speakers=%d must be 1 .. %d and decay_shift=%d 0 .. 31", who, max_speakers, WMX_MIX_MAX_PARTIES, decay_shift);
        return WMX_EINVAL;
    }
    if (!speakers_len_ok(srcU8Len)) {
        set_error("%s: the level of a row of %u elements can overflow 32 bits (at most %u)", who, srcU8Len / 2, kSpeakersMaxElements);
        return WMX_EINVAL;
    }
    return 0;
}

// one wave per conference, four to a workgroup
static int speakers_launch(wmx_mix *m, int n_slots, int parties, const int16_t *d_src, uint32_t srcU8Len, long conf_stride, long source_stride,
                           const int32_t *tab, const int32_t *members, const uint8_t *d_mute, int max_speakers, uint32_t floor,
                           int decay_shift, uint8_t *d_mute_out, hipStream_t s) {
    using namespace wmx;
    if (n_slots < 1) return 0;
    const unsigned grid = stream_grid((size_t)n_slots * 64, 256);
    hipLaunchKernelGGL(select_speakers_kernel, dim3(grid), dim3(256), 0, s, d_src, srcU8Len / 2, parties, conf_stride, source_stride, tab, members,
                       d_mute, max_speakers, floor, decay_shift, m->talkers.at<uint32_t>(kTalkerEnv), m->talkers.at<uint8_t>(kTalkerSpeaking), d_mute_out, n_slots);
    WMX_LAUNCH_CHECK();
    return 0;
}

int wmx_mix_select_speakers(wmx_mix *m, int parties, const int16_t *d_src, uint32_t srcU8Len, long conf_stride, long source_stride,
                            const uint8_t *d_mute, int max_speakers, uint32_t floor, int decay_shift, uint8_t *d_mute_out, void *stream) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    const int rcc = speakers_check("wmx_mix_select_speakers", m, d_src, srcU8Len, max_speakers, decay_shift, d_mute_out);
    if (rcc) return rcc;
    if (parties < 2 || parties > WMX_MIX_MAX_PARTIES || m->n_groups % parties != 0) {  // wmx_mix_load_minus
        set_error("wmx_mix_select_speakers: parties=%d must be 2 .. %d and divide the mixer's %d rings", parties, WMX_MIX_MAX_PARTIES, m->n_groups);
        return WMX_EINVAL;
    }
    const int rcs = m->talkers.make();
    if (rcs) return rcs;
    // every ring is a member of a conference: nothing to clear
    return speakers_launch(m, m->n_groups / parties, parties, d_src, srcU8Len, conf_stride, source_stride, nullptr, nullptr, d_mute, max_speakers,
                           floor, decay_shift, d_mute_out, as_stream(stream));
}

// Over the layout: the table and the member list are what wmx_mix_set_conferences left on the device, and one launch visits the slots
// of every size class (the kernel has no compile-time bound on the size).  The clear in front of it covers the idle rings and the
// members of placeholders.
int wmx_mix_select_speakers_conf(wmx_mix *m, const int16_t *d_src, uint32_t srcU8Len, long source_stride, const uint8_t *d_mute,
                                 int max_speakers, uint32_t floor, int decay_shift, uint8_t *d_mute_out, void *stream) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    const int rcc = speakers_check("wmx_mix_select_speakers_conf", m, d_src, srcU8Len, max_speakers, decay_shift, d_mute_out);
    if (rcc) return rcc;
    if (m->conf.n_conf < 1) {
        set_error("wmx_mix_select_speakers_conf: no layout (wmx_mix_set_conferences)");
        return WMX_EINVAL;
    }
    const int rcs = m->talkers.make();
    if (rcs) return rcs;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(speakers_clear_kernel, dim3(stream_grid((size_t)m->n_groups, 256)), dim3(256), 0, s, m->talkers.at<uint8_t>(kTalkerSpeaking), d_mute_out,
                       m->n_groups);
    WMX_LAUNCH_CHECK();
    return speakers_launch(m, m->conf.slots(), 0, d_src, srcU8Len, 0, source_stride, m->d_conf_tab, m->d_conf_members, d_mute, max_speakers, floor,
                           decay_shift, d_mute_out, s);
}

// Over the layout and the legs' packet slots, in front of wmx_mix_load_minus_legs: that call's addressing and d_len convention.
int wmx_mix_select_speakers_legs(wmx_mix *m, const int16_t *d_src, uint32_t srcU8Len, long source_stride, long packet_stride, int max_packets,
                                 const uint32_t *d_len, const uint8_t *d_mute, int max_speakers, uint32_t floor, int decay_shift,
                                 uint8_t *d_mute_out, void *stream) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    const int rcc = speakers_check("wmx_mix_select_speakers_legs", m, d_src, srcU8Len, max_speakers, decay_shift, d_mute_out);
    if (rcc) return rcc;
    if (!d_len) {
        set_error("wmx_mix_select_speakers_legs: bad argument");
        return WMX_EINVAL;
    }
    if (max_packets < 1 || max_packets > WMX_MIX_MAX_LEG_PACKETS) {
        set_error("wmx_mix_select_speakers_legs: max_packets=%d must be 1 .. %d", max_packets, WMX_MIX_MAX_LEG_PACKETS);
        return WMX_EINVAL;
    }
    const long n_el = (long)(srcU8Len / 2);
    if ((max_packets > 1 && packet_stride < n_el) || (m->n_groups > 1 && source_stride < (long)(max_packets - 1) * packet_stride + n_el) ||
        packet_stride < 0) {
        set_error("wmx_mix_select_speakers_legs: rows of %ld elements overlap (packet_stride=%ld, source_stride=%ld, max_packets=%d)", n_el,
                  packet_stride, source_stride, max_packets);
        return WMX_EINVAL;
    }
    if (m->conf.n_conf < 1) {
        set_error("wmx_mix_select_speakers_legs: no layout (wmx_mix_set_conferences)");
        return WMX_EINVAL;
    }
    const int rcs = m->talkers.make();
    if (rcs) return rcs;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(speakers_clear_kernel, dim3(stream_grid((size_t)m->n_groups, 256)), dim3(256), 0, s, m->talkers.at<uint8_t>(kTalkerSpeaking), d_mute_out,
                       m->n_groups);
    WMX_LAUNCH_CHECK();
    const int n_slots = m->conf.slots();
    if (n_slots < 1) return 0;
    hipLaunchKernelGGL(select_speakers_legs_kernel, dim3(stream_grid((size_t)n_slots * 64, 256)), dim3(256), 0, s, d_src, srcU8Len / 2, srcU8Len,
                       source_stride, packet_stride, max_packets, d_len, (const int32_t *)m->d_conf_tab, (const int32_t *)m->d_conf_members, d_mute,
                       max_speakers, floor, decay_shift, m->talkers.at<uint32_t>(kTalkerEnv), m->talkers.at<uint8_t>(kTalkerSpeaking), d_mute_out, m->n_groups, n_slots);
    WMX_LAUNCH_CHECK();
    return 0;
}

// What a new call in a reused slot does to its ring: what the old call loaded ahead of the play head is gone.  Head and tick are the
// mixer's, not the ring's, and stay.
int wmx_mix_reset_rings(wmx_mix *m, const int32_t *host_idx, int n, void *stream) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    if (!m || (host_idx && n < 0)) return WMX_EINVAL;
    if (idx_check(host_idx, n, m->n_groups, "wmx_mix_reset_rings: ring", "mixer")) return WMX_EINVAL;
    hipStream_t s = as_stream(stream);
    if (!host_idx) {
        WMX_HIP(hipMemsetAsync(m->d_rings, 0, (size_t)m->ring_bytes * m->n_groups, s));
        return 0;
    }
    for (int i = 0; i < n; i++)  // a handful of legs at a time: one fill each, nothing of the list goes to the device
        WMX_HIP(hipMemsetAsync((uint8_t *)m->d_rings + (size_t)host_idx[i] * m->ring_bytes, 0, m->ring_bytes, s));
    return 0;
}

// env = 0; the speaking flags are the next selection's to write
int wmx_mix_reset_speakers(wmx_mix *m, const int32_t *host_idx, int n, void *stream) {
    WMX_ON_DEVICE(m);
    if (!m) return WMX_EINVAL;
    return m->talkers.reset("wmx_mix_reset_speakers: ring", host_idx, n, wmx::as_stream(stream), wmx::kTalkerEnv, wmx::kTalkerEnv + 1);
}

int wmx_mix_export_speakers(const wmx_mix *m, uint32_t *host_env, uint8_t *host_speaking, void *stream) {
    WMX_ON_DEVICE(m);
    if (!m) return WMX_EINVAL;
    return m->talkers.export_to({host_env, host_speaking}, wmx::as_stream(stream));
}

// the play thread's drain (src/wmix.c:1347-1366): read `bytes` at the ring head into d_out (per group), zero what
// was read, advance head and tick.
int wmx_mix_drain(wmx_mix *m, int16_t *d_out, uint32_t bytes, long out_stride, void *stream) {
    WMX_ON_DEVICE(m);
    using namespace wmx;
    if (!m || !d_out || (bytes & 1) || bytes > m->ring_bytes) return WMX_EINVAL;
    if (bytes == 0) return 0;
    const uint32_t n = bytes / 2;
    const unsigned grid = stream_grid((size_t)n * m->n_groups, 256);
    hipLaunchKernelGGL(drain_kernel, dim3(grid), dim3(256), 0, as_stream(stream), m->d_rings, m->ring_bytes / 2, d_out, n, m->head_off / 2,
                       out_stride, m->n_groups);
    WMX_LAUNCH_CHECK();
    m->head_off = (m->head_off + bytes) % m->ring_bytes;
    m->tick += bytes;
    return 0;
}

// legacy host form, src/wmix.h:40-49.  The ring format is the reference's compile-time WMIX_CHN x WMIX_FREQ; the
// default platform is 1 x 8000 (platform/alsa/plat.h:48-50).  A differently configured daemon sets
// WMIX_AMD_RING="chn,freq" in the environment, and one built for platform/hi3516 or platform/t31 WMIX_AMD_PLAY_CORRECT=0
// (PLAT_PLAY_CORRECT in bytes, plat.h:16; unset = platform/alsa's 200 ms).
WMix_Point wmix_load_data(WMix_Struct_Head *wmix, WMix_Point src, uint32_t srcU8Len, uint16_t freq, uint8_t channels, uint8_t sample,
                          WMix_Point head, uint8_t reduce, uint32_t *tick) {
    using namespace wmx;
    WMix_Point pHead = head;
    if (!wmix || !wmix->run || !src.U8 || srcU8Len < 1) return pHead;  // src/wmix.c:1663-1664
    static int ring_chn = 0, ring_freq = 0;
    static long play_correct = -1;  // -1: the default of wmx_mix_create
    if (!ring_chn) {
        const char *pc = getenv("WMIX_AMD_PLAY_CORRECT");
        char *endp = nullptr;
        if (pc && pc[0]) {
            const long v = strtol(pc, &endp, 10);
            if (endp && !*endp && v >= 0) play_correct = v;
        }
        ring_chn = 1;
        ring_freq = 8000;
        const char *env = getenv("WMIX_AMD_RING");
        int c = 0, f = 0;
        if (env && sscanf(env, "%d,%d", &c, &f) == 2 && (c == 1 || c == 2) && f >= 1000) {
            ring_chn = c;
            ring_freq = f;
        }
    }
    const uint32_t size = (uint32_t)(wmix->end.U8 - wmix->start.U8);
    // this thread's device ring: destroyed with the thread (a finished task thread of the daemon gives it back)
    struct MixOwner {
        wmx_mix *m = nullptr;
        ~MixOwner() {
            if (m && !runtime_exiting()) wmx_mix_destroy(m);
        }
    };
    static thread_local MixOwner owner;
    wmx_mix *&m = owner.m;
    if (!m || m->chn != ring_chn || m->freq != ring_freq) {
        if (m) wmx_mix_destroy(m);
        m = nullptr;
        if (wmx_mix_create(&m, 1, ring_chn, ring_freq) != 0) return pHead;
        {  // this ring only ever holds the span of one call: pinned host memory the kernel works on over PCIe (see legacy_stage.h)
            void *hp = nullptr, *dp = nullptr;
            if (hipHostMalloc(&hp, m->ring_bytes, hipHostMallocMapped | hipHostMallocPortable) == hipSuccess && hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
                (void)hipFree(m->d_rings);
                memset(hp, 0, m->ring_bytes);
                m->h_rings = static_cast<uint8_t *>(hp);
                m->d_rings = static_cast<int16_t *>(dp);
            } else {
                (void)hipGetLastError();
                if (hp) (void)hipHostFree(hp);
            }
        }
        if (play_correct >= 0 && wmx_mix_set_play_correct(m, (uint32_t)play_correct) != 0) {
            fprintf(stderr, "wmix_amd: WMIX_AMD_PLAY_CORRECT=%ld: %s\n", play_correct, wmx_last_error());
            wmx_mix_destroy(m);
            m = nullptr;
            return pHead;
        }
    }
    if (size != m->ring_bytes) {
        set_error("wmix_load_data: ring of %u bytes does not match WMIX_AMD_RING=%d,%d", size, ring_chn, ring_freq);
        fprintf(stderr, "wmix_amd: %s\n", wmx_last_error());
        return pHead;
    }
    m->head_off = (uint32_t)(wmix->head.U8 - wmix->start.U8);
    m->tick = wmix->tick;
    m->reduce_mode = wmix->reduceMode;
    uint32_t h = head.U8 ? (uint32_t)(head.U8 - wmix->start.U8) : UINT32_MAX, t = *tick;
    // The reference touches ring bytes [head, head + n_out*2) only, while other task threads and the play thread work on
    // the same ring without a lock (src/wmix.c:1347-1352, 1678-1702).  So does this adapter: the span the call will write
    // is worked out first (the cursor rule, then the schedule, which wmx_mix_load finds in the handle's cache afterwards), only
    // that span goes up, and only it comes back.  Between the two copies the adapter is a read-modify-write like the reference's
    // per-sample `*pHead = ...`, just longer: it gives no more atomicity than the reference does, and no less outside the span.
    uint32_t span_off = h, span_tick = t;
    mix_cursor_begin(cursor_state(m), span_off, span_tick);
    if (span_off >= size || (span_off & 1)) return pHead;
    SchedCache::Entry *ent = nullptr;
    int rcb;
    {
        DeviceScope on(m->device);  // the schedule goes where wmx_mix_load reads it
        rcb = on.err == hipSuccess ? load_sched(m, "wmix_load_data", srcU8Len, freq, channels, sample, &ent)
                                   : hip_fail(on.err, "hipSetDevice", __FILE__, __LINE__);
    }
    if (rcb) {
        fprintf(stderr, "wmix_amd: %s\n", rcb == WMX_EINVAL ? "wmix_load_data: unsupported rate ratio or more than one ring of output" : wmx_last_error());
        return pHead;
    }
    const uint32_t span = (uint32_t)ent->n * 2;
    const uint32_t first = span < size - span_off ? span : size - span_off, second = span - first;  // split at the wrap
    // the up-sampling fill interpolates towards the frame behind the last one (src/wmix.c:1857,1914); the copy and
    // down-sampling branches never read ahead, and neither does the adapter
    const bool reads_ahead = sample == 16 && (channels == 1 || channels == 2) && (int)freq < m->freq;
    const size_t src_bytes = (size_t)srcU8Len + (reads_ahead ? 2 * channels : 0);
    static thread_local Stage st;
    // six task threads of the daemon load side by side (src/wmixTask.c:85, 973, 1311, 1484, 1704, 1927): each on its own non-blocking
    // stream, waiting for that stream alone (wmx_internal.h: thread_stream)
    hipStream_t ts = thread_stream();
    // the span between the caller's ring and ours, split at the wrap: plain memcpy when ours is the mapped one, else copies on the stream
    const bool ring_mapped = m->h_rings != nullptr;
    auto move_span = [&](bool up) {
        const uint32_t at[2] = {span_off, 0}, len[2] = {first, second};
        for (int k = 0; k < 2; k++) {
            uint8_t *theirs = wmix->start.U8 + at[k], *ours = (ring_mapped ? m->h_rings : (uint8_t *)m->d_rings) + at[k];
            uint8_t *dst = up ? ours : theirs, *from = up ? theirs : ours;
            if (!len[k]) continue;
            if (ring_mapped)
                memcpy(dst, from, len[k]);
            else if (hipMemcpyAsync(dst, from, len[k], up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, ts) != hipSuccess)
                return false;
        }
        return true;
    };
    bool ok = st.begin(src_bytes, kMappedMaxBytes, {src_bytes + 8}) == 0;
    ok = ok && st.put(0, src.U8, src_bytes, ts) == 0 && move_span(true);
    ok = ok && wmx_mix_load(m, st.dev<const int16_t>(0), srcU8Len, freq, channels, sample, 1, 0, 0, reduce, &h, &t, ts) == 0;
    if (!ring_mapped) ok = ok && move_span(false);  // stream copies: queued before the one wait
    ok = (st.finish(ts) == 0) && ok;
    if (ring_mapped) ok = ok && move_span(false);  // memcpy: the kernel's writes are in host memory after the wait
    if (!ok) {
        (void)hipGetLastError();
        fprintf(stderr, "wmix_amd: wmix_load_data failed on the GPU: %s\n", wmx_last_error());
        return pHead;
    }
    *tick = t;
    pHead.U8 = wmix->start.U8 + h;
    return pHead;
}

// collision-free names of the legacy group for the daemon link shim (include/wmix_compat.h, daemon_shim.c)
WMix_Point wmx_compat_load_data(WMix_Struct_Head *wmix, WMix_Point src, uint32_t srcU8Len, uint16_t freq, uint8_t channels, uint8_t sample,
                                WMix_Point head, uint8_t reduce, uint32_t *tick) {
    return wmix_load_data(wmix, src, srcU8Len, freq, channels, sample, head, reduce, tick);
}
uint32_t wmx_compat_len_of_out(uint8_t inChn, uint16_t inFreq, uint32_t inLen, uint8_t outChn, uint16_t outFreq) {
    return wmix_len_of_out(inChn, inFreq, inLen, outChn, outFreq);
}
uint32_t wmx_compat_len_of_in(uint8_t inChn, uint16_t inFreq, uint8_t outChn, uint16_t outFreq, uint32_t outLen) {
    return wmix_len_of_in(inChn, inFreq, outChn, outFreq, outLen);
}
uint32_t wmx_compat_pcm_zoom(uint8_t inChn, uint16_t inFreq, uint8_t *in, uint32_t inLen, uint8_t outChn, uint16_t outFreq, uint8_t *out) {
    return wmix_pcm_zoom(inChn, inFreq, in, inLen, outChn, outFreq, out);
}

int wmx_mix_export(const wmx_mix *m, int group, int16_t *host_ring, uint32_t *head_off, uint32_t *tick) {
    WMX_ON_DEVICE(m);
    if (!m || group < 0 || group >= m->n_groups) return WMX_EINVAL;
    if (host_ring) {
        WMX_HIP(hipDeviceSynchronize());
        WMX_HIP(hipMemcpy(host_ring, (const uint8_t *)m->d_rings + (size_t)group * m->ring_bytes, m->ring_bytes, hipMemcpyDeviceToHost));
    }
    if (head_off) *head_off = m->head_off;
    if (tick) *tick = m->tick;
    return 0;
}

}  // extern "C"
