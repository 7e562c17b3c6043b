// lane_sites.h -- every lane-mask constant the kernels use (wmx_internal.h lanes<>), each beside the arithmetic predicate of the
// lane id it stands for.  A call site names its mask (lanes<site::aec_lane0>()); the debug kernel of lane_debug.hip is generated from
// the same list and evaluates, per lane, the mask and the arithmetic form side by side (tests/test_lane_masks_gpu.py), so a wrong
// mask cannot hide behind a test that still passes.
//     X(name, mask built with the constexpr builders, arithmetic predicate of `lane`)
// g = lane & 3 and gl = lane >> 2 are the transform and the index inside it of the register FFTs (fft_regs.h).
#pragma once
#include "wmx_internal.h"

#define WMX_LANE_SITES(X)                                                                                              \
    /* aec_block */                                                                                                    \
    X(aec_lane0, lane_eq(0), lane == 0)                                                                                \
    X(aec_lane1, lane_eq(1), lane == 1)                                                                                \
    X(aec_lower, lane_lt(32), lane < 32)                                                                               \
    X(aec_upper, lane_ge(32), lane >= 32)                                                                              \
    X(aec_upd8, lane_lt(8), lane < 8)                        /* lane < cnt, first pass of the filter update */         \
    X(aec_upd4, lane_lt(4), lane < 4)                        /* lane < cnt, second pass */                             \
    X(aec_parts, lane_lt(12), lane < 12)                                                                               \
    X(aec_pref24, lane_lt(24), lane < 24)                    /* lane < prefSize at 8 kHz */                            \
    X(aec_pref12, lane_lt(12), lane < 12)                    /* lane < prefSize at 16 kHz */                           \
    X(aec_win, lane_bit(0), ((lane & 3) & 1) != 0)           /* the windowed transforms: g odd */                      \
    X(aec_err, fft_g_ge(2), (lane & 3) >= 2)                 /* the error transforms */                                \
    X(aec_ef, fft_g_eq(2), (lane & 3) == 2)                  /* rdft([0 | e]) */                                       \
    /* fft_regs.h, HwLanes forms */                                                                                    \
    X(fft_p1_b1, fft_gl_eq(1), (lane >> 2) == 1)             /* pass 1, butterfly b = gl == 1 */                       \
    X(fft_p2_b1, fft_gl_hi_eq(1), ((lane >> 2) >> 2) == 1)   /* pass 2, butterfly b = gl >> 2 == 1 */                  \
    X(fft_inv_b0, fft_gl_eq(0), (lane >> 2) == 0)            /* rdft128_inv_point_m, b = gl == 0 */                    \
    X(fwd_lower, lane_lt(32), lane < 32)                     /* rdft128_fwd_coef */                                    \
    X(fwd_wr0, lane_eq(0) | lane_eq(32), (lane & 31) == 0)                                                             \
    X(fwd_lane0, lane_eq(0), lane == 0)                                                                                \
    X(fwd_lane32, lane_eq(32), lane == 32)                                                                             \
    X(inv_lower, lane_lt(32), lane < 32)                     /* rdft128_inv_point_lanes */                             \
    X(inv_lane0, lane_eq(0), lane == 0)                                                                                \
    X(inv_lane32, lane_eq(32), lane == 32)                                                                             \
    /* fft64_lanes: output j of butterfly b; pass 1 j = lane & 3, b = lane >> 2; pass 2 j = (lane >> 2) & 3, b = lane >> 4; */ \
    /* closing pass j = lane >> 4 */                                                                                   \
    X(l1_j_odd, lane_bit(0), ((lane & 3) & 1) != 0)                                                                    \
    X(l1_j_hi, lane_bit(1), ((lane & 3) & 2) != 0)                                                                     \
    X(l1_rot_p, fft_gl_eq(1) & every(4, 1), (lane >> 2) == 1 && ((lane & 3) & 1) && (lane & 3) == 1)                   \
    X(l1_rot_m, fft_gl_eq(1) & every(4, 3), (lane >> 2) == 1 && ((lane & 3) & 1) && (lane & 3) != 1)                   \
    X(l2_j_odd, lane_bit(2), (((lane >> 2) & 3) & 1) != 0)                                                             \
    X(l2_j_hi, lane_bit(3), (((lane >> 2) & 3) & 2) != 0)                                                              \
    X(l2_rot_p, lanes_where(0x3c, 0x14), (lane >> 4) == 1 && (((lane >> 2) & 3) & 1) && ((lane >> 2) & 3) == 1)        \
    X(l2_rot_m, lanes_where(0x3c, 0x1c), (lane >> 4) == 1 && (((lane >> 2) & 3) & 1) && ((lane >> 2) & 3) != 1)        \
    X(l3_j_odd, lane_bit(4), ((lane >> 4) & 1) != 0)                                                                   \
    X(l3_j_hi, lane_bit(5), ((lane >> 4) & 2) != 0)                                                                    \
    /* fft_ooura.h, the LDS executor under HwLanes: NC = 128 or 64 complex points, butterfly = lane */                 \
    X(oo128_act, lane_lt(32), lane < 128 / 4)                /* lane < NB */                                           \
    X(oo64_act, lane_lt(16), lane < 64 / 4)                                                                            \
    X(oo_p1_b1, lane_eq(1), lane == 1)                       /* pass 1: b = lane */                                    \
    X(oo_hc4_b1, fft_gl_eq(1), lane / 4 == 1)                /* stride 4: b = lane / 4 */                              \
    X(oo_hc16_b1, fft_gl_hi_eq(1), lane / 16 == 1)           /* stride 16: b = lane / 16 */                            \
    X(oo64_close, lane_lt(16), lane < 16)                    /* closing radix-4 of NC = 64: lane < HC */               \
    X(oo64_split, lane_lt(32), lane < 64 / 2)                /* fft_real_split of NC = 64: q = lane < NQ */            \
    X(oo_lane0, lane_eq(0), lane == 0)                                                                                 \
    /* ns_frame<L>, L = 128 (8 kHz) and 256 (16 / 32 kHz): site::ns<L> below, group k of 64 bins or samples */         \
    X(ns128_bin_ok, ns<128>::bin_ok(1), lane + 64 < 65)      /* the last group holds bin M - 1 alone */                \
    X(ns256_bin_ok, ns<256>::bin_ok(2), lane + 128 < 129)                                                              \
    X(ns128_old, ns<128>::old(0), lane < 48)                 /* i < KEEP in the group that mixes old and new samples */ \
    X(ns256_old, ns<256>::old(1), lane + 64 < 96)                                                                      \
    X(ns128_kept, ns<128>::kept(1), lane + 64 >= 80)         /* i >= B in the group the block boundary cuts */         \
    X(ns256_kept, ns<256>::kept(2), lane + 128 >= 160)                                                                 \
    X(ns128_tail, ns<128>::tail(), lane < 68 - 65)           /* lane < MP - M */                                       \
    X(ns256_tail, ns<256>::tail(), lane < 132 - 129)                                                                   \
    X(ns_dc, lane_eq(0), lane == 0)                          /* bin 0 (k == 0) */                                      \
    X(ns_from_band, lane_ge(5), lane >= 5)                   /* b >= kStartBand (k == 0) */                            \
    X(ns_from_1, lane_ge(1), lane >= 1)                      /* b >= 1, b > 0 (k == 0) */                              \
    X(ns_scalars, lane_lt(24), lane < 24)                                                                              \
    X(ns_lane0, lane_eq(0), lane == 0)                                                                                 \
    X(ns_pick1, lane_eq(1), lane == 1)                       /* the lanes of the ordered sums and of the three tanh */ \
    X(ns_pick2, lane_eq(2), lane == 2)                                                                                 \
    X(ns_pick3, lane_eq(3), lane == 3)                                                                                 \
    X(ns_pick4, lane_eq(4), lane == 4)                                                                                 \
    X(ns_pick5, lane_eq(5), lane == 5)

namespace wmx {
namespace site {
// the lane sets of ns_frame<L> that depend on the frame length: M bins, B new samples per frame, KEEP = L - B carried over, bin
// arrays padded to MP (ns_layout.h; ns.hip asserts that the numbers are the layout's)
template <int L>
struct ns {
    static constexpr int M = L / 2 + 1, MP = (M + 3) & ~3, B = L == 128 ? 80 : 160, KEEP = L - B;
    static constexpr uint64_t bin_ok(int k) { return lane_plus_lt(64 * k, M); }  // lane + 64 k < M
    static constexpr uint64_t old(int k) { return lane_plus_lt(64 * k, KEEP); }  // lane + 64 k < KEEP
    static constexpr uint64_t kept(int k) { return lane_plus_ge(64 * k, B); }    // lane + 64 k >= B
    static constexpr uint64_t tail() { return lane_lt(MP - M); }                 // lane < MP - M
};
#define WMX_LANE_SITE_CONST(name, mask, arith) constexpr uint64_t name = (mask);
WMX_LANE_SITES(WMX_LANE_SITE_CONST)
#undef WMX_LANE_SITE_CONST
}  // namespace site
}  // namespace wmx
