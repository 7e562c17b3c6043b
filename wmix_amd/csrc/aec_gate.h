// aec_gate.h -- the two decisions SmoothedPSD takes from sdSum and seSum (oracle/orc_aec.c:241-256, aec_core.c:333-386)
// without the two ordered 65-term sums, wherever the outcome cannot depend on the order of the additions.
//
//     divergeState = (divergeState ? 1.05f : 1.0f) * seSum > sdSum
//     reset wfBuf    if seSum > 19.95f * sdSum
//
// are all the reference does with the two sums.  Every term is non-negative: sd[i] = gc0 * sd[i] + gc1 * |d_i|^2 and the
// same for se, both zero when the handle is made (a NaN in a term is a NaN in any sum of them: handled below).  For
// non-negative terms no addition cancels, and a float addition has no underflow error, so ANY order of the 64 additions lands
// within gamma_64 = 64u / (1 - 64u), u = 2^-24, of the exact sum S (Higham, Accuracy and Stability, section 4.2):
//     ordered sum = S (1 + a),  lane-parallel sum = S (1 + a'),   |a|, |a'| <= gamma_64 = 3.82e-6.
// The reference compares fl(f * seSum) with sdSum and seSum with fl(19.95f * sdSum); here the same expressions are formed
// from the parallel sums sd_t, se_t.  Between the reference's two sides and ours lie at most: the two sums' errors on each side
// (4 gamma_64 in the ratio of the sides), the rounding of the product on each side (2u; relative only while the product is a
// normal number, hence the range check) and the rounding of the band's own product sd_t * (1 +- delta) (u) -- 4 gamma_64 + 3u
// < 1.55e-5 relative.  With delta = 2^-14 = 6.1e-5, four times that, a comparison that holds with the band on its far side
// holds for the reference's operands:
//     f * se_t > sd_t * (1 + delta)  =>  f * seSum > sdSum,        f * se_t < sd_t * (1 - delta)  =>  not,
// and the same around 19.95f * sd_t.  Inside the band, and for anything the argument does not cover -- a NaN or an infinity in a
// sum, a sum outside [2^-100, 2^100] (products that leave the normal range; all-zero rows) -- `decided` is 0 and the caller
// runs the ordered sums as before.  Both decisions must be clear for `decided` to be set.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WMX_GATE_HD __host__ __device__
#else
#define WMX_GATE_HD
#endif

namespace wmx {

struct AecGate {
    int decided, diverge, reset;
};

WMX_GATE_HD inline AecGate aec_gate_decide(float sd_t, float se_t, int prev_diverge) {
    const float lo = 0x1p-100f, hi = 0x1p100f, up = 1.f + 0x1p-14f, dn = 1.f - 0x1p-14f;
    // (a NaN slips through fminf / fmaxf and then fails all four comparisons below: undecided)
    const bool in_range = fminf(sd_t, se_t) >= lo && fmaxf(sd_t, se_t) <= hi;
    const float fse = (prev_diverge ? 1.05f : 1.0f) * se_t, rsd = 19.95f * sd_t;
    const bool div_yes = fse > sd_t * up, div_no = fse < sd_t * dn;
    const bool rst_yes = se_t > rsd * up, rst_no = se_t < rsd * dn;
    AecGate r;
    r.decided = (in_range && (div_yes || div_no) && (rst_yes || rst_no)) ? 1 : 0;
    r.diverge = div_yes ? 1 : 0;
    r.reset = rst_yes ? 1 : 0;
    return r;
}

// The order in which the device adds (aec_gate_wave_sums): inside every group of 16 lanes a butterfly over lane ^ 1, ^ 2, ^ 7, ^ 15,
// then (row 1 + row 3) + (row 0 + row 2), then bin 64.  The host form below adds the same pairs, so both give the same float; the
// argument above needs no particular order.
inline float aec_gate_sum_host(const float *x) {  // x[0..64]
    float row[4];
    for (int r = 0; r < 4; r++) {
        float v[16], w[16];
        for (int i = 0; i < 16; i++) v[i] = x[16 * r + i];
        const int steps[4] = {1, 2, 7, 15};
        for (int s = 0; s < 4; s++) {
            for (int i = 0; i < 16; i++) w[i] = v[i] + v[i ^ steps[s]];
            for (int i = 0; i < 16; i++) v[i] = w[i];
        }
        row[r] = v[15];
    }
    return ((row[1] + row[3]) + (row[0] + row[2])) + x[64];
}

#if defined(__HIPCC__)
// Sums of a and of b over the 64 lanes of the wave, side by side, as wave-uniform values.  DPP adds -- quad_perm [1,0,3,2],
// [2,3,0,1], row_half_mirror, row_mirror -- leave every lane of a row with its row's sum of each; one v_permlane32_swap then puts
// a's sums of rows r and r + 2 into the lower half of the wave and b's into the upper half, one add joins them, and row_bcast:15
// into rows 1 and 3 completes a's sum in lane 31 and b's in lane 63.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float aec_gate_dpp(float x) {  // lanes outside ROW_MASK receive the `old` operand, 0
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ void aec_gate_wave_sums(float &a, float &b) {
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    a = a + aec_gate_dpp<0xB1, 0xf>(a), b = b + aec_gate_dpp<0xB1, 0xf>(b);    // quad_perm:[1,0,3,2]
    a = a + aec_gate_dpp<0x4E, 0xf>(a), b = b + aec_gate_dpp<0x4E, 0xf>(b);    // quad_perm:[2,3,0,1]
    a = a + aec_gate_dpp<0x141, 0xf>(a), b = b + aec_gate_dpp<0x141, 0xf>(b);  // row_half_mirror
    a = a + aec_gate_dpp<0x140, 0xf>(a), b = b + aec_gate_dpp<0x140, 0xf>(b);  // row_mirror
    // lanes 0..31: (a of the own row, a of the row 32 lanes up); lanes 32..63: (b of the row 32 lanes down, b of the own row)
    const v2u r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    float s = __uint_as_float(r.x) + __uint_as_float(r.y);
    s = s + aec_gate_dpp<0x142, 0xa>(s);  // row_bcast:15 -> rows 1, 3
    a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), 31));
    b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), 63));
}

// The reference's own sums: lane 0 adds sd[0..64], lane 1 adds se[0..64], index order each, side by side (rows in LDS, 16-byte
// aligned).  The path every block took until the gate, and the one an undecided block takes.
__device__ __forceinline__ void aec_gate_ordered_sums(const float *sd, const float *se, int lane, float &sdSum, float &seSum) {
    const float *mine = lane == 1 ? se : sd;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 64; i += 8) {
        const float4 a = *reinterpret_cast<const float4 *>(mine + i), b = *reinterpret_cast<const float4 *>(mine + i + 4);
        acc += a.x;
        acc += a.y;
        acc += a.z;
        acc += a.w;
        acc += b.x;
        acc += b.y;
        acc += b.z;
        acc += b.w;
    }
    acc += mine[64];
    sdSum = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 0));
    seSum = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 1));
}
#endif

}  // namespace wmx
