// mix_minus.h -- the algebra behind wmx_mix_load_minus (mix.hip): every participant of a conference hears the others.
//
// volumeAdd(x, c) (src/wmix.c:1617-1636) equals clamp16(x + c) for every pair of int16 -- its two `== 0` shortcuts return what the
// clamp returns -- and maps of the form x -> clamp(x + a, lo, hi) with lo <= hi are closed under composition.  So the P - 1 ordered
// wmix_load_data calls that fill participant q's ring, f_(P-1) o .. o f_(q+1) o f_(q-1) o .. o f_0 with f_s = clamp16(. + c_s), are a
// prefix map F_q = f_(q-1) o .. o f_0 followed by a suffix map G_q = f_(P-1) o .. o f_(q+1), and both families come out of one sweep
// each over the P sources: P source reads per ring column instead of P * (P - 1), saturation history included.  "Total minus own" is
// NOT this: the saturating add is order dependent.
//
// Plain C++ without HIP types: mix.hip includes it for the kernel, tests/test_mix_minus_host.py compiles it with g++ and compares
// G_q(F_q(x)) with the sequential volumeAdd loop.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define WMX_MINUS_FN __host__ __device__ inline
#else
#define WMX_MINUS_FN inline
#endif

namespace wmx {

// x -> clamp(x + a, lo, hi), lo <= hi.  |a| <= 32 * 32768 for WMX_MIX_MAX_PARTIES sources: int32 is ample.
struct ClampMap {
    int32_t a;
    int16_t lo, hi;
};

WMX_MINUS_FN int32_t clamp_i32(int32_t x, int32_t lo, int32_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

WMX_MINUS_FN ClampMap clamp_map_identity() { return ClampMap{0, INT16_MIN, INT16_MAX}; }

WMX_MINUS_FN int16_t clamp_map_apply(ClampMap m, int16_t x) { return (int16_t)clamp_i32((int32_t)x + m.a, m.lo, m.hi); }

// m, then volumeAdd(., c):   (a, lo, hi) -> (a + c, clamp16(lo + c), clamp16(hi + c))
WMX_MINUS_FN ClampMap clamp_map_then_add(ClampMap m, int16_t c) {
    return ClampMap{m.a + c, (int16_t)clamp_i32((int32_t)m.lo + c, INT16_MIN, INT16_MAX), (int16_t)clamp_i32((int32_t)m.hi + c, INT16_MIN, INT16_MAX)};
}

// volumeAdd(., c), then m:   (a, lo, hi) -> (c + a, clamp(LO + a, lo, hi), clamp(HI + a, lo, hi))
WMX_MINUS_FN ClampMap clamp_map_add_then(int16_t c, ClampMap m) {
    return ClampMap{m.a + c, (int16_t)clamp_i32(INT16_MIN + m.a, m.lo, m.hi), (int16_t)clamp_i32(INT16_MAX + m.a, m.lo, m.hi)};
}

}  // namespace wmx
