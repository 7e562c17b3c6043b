// spl_debug.hip -- test hooks: the fixed-point primitives of spl_dev.h / spl_fx.h run stand-alone on the device, so that `-m gpu`
// tests can sweep them against the reference's routines on the edge arguments that speech-like signals never produce inside a whole
// kernel (tests/test_spl_primitives_gpu.py).  Same headers and -fwrapv as vad.hip / agc.hip / nsx.hip / aecm.hip; nothing here is on
// the product path.
//   elementwise kinds: y[i] = f(a[i], b[i], c[i]); a, b, c are int32 and are narrowed the way the callee's parameter does ((int16_t),
//   (uint16_t), (uint32_t) conversions: the low bits are kept); operands a kind does not take are not read and may be NULL
//   kind 0   norm_w16((int16_t)a)                    kind 1   norm_w32(a)
//   kind 2   norm_u32((uint32_t)a)                   kind 3   size_in_bits((uint32_t)a)
//   kind 4   div_w32_w16(a, (int16_t)b)              kind 5   div_u32_u16((uint32_t)a, (uint16_t)b)
//   kind 6   sqrt_floor(a)                           kind 7   spl_sqrt(a)
//   kind 8   mul_rsft_round((int16_t)a, (int16_t)b, c), c in 1 .. 31
//   kind 9   agc_scalediff32(a, b, c)                kind 10  agc_mul32(a, b)
//   kind 11  spl_scalediff32(a, b, c)
//   kind 12  pk_abs16(a) (both int16 halves)         kind 13  pk_max_u16(a, b) (both uint16 halves)
//   wave kinds: a and y are [n / 64][64], n a multiple of 64; one wavefront per row with all 64 lanes on, as the reductions require;
//   every lane stores the value it holds after the reduction, so a result that is not wave-uniform shows
//   kind 16  wave_sum     kind 17  wave_max     kind 18  wave_min     kind 19  wave_umax     kind 20  wave_umin
#include "wmx_internal.h"
#include "spl_fx.h"

namespace wmx {
namespace {

constexpr int kSplWaveKind0 = 16, kSplKindLast = 20, kSplElemKindLast = 13;

template <int KIND>
__device__ __forceinline__ int32_t dbg_spl_one(int32_t a, int32_t b, int32_t c) {
    if constexpr (KIND == 0) return norm_w16((int16_t)a);
    if constexpr (KIND == 1) return norm_w32(a);
    if constexpr (KIND == 2) return norm_u32((uint32_t)a);
    if constexpr (KIND == 3) return size_in_bits((uint32_t)a);
    if constexpr (KIND == 4) return div_w32_w16(a, (int16_t)b);
    if constexpr (KIND == 5) return (int32_t)div_u32_u16((uint32_t)a, (uint16_t)b);
    if constexpr (KIND == 6) return sqrt_floor(a);
    if constexpr (KIND == 7) return spl_sqrt(a);
    if constexpr (KIND == 8) return mul_rsft_round((int16_t)a, (int16_t)b, c);
    if constexpr (KIND == 9) return agc_scalediff32(a, b, c);
    if constexpr (KIND == 10) return agc_mul32(a, b);
    if constexpr (KIND == 11) return spl_scalediff32(a, b, c);
    if constexpr (KIND == 12) return (int32_t)pk_abs16(a);
    if constexpr (KIND == 13) return (int32_t)pk_max_u16((uint32_t)a, (uint32_t)b);
    return 0;
}

// operands per kind
__host__ __device__ constexpr int dbg_spl_arity(int kind) {
    return (kind == 8 || kind == 9 || kind == 11) ? 3 : (kind == 4 || kind == 5 || kind == 10 || kind == 13) ? 2 : 1;
}

template <int KIND>
__global__ __launch_bounds__(256) void dbg_spl_elem(const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                    const int32_t *__restrict__ c, int32_t *__restrict__ y, size_t n) {
    constexpr int kArity = dbg_spl_arity(KIND);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] = dbg_spl_one<KIND>(a[i], kArity >= 2 ? b[i] : 0, kArity >= 3 ? c[i] : 0);
}

template <int KIND>
__global__ __launch_bounds__(64) void dbg_spl_wave(const int32_t *__restrict__ a, int32_t *__restrict__ y) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const int32_t v = a[i];
    int32_t r;
    if constexpr (KIND == 16)
        r = (int32_t)wave_sum((uint32_t)v);
    else if constexpr (KIND == 17)
        r = wave_max(v);
    else if constexpr (KIND == 18)
        r = wave_min(v);
    else if constexpr (KIND == 19)
        r = (int32_t)wave_umax((uint32_t)v);
    else
        r = (int32_t)wave_umin((uint32_t)v);
    y[i] = r;
}

}  // namespace
}  // namespace wmx

// d_a, d_b, d_c, d_y: device pointers to n int32 each; synchronises `stream`.
extern "C" int wmx_debug_spl(int kind, const int32_t *d_a, const int32_t *d_b, const int32_t *d_c, int32_t *d_y, size_t n, void *stream) {
    using namespace wmx;
    if (kind < 0 || kind > kSplKindLast || (kind > kSplElemKindLast && kind < kSplWaveKind0) || !d_a || !d_y) return WMX_EINVAL;
    const bool wave = kind >= kSplWaveKind0;
    if (!wave && ((dbg_spl_arity(kind) >= 2 && !d_b) || (dbg_spl_arity(kind) >= 3 && !d_c))) return WMX_EINVAL;
    if (wave && (n % 64 != 0 || n / 64 > 0x7fffffffu)) return WMX_EINVAL;
    if (n == 0) return 0;
    if (current_device() < 0) return WMX_ENODEV;
    hipStream_t s = as_stream(stream);
    const dim3 eg(stream_grid(n, 256)), eb(256), wg((unsigned)(n / 64)), wb(64);
#define WMX_DBG_ELEM(K) \
    case K: hipLaunchKernelGGL((dbg_spl_elem<K>), eg, eb, 0, s, d_a, d_b, d_c, d_y, n); break
#define WMX_DBG_WAVE(K) \
    case K: hipLaunchKernelGGL((dbg_spl_wave<K>), wg, wb, 0, s, d_a, d_y); break
    switch (kind) {
        WMX_DBG_ELEM(0);
        WMX_DBG_ELEM(1);
        WMX_DBG_ELEM(2);
        WMX_DBG_ELEM(3);
        WMX_DBG_ELEM(4);
        WMX_DBG_ELEM(5);
        WMX_DBG_ELEM(6);
        WMX_DBG_ELEM(7);
        WMX_DBG_ELEM(8);
        WMX_DBG_ELEM(9);
        WMX_DBG_ELEM(10);
        WMX_DBG_ELEM(11);
        WMX_DBG_ELEM(12);
        WMX_DBG_ELEM(13);
        WMX_DBG_WAVE(16);
        WMX_DBG_WAVE(17);
        WMX_DBG_WAVE(18);
        WMX_DBG_WAVE(19);
        default: hipLaunchKernelGGL((dbg_spl_wave<20>), wg, wb, 0, s, d_a, d_y); break;
    }
#undef WMX_DBG_ELEM
#undef WMX_DBG_WAVE
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e == hipSuccess ? 0 : hip_fail(e, "wmx_debug_spl", __FILE__, __LINE__);
}
