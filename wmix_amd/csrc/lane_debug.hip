// lane_debug.hip -- test hook for the lane-mask constants (wmx_internal.h lanes<>, lane_sites.h): every mask the kernels use,
// evaluated per lane beside the arithmetic predicate of the lane id it replaces.  One row per entry of WMX_LANE_SITES, generated
// from the same list the call sites take their masks from; nothing here is on the product path.
#include "wmx_internal.h"
#include "lane_sites.h"

namespace wmx {
namespace {

#define WMX_LANE_SITE_COUNT(name, mask, arith) +1
constexpr int kLaneSites = 0 WMX_LANE_SITES(WMX_LANE_SITE_COUNT);
#undef WMX_LANE_SITE_COUNT
#define WMX_LANE_SITE_NAME(name, mask, arith) #name,
const char *const kLaneSiteNames[] = {WMX_LANE_SITES(WMX_LANE_SITE_NAME)};
#undef WMX_LANE_SITE_NAME

// out[site][thread] = bit 0: lanes<mask>(), bit 1: the arithmetic predicate of lane = threadIdx.x & 63; threads that do not run
// leave their words alone
__device__ __forceinline__ void lane_sites_eval(int32_t *out, int threads, int t) {
    const int lane = t & 63;
    int row = 0;
#define WMX_LANE_SITE_EVAL(name, mask, arith) \
    out[(size_t)(row++) * threads + t] = (lanes<site::name>() ? 1 : 0) | ((arith) ? 2 : 0);
    WMX_LANE_SITES(WMX_LANE_SITE_EVAL)
#undef WMX_LANE_SITE_EVAL
}

// diverge_mask: the lanes (bit = lane id) that evaluate the masks, inside a divergent `if`; ~0: all of them, no branch around
__global__ void dbg_lane_sites(int32_t *out, uint64_t diverge_mask) {
    const int t = threadIdx.x, threads = blockDim.x;
    if (diverge_mask == ~0ull) {
        lane_sites_eval(out, threads, t);
    } else if ((diverge_mask >> (t & 63)) & 1ull) {
        lane_sites_eval(out, threads, t);
    }
}

}  // namespace
}  // namespace wmx

extern "C" int wmx_debug_lane_sites(void) { return wmx::kLaneSites; }

extern "C" const char *wmx_debug_lane_site_name(int site) {
    return site >= 0 && site < wmx::kLaneSites ? wmx::kLaneSiteNames[site] : nullptr;
}

extern "C" int wmx_debug_lane_masks(int block_threads, uint64_t diverge_mask, int32_t *d_out, void *stream) {
    using namespace wmx;
    if (block_threads < 64 || block_threads > 1024 || block_threads % 64 != 0 || !d_out) return WMX_EINVAL;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(dbg_lane_sites, dim3(1), dim3((unsigned)block_threads), 0, s, d_out, diverge_mask);
    WMX_LAUNCH_CHECK();
    WMX_HIP(hipStreamSynchronize(s));
    return 0;
}
