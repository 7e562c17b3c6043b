// wmx_internal.h -- shared host-side helpers for libwmix_amd.so (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/wmix_amd.h"
#include "build_flags.h"
#include "leg_calls.h"

// Fault injection (developer variant only: -DWMX_FAULT_INJECTION, recorded by wmx_build_info and refused by the Python mirror like every
// variant build).  Every runtime call that goes through WMX_HIP first passes a countdown; when it reaches zero the call is
// NOT made and reports hipErrorUnknown instead -- "call n of this entry point failed" -- so that tests can walk a fault through every
// fallible step of an entry point (tests/test_pipe_faults_gpu.py).  Armed by wmx_debug_fail_nth_hip_call(n) or, for the first arming,
// WMIX_AMD_FAIL_NTH_HIP_CALL=n in the environment; wmx_debug_hip_calls() = calls counted since the last arming.
#ifdef WMX_FAULT_INJECTION
namespace wmx {
hipError_t fault_point();
}
#define WMX_FAULT_OR(expr) (wmx::fault_point() != hipSuccess ? hipErrorUnknown : (expr))
#else
#define WMX_FAULT_OR(expr) (expr)
#endif

#define WMX_HIP(expr)                                                         \
    do {                                                                      \
        hipError_t _e = WMX_FAULT_OR(expr);                                   \
        if (_e != hipSuccess) return wmx::hip_fail(_e, #expr, __FILE__, __LINE__); \
    } while (0)

namespace wmx {

void set_error(const char *fmt, ...);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Device affinity of a handle.  The reference is one thread per device; a C host of ours runs one thread per GPU
// (SURVEY 8b "Threading") and must not depend on a thread-local current device: every handle
// records the device that was current when it was created and every entry point runs on it, restoring the caller's
// device afterwards.  hipGetDevice is a thread-local read; the switch happens only when the two differ.
int current_device();  // -1 (and the error set) when there is no usable device
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int dev) {
        if (dev < 0) return;
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            switched = err == hipSuccess;
        }
    }
    ~DeviceScope() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};

// Grid size for a grid-stride, HBM-bound kernel: enough workgroups to fill
// 256 CUs x 8 (guide: Guideline 11), never more than the work needs.
inline unsigned stream_grid(size_t work_items, unsigned block) {
    size_t need = (work_items + block - 1) / block;
    size_t cap = 256u * 8u;
    if (need < 1) need = 1;
    return (unsigned)(need < cap ? need : cap);
}

// ---- what the entry points that take a list of indices share (mix.hip, rtp.hip, conf.hip)
// Every host_idx[i] of the n (NULL: no list, nothing to check) lies inside the handle's `count`; otherwise WMX_EINVAL and the error
// text "<what> <index> is outside the <whose>'s <count>".
static inline int idx_check(const int32_t *host_idx, int n, int count, const char *what, const char *whose) {
    for (int i = 0; host_idx && i < n; i++)
        if (host_idx[i] < 0 || host_idx[i] >= count) {
            set_error("%s %d is outside the %s's %d", what, (int)host_idx[i], whose, count);
            return WMX_EINVAL;
        }
    return 0;
}

// ---- what the per-leg stages of the bridge share (wmx_nsx_process_legs, wmx_agc_process_legs, wmx_vad_process_legs): the rows of
// n_streams legs as [leg_stride][packet_stride] samples with max_packets slots per leg and their lengths.  The handle's own shape is
// the stage's check; `entry` names the entry point in the error text.
static inline int legs_rows_check(const char *entry, int n_streams, const int16_t *d_pcm, long leg_stride, long packet_stride,
                                  int max_packets, const uint32_t *d_len) {
    if (!d_pcm || !d_len || max_packets < 1 || max_packets > kLegMaxCalls) {
        set_error("%s: max_packets=%d must be 1 .. %d, and neither d_pcm nor d_len NULL", entry, max_packets, kLegMaxCalls);
        return WMX_EINVAL;
    }
    if (packet_stride < kLegRow || (n_streams > 1 && leg_stride < packet_stride * max_packets)) {
        set_error("%s: rows that overlap (packet_stride %ld < %d, or leg_stride %ld shorter than %d rows)", entry, packet_stride, kLegRow,
                  leg_stride, max_packets);
        return WMX_EINVAL;
    }
    if (reinterpret_cast<uintptr_t>(d_pcm) % sizeof(int16_t) != 0) {  // the strides count samples: every row is then where d_pcm is
        set_error("%s: d_pcm %p is not on a 2-byte boundary (the rows are read and written as int16)", entry, (const void *)d_pcm);
        return WMX_EINVAL;
    }
    return 0;
}

// A device block of state made by the first call that needs it: zero, except fill_bytes at fill_off that hold the byte `fill`;
// complete on the device when this returns.
static inline int zeroed_block(void **out, size_t bytes, const char *what, size_t fill_off = 0, int fill = 0, size_t fill_bytes = 0) {
    void *p = nullptr;
    WMX_HIP(hipMalloc(&p, bytes));
    hipError_t e = hipMemset(p, 0, bytes);
    if (e == hipSuccess && fill_bytes) e = hipMemset(static_cast<uint8_t *>(p) + fill_off, fill, fill_bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)hipFree(p);
        return hip_fail(e, what, __FILE__, __LINE__);
    }
    *out = p;
    return 0;
}

// The n indices of a host list in a device buffer the handle keeps and grows: a launch in flight on `s` may still read the list that
// is rewritten here, so the stream is waited for first.
static inline int upload_idx(int32_t *&d_idx, size_t &cap, const int32_t *host_idx, int n, hipStream_t s) {
    WMX_HIP(hipStreamSynchronize(s));
    if ((size_t)n > cap) {
        if (d_idx) (void)hipFree(d_idx);
        d_idx = nullptr, cap = 0;
        WMX_HIP(hipMalloc(&d_idx, (size_t)n * sizeof(int32_t)));
        cap = (size_t)n;
    }
    WMX_HIP(hipMemcpy(d_idx, host_idx, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    return 0;
}

// True once the process has begun to exit (an atexit handler registered when the library is loaded, i.e. after the HIP
// runtime's own handlers, so it runs before them; also the library's destructor).  Thread-local owners of device memory
// free it normally when their thread ends and leave it alone only then: the HIP runtime may already be gone, and a
// finished task thread of the daemon (src/wmixTask.c starts one per play / record task) must not leak its buffers
// (round-2 ADVICE).
bool runtime_exiting();

// Device-resident schedules (gather lists, load schedules) the host builds per format.  An entry, once uploaded, is never
// overwritten while other work may read it (round-1 ADVICE: the scratch buffers used to be rewritten by the next call).
// A cache holds at most kMax entries; a new format beyond that evicts the least recently used ONE, after waiting for the
// event recorded behind the last kernel that read it (round-2 ADVICE: no device-wide synchronisation, no mass eviction),
// on the device the entry lives on (a thread-local cache may hold entries of several devices).  The upload is a blocking
// copy, once per format.
struct SchedCache {
    struct Entry {
        uint64_t k0, k1;
        void *p;
        size_t n;  // elements
        int device;
        uint64_t last_use;
        hipEvent_t ev;  // recorded by used(); nullptr until the first kernel has read the entry
    };
    static constexpr size_t kMax = 64;
    // a list, not a vector: callers keep Entry pointers across add()
    std::vector<Entry *> e;
    uint64_t tick = 0;
    SchedCache() = default;
    SchedCache(const SchedCache &) = delete;
    SchedCache &operator=(const SchedCache &) = delete;
    Entry *find(uint64_t k0, uint64_t k1) {
        for (Entry *x : e)
            if (x->k0 == k0 && x->k1 == k1) {
                x->last_use = ++tick;
                return x;
            }
        return nullptr;
    }
    static void drop(Entry *x) {
        if (!runtime_exiting()) {
            DeviceScope on(x->device);
            if (x->ev) {
                (void)hipEventSynchronize(x->ev);
                (void)hipEventDestroy(x->ev);
            }
            if (x->p) (void)hipFree(x->p);
        }
        delete x;
    }
    // returns 0 and *out on success, a WMX error otherwise
    int add(uint64_t k0, uint64_t k1, const void *host, size_t bytes, size_t n, Entry **out) {
        if (e.size() >= kMax) {
            size_t lru = 0;
            for (size_t i = 1; i < e.size(); i++)
                if (e[i]->last_use < e[lru]->last_use) lru = i;
            drop(e[lru]);
            e.erase(e.begin() + (long)lru);
        }
        int dev = -1;
        WMX_HIP(hipGetDevice(&dev));
        void *p = nullptr;
        if (bytes) {
            WMX_HIP(hipMalloc(&p, bytes));
            hipError_t er = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
            if (er != hipSuccess) {
                (void)hipFree(p);
                return hip_fail(er, "hipMemcpy(schedule)", __FILE__, __LINE__);
            }
        }
        Entry *x = new Entry{k0, k1, p, n, dev, ++tick, nullptr};
        e.push_back(x);
        *out = x;
        return 0;
    }
    // call after launching the kernel that reads `x` on stream `s`
    int used(Entry *x, hipStream_t s) {
        if (!x->ev) WMX_HIP(hipEventCreateWithFlags(&x->ev, hipEventDisableTiming));
        WMX_HIP(hipEventRecord(x->ev, s));
        return 0;
    }
    void clear() {
        for (Entry *x : e) drop(x);
        e.clear();
    }
    ~SchedCache() { clear(); }
};

// The legacy adapters' launch streams (round-5 VERDICT weak 4).  The reference calls its per-handle functions from many threads at once --
// wmix_load_data from six task threads, agc_addition from the message thread, the four-call heartbeat from the record thread (SURVEY 8b
// "Threading"; src/wmixTask.c:85, 973, 1311, 1484, 1704, 1927; src/wmix.c:1070) -- and rounds 1-5 put every one of those launches on the
// legacy NULL stream and waited with hipStreamSynchronize(NULL): each caller waited for all the others' launches, and a batch running
// on a blocking stream of the same process stalled them all (and was stalled by them).  Now: one NON-BLOCKING stream per compat handle
// (legacy_stream_create; the handle's calls are ordered among themselves whatever thread makes them) and one per THREAD for the
// stateless adapters (thread_stream: G.711, wmix_pcm_zoom, wmix_load_data, math/fft.c), at the device's highest priority -- a legacy call
// is a few hundred samples somebody waits for.  nullptr (the NULL stream, the old behaviour) only if the runtime refuses a stream.
// Measured (examples/host_legacy_threads.c, profiles/r06/legacy_threads.jsonl): the heartbeat beside the six loaders and the
// agc_addition thread costs what it costs alone (p99 ratio 1.0).  Beside a BATCH that saturates the device it still waits -- not for a
// stream, for the hardware: a launch from another queue is served when the batch's running kernel has issued its workgroups, so the
// wait grows with the batch's launch size (p50 per heartbeat of four calls: 0.21 ms alone, 0.28 ms beside 1 024-stream launches, 0.63
// beside 16 384, 1.2 beside 65 536).  Stream priority does not change that, and compute units reserved with a CU mask made it worse
// (tried, round 6).  A gateway that serves legacy callers and a batch on one device keeps its launches small (wmx_rt's sub-batches).
hipStream_t legacy_stream_create();
void legacy_stream_destroy(hipStream_t s);
hipStream_t thread_stream();

// chain.hip -> aec.hip: let the far kernel of the next wmx_aec_run_* call start at this point of `stream` (see aec.hip)
int aec_fork_far(wmx_aec *h, hipStream_t stream);
// the caller returns without the AEC call the fork was made for: the next wmx_aec_run_* starts on its own stream again
void aec_cancel_fork(wmx_aec *h);
// the same for the fixed-point canceller's far kernel (beside the NSX)
int aecm_fork_far(wmx_aecm *h, hipStream_t stream);
void aecm_cancel_fork(wmx_aecm *h);
// pipe.hip -> chain.hip: an event the next wmx_chain_process call records between the noise suppressor and the echo canceller
void chain_gate_after_ns(wmx_chain *h, hipEvent_t ev);
// tick.hip -> chain.hip: the cohorts a canceller switched on later (wmx_chain_set_stages) is made with
void chain_cohorts_when_made(wmx_chain *h, int n_cohorts, const int32_t *stream_cohort);

// wmix_pcm_zoom's cursor walk (src/wmix.c:139-222) as a gather list: out int16 i <- in int16 idx[i]; identical formats
// give the identity (the reference's memcpy branch).  Defined in mix.hip.
void zoom_gather_list(int inChn, int inFreq, uint32_t inLen, int outChn, int outFreq, std::vector<int32_t> &idx);

// rtp.hip -> mix.hip: what wmx_rtp_egress_rings reads of a mixer, and the advance of head and tick that wmx_mix_drain makes
struct MixPlayView {
    int device, n_groups, chn, freq;
    uint32_t ring_bytes, head_off;
    int16_t *d_rings;
};
MixPlayView mix_play_view(const wmx_mix *m);
void mix_played(wmx_mix *m, uint32_t bytes);

// conf.hip -> rtp.hip: whether the coming wmx_rtp_record_rings has a tap that writes a row (leg_record.h; the host's copy of the state)
bool rtp_record_running(const wmx_rtp *h);

#ifdef __HIPCC__
// Hand-off of LDS data between lanes of ONE wavefront.  A wave's LDS instructions are executed in issue order by the
// hardware, so a ds_read issued after a ds_write of another lane of the same wave already sees the data.  What is needed
// is only that the COMPILER keeps the order: a wavefront-scope fence (no s_waitcnt vmcnt(0), no s_barrier -- unlike
// __syncthreads(), which would also drain every outstanding global load/store at each of the ~40 LDS phases of a block).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}
// Lane-per-stream kernels (VAD, AGC) walk their state field by field along a sequential dependency chain, one wave
// per SIMD: every first touch of a field would expose a full HBM round trip.  touch_line() requests a line up front
// (result discarded; loads return in order, so ordinary loads behind the touches are still waited for correctly);
// the chain then runs against L2.
// The load's result arrives asynchronously, so its destination must be a register the compiler keeps reserved until
// the wave has waited for every touch: `sink` is threaded through all touches as a read-write operand and pinned by
// touch_done() at the end of the kernel.
__device__ __forceinline__ void touch_line(const void *p, int &sink) {
    asm volatile("global_load_ubyte %0, %1, off" : "+v"(sink) : "v"(p) : "memory");
}
// ---- wave-uniform rows in HBM: SGPR row pointer + 32-bit lane offset
// A wave-per-stream kernel reads and writes its stream's state as `st[ARRAY + bin]` with a wave-uniform `st`.  Left to itself
// the compiler folds everything into one 64-bit per-lane address per access (v_lshl_add_u64, plus a v_add_co / v_addc_co pair
// when the array lies beyond the 4 KB immediate range) -- vector instructions in kernels that are bound by vector issue.
// global_row() forms the array's address on the scalar unit and keeps it an SGPR pair (the empty asm stops the folding; it
// also strips the address space, which is restated -- accesses through a laundered generic pointer become FLAT instructions);
// row_ld / row_st add the lane's 32-bit byte offset: global_load / global_store in their `v_off, s[row]` form.
typedef float __attribute__((address_space(1))) *GlobalF;
typedef const float __attribute__((address_space(1))) *GlobalCF;
__device__ __forceinline__ GlobalF global_row(float *uniform_base, int word) {
    float *p = uniform_base + word;
    asm("" : "+s"(p));
    return (GlobalF)p;
}
__device__ __forceinline__ GlobalCF global_row(const float *uniform_base, int word) {
    const float *p = uniform_base + word;
    asm("" : "+s"(p));
    return (GlobalCF)p;
}
__device__ __forceinline__ float row_ld(GlobalCF row, unsigned idx) {
    return *(GlobalCF)((const char __attribute__((address_space(1))) *)row + 4u * idx);
}
__device__ __forceinline__ void row_st(GlobalF row, unsigned idx, float v) {
    *(GlobalF)((char __attribute__((address_space(1))) *)row + 4u * idx) = v;
}

// ---- values kept in a VGPR for the rest of the kernel
// A lane constant that a kernel forms once (a coefficient vector, an address) and wants to KEEP: behind the empty asm the value has
// no origin, so the register allocator can neither rematerialise it at every use nor fold it back into the instructions that made
// it.  Costs nothing at run time.  Use it with all 64 lanes active: a value formed under a divergent branch is garbage in the others.
__device__ __forceinline__ void pin_vgpr(float &x) { asm volatile("" : "+v"(x)); }

// ---- lane predicates as scalar mask constants
// A test such as `lane == 0`, `lane < 32` or `(lane & 3) == 2` selects a set of lanes that is known when the kernel is compiled, but
// the compiler cannot know that `lane` is the hardware lane id and spends a v_cmp (and often the v_and / v_lshr in front of it) per
// test on the vector ALU.  lanes<M>() is the same predicate taken from the scalar side: "this lane is in M", bit l of M standing for
// hardware lane l, ANDed with EXEC as every predicate is.  A select on it is s_mov_b64 + v_cndmask_b32, an `if` an s_and_saveexec_b64
// of the constant; no vector compare.
// PRECONDITION: the caller's `lane` IS the hardware lane id -- wave64, lane = threadIdx.x & 63 (or threadIdx.x in a 64-thread
// block) and a block size that is a multiple of 64.  A kernel that relabels its lanes keeps the arithmetic form.
// tests/test_lane_masks_gpu.py evaluates every mask in use (lane_sites.h) beside the arithmetic predicate it replaces.
template <uint64_t M>
__device__ __forceinline__ bool lanes() {
    return __builtin_amdgcn_inverse_ballot_w64(M);
}
// ... and for a mask that is a constant only once its loop is unrolled (the group index k of a `#pragma unroll` loop is no constant
// expression): `m` must be the same in every lane, and must fold to a constant for the predicate to be free
__device__ __forceinline__ bool lanes_in(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
// HwLanes: tag of the overloads (fft_ooura.h, fft_regs.h) for callers whose `lane` is the hardware lane id: every predicate of the lane
// alone is then a mask constant of lane_sites.h.  The overloads without the tag keep the arithmetic form and hold under any mapping.
struct HwLanes {};
// the mask builders: call sites read as the test they replace
constexpr uint64_t lane_lt(int n) { return n <= 0 ? 0ull : (n >= 64 ? ~0ull : (1ull << n) - 1ull); }  // lane < n
constexpr uint64_t lane_ge(int n) { return ~lane_lt(n); }                                             // lane >= n
constexpr uint64_t lane_eq(int n) { return n < 0 || n > 63 ? 0ull : 1ull << n; }                      // lane == n
constexpr uint64_t lane_plus_lt(int off, int n) { return lane_lt(n - off); }                           // lane + off < n
constexpr uint64_t lane_plus_ge(int off, int n) { return lane_ge(n - off); }                           // lane + off >= n
constexpr uint64_t lanes_where(int and_mask, int value) {                                            // (lane & and_mask) == value
    uint64_t m = 0;
    for (int l = 0; l < 64; l++)
        if ((l & and_mask) == value) m |= 1ull << l;
    return m;
}
constexpr uint64_t every(int period, int phase) {  // lane % period == phase
    uint64_t m = 0;
    for (int l = 0; l < 64; l++)
        if (l % period == phase) m |= 1ull << l;
    return m;
}
constexpr uint64_t lane_bit(int k) { return lanes_where(1 << k, 1 << k); }  // bit k of the lane id is set
// the lane sets of the register FFTs (fft_regs.h): a transform is the 16 lanes with the same g = lane & 3, gl = lane >> 2 its index
constexpr uint64_t fft_g_eq(int g) { return every(4, g); }                   // g == n
constexpr uint64_t fft_g_ge(int g) {                                         // g >= n
    uint64_t m = 0;
    for (int k = g < 0 ? 0 : g; k < 4; k++) m |= every(4, k);
    return m;
}
constexpr uint64_t fft_gl_eq(int n) { return lanes_where(0x3c, n << 2); }    // gl == n          (pass 1: butterfly b = gl)
constexpr uint64_t fft_gl_hi_eq(int n) { return lanes_where(0x30, n << 4); }  // (gl >> 2) == n  (pass 2: butterfly b = gl >> 2)

// refill of block-layout state ([stream][words]) for a list of streams: one workgroup per listed stream
template <class T>
__global__ void fill_rows_idx(T *state, const T *tmpl, int words, const int32_t *idx, int n_idx) {
    for (int j = blockIdx.x; j < n_idx; j += gridDim.x) {
        T *dst = state + (size_t)idx[j] * words;
        for (int i = threadIdx.x; i < words; i += blockDim.x) dst[i] = tmpl ? tmpl[i] : T(0);
    }
}
// a stream takes part in a launch when it exists and the batch's active mask (if any) has it switched on; wave-uniform
// callers get a scalar byte load
__device__ __forceinline__ bool stream_active(const uint8_t *active, int sidx, int n_streams) {
    return sidx < n_streams && (!active || active[sidx] != 0);
}
__device__ __forceinline__ void touch_done(int &sink) { asm volatile("s_waitcnt vmcnt(0)" : "+v"(sink) : : "memory"); }
#endif

}  // namespace wmx

#define WMX_LAUNCH_CHECK() WMX_HIP(hipGetLastError())

// first statement of every entry point that takes a handle (null-safe: the null check follows it)
#define WMX_ON_DEVICE(h)                              \
    wmx::DeviceScope _dev_scope((h) ? (h)->device : -1); \
    WMX_HIP(_dev_scope.err)
