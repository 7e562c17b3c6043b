// legacy_stage.h -- the ONE way a legacy adapter (host pointers in, host pointers out: include/wmix_compat.h, math/fft.h) gets the
// caller's bytes to a kernel and the result back.  A call is
//
//     begin(staged bytes, threshold, {region sizes})   pick the mode, make room, lay the regions out
//     put(region, src, bytes, stream)                   caller bytes into a region
//     dev(region)                                       the pointer the wmx_* entry point gets
//     get(region, dst, bytes)                           after a launch that succeeded: where the region's bytes go
//     finish(stream)                                    ALWAYS, also when the launch failed: results out, the stream waited for
//
// and runs in one of two modes the adapter cannot tell apart:
//
//   mapped   pinned HOST memory mapped into the device.  A legacy call moves a few hundred bytes, and two runtime copies around the
//            launch cost several times the work (wmix_pcm_zoom of one package: 43 us with copies; a compat handle's call ~ 45 us, of
//            which the kernel ~ 8).  The kernel reads and writes the buffer over PCIe instead: memcpy in, one launch, one
//            hipStreamSynchronize, memcpy out.  No other runtime call once the buffer is large enough.
//   copied   device memory and hipMemcpyAsync on the call's stream, all waited for by the one hipStreamSynchronize of finish(): above
//            the caller's threshold the DMA engines win, and it is what is left when the pinned allocation fails.
//
// An instance belongs to a compat handle or is thread_local.  Either buffer grows (never below 4 096 bytes, never shrinks) and is
// freed with its owner -- a finished task thread of the daemon gives its staging back (round-2 ADVICE) -- unless the process is
// exiting (runtime_exiting()).  The device buffer follows its thread: a thread that moved to another device gets a fresh one there.
#pragma once
#include <initializer_list>
#include "wmx_internal.h"

namespace wmx {

struct Stage {
    static constexpr int kMaxRegions = 6;
    static constexpr size_t kAlways = SIZE_MAX;  // threshold of a caller that is mapped at every size
    Stage() = default;
    Stage(const Stage &) = delete;
    Stage &operator=(const Stage &) = delete;
    ~Stage() {
        if (runtime_exiting()) return;
        if (host) (void)hipHostFree(host);
        drop_device();
    }

    // `staged` bytes of the caller's against `mapped_max` decide the mode; every region starts on a 16-byte boundary
    int begin(size_t staged, size_t mapped_max, std::initializer_list<size_t> sizes) {
        size_t need = 0;
        int r = 0;
        n_out = 0;
        for (size_t bytes : sizes) {
            off[r++] = need;
            need += (bytes + 15) & ~(size_t)15;
        }
        if (need < 4096) need = 4096;
        mapped = staged <= mapped_max && ensure_mapped(need);
        return mapped ? 0 : ensure_device(need);
    }
    template <class T>
    T *dev(int r) const {
        return reinterpret_cast<T *>((mapped ? host_dev : dmem) + off[r]);
    }
    int put(int r, const void *src, size_t bytes, hipStream_t s) {
        if (mapped)
            memcpy(host + off[r], src, bytes);
        else  // a pageable source: finish() waits for the stream before the caller has it back
            WMX_HIP(hipMemcpyAsync(dmem + off[r], src, bytes, hipMemcpyHostToDevice, s));
        return 0;
    }
    void get(int r, void *dst, size_t bytes) {
        if (bytes) out[n_out++] = {dst, off[r], bytes};
    }
    // after it nothing of this call can still touch the buffer, whatever failed before
    int finish(hipStream_t s) {
        hipError_t e = hipSuccess;
        for (int i = 0; !mapped && i < n_out && e == hipSuccess; i++)
            e = hipMemcpyAsync(out[i].dst, dmem + out[i].off, out[i].bytes, hipMemcpyDeviceToHost, s);
        const hipError_t waited = hipStreamSynchronize(s);
        if (e == hipSuccess) e = waited;
        for (int i = 0; mapped && i < n_out && e == hipSuccess; i++) memcpy(out[i].dst, host + out[i].off, out[i].bytes);
        n_out = 0;
        return e == hipSuccess ? 0 : hip_fail(e, "legacy staging: results out", __FILE__, __LINE__);
    }

private:
    struct Out {
        void *dst;
        size_t off, bytes;
    };
    uint8_t *host = nullptr, *host_dev = nullptr, *dmem = nullptr;  // the pinned buffer, the device's view of it; the device buffer
    size_t host_cap = 0, dmem_cap = 0;
    int device = -1;  // of dmem
    bool mapped = false;
    int n_out = 0;
    size_t off[kMaxRegions];
    Out out[kMaxRegions];

    bool ensure_mapped(size_t bytes) {
        if (bytes <= host_cap) return true;
        if (host) (void)hipHostFree(host);
        host = host_dev = nullptr;
        host_cap = 0;
        void *hp = nullptr, *dp = nullptr;
        if (hipHostMalloc(&hp, bytes, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess || hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) {
            (void)hipGetLastError();
            if (hp) (void)hipHostFree(hp);
            return false;
        }
        host = static_cast<uint8_t *>(hp);
        host_dev = static_cast<uint8_t *>(dp);
        host_cap = bytes;
        return true;
    }
    void drop_device() {
        if (!dmem) return;
        DeviceScope on(device);
        (void)hipFree(dmem);
        dmem = nullptr;
        dmem_cap = 0;
    }
    int ensure_device(size_t bytes) {
        int now = -1;
        WMX_HIP(hipGetDevice(&now));
        if (now != device) drop_device();  // the thread moved to another device: the old buffer is of no use there
        device = now;
        if (bytes <= dmem_cap) return 0;
        drop_device();
        void *p = nullptr;
        WMX_HIP(hipMalloc(&p, bytes));
        dmem = static_cast<uint8_t *>(p);
        dmem_cap = bytes;
        return 0;
    }
};

}  // namespace wmx
