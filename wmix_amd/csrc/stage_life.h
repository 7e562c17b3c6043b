// stage_life.h -- per-stream lifetime and migration of a batched stage (ns, nsx, aec, aecm, agc, vad): the parts, and ONE copy of the
// procedure around them.  A stage's handle has `device`, `n_streams` and a StreamLife `life`; it says once what a stream's blob holds
// (a StreamBlob: tag, layout word, version, the state arrays), launches its own refill kernels, and its wmx_<m>_set_active /
// _reset_streams / _stream_state_bytes / _export_stream / _import_stream entry points are calls of the templates below.
#pragma once
#include <cstring>
#include "wmx_internal.h"

namespace wmx {

// Per-stream lifetime inside a batch.  The reference creates every handle lazily, releases it when its flag drops or recording
// idles and creates a new one later (src/wmix.c:565-600, 617-618, 635-636, 683-684, 702-703, 783-813): streams of a batch join,
// leave and restart on their own.  Two device-side facilities serve that without a new batch:
//   * an ACTIVE mask [n_streams] (1 = the stream is processed; 0 = its state, and its PCM rows, are left alone, like a handle
//     nobody calls); nullptr = every stream is active;
//   * RESET of a list of streams to the state *_init gives (release + init), by a refill kernel of the module.
// The index list of a reset is staged in a device buffer that is rewritten only after the kernel that read it last has
// finished (an event, like the AEC plan slots).
struct StreamLife {
    uint8_t *d_active = nullptr;
    int32_t *d_idx = nullptr;
    size_t idx_cap = 0;
    hipEvent_t idx_free = nullptr;
    bool idx_used = false;
    StreamLife() = default;
    StreamLife(const StreamLife &) = delete;
    StreamLife &operator=(const StreamLife &) = delete;
    // host_mask: n_streams bytes, or nullptr for "all active" (the mask is dropped)
    int set_active(int n_streams, const uint8_t *host_mask, hipStream_t s) {
        if (!host_mask) {
            if (d_active) {
                // kernels in flight still read it, on `s` or on any other stream the caller ran this handle on: the whole
                // device is drained before the mask goes (a control-plane call, rare)
                (void)s;
                WMX_HIP(hipDeviceSynchronize());
                (void)hipFree(d_active);
                d_active = nullptr;
            }
            return 0;
        }
        if (!d_active) WMX_HIP(hipMalloc(reinterpret_cast<void **>(&d_active), (size_t)n_streams));
        WMX_HIP(hipMemcpyAsync(d_active, host_mask, (size_t)n_streams, hipMemcpyHostToDevice, s));
        return 0;
    }
    // validates and uploads a reset list; *d_out = device copy, valid for kernels launched on `s` before done(s)
    int upload(const int32_t *idx, int n, int n_streams, hipStream_t s, const int32_t **d_out) {
        for (int i = 0; i < n; i++)
            if (idx[i] < 0 || idx[i] >= n_streams) {
                set_error("reset_streams: index %d of the list is stream %d of %d", i, idx[i], n_streams);
                return WMX_EINVAL;
            }
        if (idx_used) WMX_HIP(hipEventSynchronize(idx_free));
        if ((size_t)n > idx_cap) {
            if (d_idx) (void)hipFree(d_idx);
            d_idx = nullptr;
            idx_cap = 0;
            const size_t cap = (size_t)n < 256 ? 256 : (size_t)n;
            WMX_HIP(hipMalloc(reinterpret_cast<void **>(&d_idx), cap * sizeof(int32_t)));
            idx_cap = cap;
        }
        if (!idx_free) WMX_HIP(hipEventCreateWithFlags(&idx_free, hipEventDisableTiming));
        WMX_HIP(hipMemcpyAsync(d_idx, idx, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        *d_out = d_idx;
        return 0;
    }
    int done(hipStream_t s) {
        WMX_HIP(hipEventRecord(idx_free, s));
        idx_used = true;
        return 0;
    }
    void release() {
        if (d_active) (void)hipFree(d_active);
        if (d_idx) (void)hipFree(d_idx);
        if (idx_free) (void)hipEventDestroy(idx_free);
        d_active = nullptr;
        d_idx = nullptr;
        idx_free = nullptr;
        idx_cap = 0;
        idx_used = false;
    }
};

// The entry points' bodies (static: instantiated in the stage's translation unit, no symbol of the library).
// wmx_<m>_set_active
template <class H>
static int set_active(H *h, const uint8_t *host_mask, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    return h->life.set_active(h->n_streams, host_mask, as_stream(stream));
}

// wmx_<m>_reset_streams (and the AGC's calls on a list of streams): the list is checked and uploaded, then the module's part,
//     int refill(hipStream_t s, const int32_t *d_idx)     its launches on `s` and their WMX_LAUNCH_CHECK; may refuse before it launches
// and the list's buffer is released behind them.  `refused`: the verdict on the module's OWN arguments (0, or the code to return),
// worked out by the caller without touching anything; it takes its place behind the common argument check.
template <class H, class Refill>
static int reset_streams(H *h, const int32_t *idx, int n, void *stream, Refill refill, int refused = 0) {
    WMX_ON_DEVICE(h);
    if (!h || n < 0 || (n > 0 && !idx)) return WMX_EINVAL;
    if (refused != 0) return refused;
    if (n == 0) return 0;
    hipStream_t s = as_stream(stream);
    const int32_t *d_idx = nullptr;
    int rc = h->life.upload(idx, n, h->n_streams, s, &d_idx);  // validates the list
    if (rc == 0) rc = refill(s, d_idx);
    return rc != 0 ? rc : h->life.done(s);
}

// Stream migration (wmx_<m>_export_stream / _import_stream): a stream's complete state as a self-describing host blob --
// a header that names the module and its layout, then the bytes.  Blocking calls (a control-plane operation): the device is
// drained first, so the blob is the state after every call made so far.
struct BlobHeader {
    uint32_t magic;    // 'WMXS'
    uint32_t module;   // four characters
    uint32_t layout;   // module-defined: sizes that must agree between exporter and importer (e.g. words per stream, rate)
    uint32_t bytes;    // payload bytes behind the header
};
constexpr uint32_t kBlobMagic = 0x53584d57u;
// The FORMAT VERSION of a module's blob rides in the top byte of `layout` (rates and word counts stay far below 2^24).  A module bumps
// its version whenever the MEANING of a state word changes, even if tag, layout and size do not: round 5 turned the AEC's block count
// (AS_NBLK) into the comfort-noise generator's state (AS_NSEED) in place, and a blob exported by the build before would have been
// accepted and replayed with the old block count as the seed (round-5 ADVICE, medium).  Blobs of rounds 1-5 carry version 0 and are
// refused with WMX_ESTATE.
inline uint32_t blob_layout(uint32_t layout, uint32_t version) { return (layout & 0x00ffffffu) | (version << 24); }
inline uint32_t blob_tag(const char (&t)[5]) { return (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24); }
inline void blob_begin(void *blob, uint32_t module, uint32_t layout, uint32_t bytes) {
    BlobHeader hd{kBlobMagic, module, layout, bytes};
    memcpy(blob, &hd, sizeof(hd));
}
// 0, or WMX_ESTATE when the blob was made by another module / layout
inline int blob_check(const void *blob, uint32_t module, uint32_t layout, uint32_t bytes) {
    BlobHeader hd;
    memcpy(&hd, blob, sizeof(hd));
    if (hd.magic != kBlobMagic || hd.module != module || hd.layout != layout || hd.bytes != bytes) {
        if (hd.magic == kBlobMagic && hd.module == module && (hd.layout >> 24) != (layout >> 24))
            set_error("import: the blob is format version %u of this module, this library reads version %u (the meaning of a state word "
                      "changed in between: re-export from a stream of this build)", hd.layout >> 24, layout >> 24);
        else
            set_error("import: the blob is not a state of this module / format (module %08x layout %u bytes %u, expected %08x %u %u)", hd.module,
                      hd.layout & 0x00ffffffu, hd.bytes, module, layout & 0x00ffffffu, bytes);
        return WMX_ESTATE;
    }
    return 0;
}

// What a stream's blob holds behind the header, said ONCE per module (a function of the handle that returns a StreamBlob): the state
// arrays in the blob's order, then `tail` bytes that are not an array's and that the module's hooks write and read (the AGC's gain).
struct Plane {
    void *dev = nullptr;       // the device array, all streams
    size_t elem = 0;           // bytes per element
    size_t count = 0;          // elements per stream (0: no such plane)
    bool field_major = false;  // [field][n_streams] (AGC, VAD) instead of [stream][count]
    size_t bytes() const { return elem * count; }
    // one stream's part to / from a packed host array (field-major: a column, `count` rows of one element)
    char *at(int stream) const { return static_cast<char *>(dev) + (size_t)stream * (field_major ? elem : bytes()); }
    hipError_t to_host(char *host, int n_streams, int stream) const {
        if (!field_major) return hipMemcpy(host, at(stream), bytes(), hipMemcpyDeviceToHost);
        return hipMemcpy2D(host, elem, at(stream), (size_t)n_streams * elem, elem, count, hipMemcpyDeviceToHost);
    }
    hipError_t from_host(const char *host, int n_streams, int stream) const {
        if (!field_major) return hipMemcpy(at(stream), host, bytes(), hipMemcpyHostToDevice);
        return hipMemcpy2D(at(stream), (size_t)n_streams * elem, host, elem, elem, count, hipMemcpyHostToDevice);
    }
};
struct StreamBlob {
    uint32_t tag, layout;  // blob_tag(...), blob_layout(layout, version)
    Plane plane[2];
    size_t tail;
    size_t plane_bytes() const { return plane[0].bytes() + plane[1].bytes(); }
    uint32_t bytes() const { return (uint32_t)(plane_bytes() + tail); }
};
struct NoHook {
    int operator()(const char *) const { return 0; }
};

template <class H, class Describe>
static int stream_state_bytes(const H *h, Describe describe) {
    return h ? (int)(sizeof(BlobHeader) + describe(h).bytes()) : WMX_EINVAL;
}

// int tail(char *p): writes the blob's tail at p
template <class H, class Describe, class Tail = NoHook>
static int export_stream(H *h, int stream_index, void *host_blob, Describe describe, Tail tail = {}) {
    WMX_ON_DEVICE(h);
    if (!h || !host_blob || stream_index < 0 || stream_index >= h->n_streams) return WMX_EINVAL;
    WMX_HIP(hipDeviceSynchronize());
    const StreamBlob b = describe(h);
    char *p = static_cast<char *>(host_blob);
    blob_begin(p, b.tag, b.layout, b.bytes());
    p += sizeof(BlobHeader);
    for (const Plane &pl : b.plane)
        if (pl.count) {
            WMX_HIP(pl.to_host(p, h->n_streams, stream_index));
            p += pl.bytes();
        }
    return tail(p);
}

// args_ok: the module's own arguments are in range (worked out by the caller without touching anything).  The hooks see the blob's
// tail: before(p) may still refuse -- nothing has been written then; after(p) does what follows the state (cohort membership).
template <class H, class Describe, class Before = NoHook, class After = NoHook>
static int import_stream(H *h, int stream_index, const void *host_blob, Describe describe, bool args_ok = true, Before before = {}, After after = {}) {
    WMX_ON_DEVICE(h);
    if (!h || !host_blob || stream_index < 0 || stream_index >= h->n_streams || !args_ok) return WMX_EINVAL;
    const StreamBlob b = describe(h);
    int rc = blob_check(host_blob, b.tag, b.layout, b.bytes());
    if (rc) return rc;
    WMX_HIP(hipDeviceSynchronize());
    const char *p = static_cast<const char *>(host_blob) + sizeof(BlobHeader), *tail = p + b.plane_bytes();
    if ((rc = before(tail)) != 0) return rc;
    for (const Plane &pl : b.plane)
        if (pl.count) {
            WMX_HIP(pl.from_host(p, h->n_streams, stream_index));
            p += pl.bytes();
        }
    return after(tail);
}

}  // namespace wmx

// In wmx_<m>_create, behind `new`: a runtime call that must succeed -- or the half-made handle goes (`cleanup`, the module's destroy)
// and the caller gets the error
#define WMX_CREATE_TRY(cleanup, x)                                       \
    do {                                                                 \
        const hipError_t _e = (x);                                       \
        if (_e != hipSuccess) {                                          \
            const int _rc = wmx::hip_fail(_e, #x, __FILE__, __LINE__);   \
            cleanup;                                                     \
            return _rc;                                                  \
        }                                                                \
    } while (0)
