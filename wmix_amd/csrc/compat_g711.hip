// compat_g711.hip -- the reference's G.711 entry points (src/g711codec.h:24-34,
// src/g711codec.c:194-308) exported unchanged over HOST buffers.  Each call stages
// the buffer where the device reads it (legacy_stage.h), runs the batched kernel
// of g711.hip and brings the result back; there is no CPU arithmetic here.  Error behaviour follows the reference:
// the PCM2G711x/G711x2PCM null check only fires when in, out AND len are all
// null/0 (src/g711codec.c:230 uses &&); otherwise the element count (encode) or
// byte count (decode) is returned.  A HIP failure returns -1 and sets
// wmx_last_error().
#include "legacy_stage.h"
#include "../../include/wmix_compat.h"

namespace {

// The daemon converts one RTP payload per call (160 - 320 samples, src/wmixTask.c:285, 1139, 1282): up to kMappedMax elements a call is
// staged in mapped pinned memory, above it through device memory (legacy_stage.h).  Every launch and copy of a call goes to the
// calling THREAD's own non-blocking stream and only that stream is waited for (wmx_internal.h: thread_stream) -- the daemon's RTP
// threads convert side by side.
constexpr size_t kMappedMax = 16384;
thread_local wmx::Stage g_stage;  // region 0: the int16 side, region 1: the codes

int host_encode(int law, unsigned char *out, const short *in, int len) {
    if (len <= 0) return 0;
    const size_t n = (size_t)len;
    hipStream_t s = wmx::thread_stream();
    wmx::Stage &st = g_stage;
    if (st.begin(3 * n, 3 * kMappedMax, {2 * n, n})) return -1;
    bool ok = st.put(0, in, 2 * n, s) == 0 && wmx_g711_encode(law, st.dev<const int16_t>(0), st.dev<uint8_t>(1), n, s) == 0;
    if (ok) st.get(1, out, n);
    return st.finish(s) == 0 && ok ? len : -1;
}

int host_decode(int law, short *out, const unsigned char *in, int bytes) {
    if (bytes <= 0) return 0;
    const size_t n = (size_t)bytes;
    hipStream_t s = wmx::thread_stream();
    wmx::Stage &st = g_stage;
    if (st.begin(3 * n, 3 * kMappedMax, {2 * n, n})) return -1;
    bool ok = st.put(1, in, n, s) == 0 && wmx_g711_decode(law, st.dev<const uint8_t>(1), st.dev<int16_t>(0), n, s) == 0;
    if (ok) st.get(0, out, 2 * n);
    return st.finish(s) == 0 && ok ? bytes * 2 : -1;
}

bool all_null(const void *a, const void *b, int n) { return !a && !b && n == 0; }

}  // namespace

extern "C" {

int g711a_encode(unsigned char g711_data[], const short amp[], int len) { return host_encode(WMX_LAW_A, g711_data, amp, len); }
int g711u_encode(unsigned char g711_data[], const short amp[], int len) { return host_encode(WMX_LAW_U, g711_data, amp, len); }
int g711a_decode(short amp[], const unsigned char d[], int bytes) { return host_decode(WMX_LAW_A, amp, d, bytes); }
int g711u_decode(short amp[], const unsigned char d[], int bytes) { return host_decode(WMX_LAW_U, amp, d, bytes); }

int PCM2G711a(char *in, char *out, int DataLen, int reserve) {
    (void)reserve;
    if (all_null(in, out, DataLen)) {
        printf("Error, empty data or transmit failed, exit !\n");
        return -1;
    }
    return host_encode(WMX_LAW_A, (unsigned char *)out, (const short *)in, DataLen / 2);
}
int PCM2G711u(char *in, char *out, int DataLen, int reserve) {
    (void)reserve;
    if (all_null(in, out, DataLen)) {
        printf("Error, empty data or transmit failed, exit !\n");
        return -1;
    }
    return host_encode(WMX_LAW_U, (unsigned char *)out, (const short *)in, DataLen / 2);
}
int G711a2PCM(char *in, char *out, int DataLen, int reserve) {
    (void)reserve;
    if (all_null(in, out, DataLen)) {
        printf("Error, empty data or transmit failed, exit !\n");
        return -1;
    }
    return host_decode(WMX_LAW_A, (short *)out, (const unsigned char *)in, DataLen);
}
int G711u2PCM(char *in, char *out, int DataLen, int reserve) {
    (void)reserve;
    if (all_null(in, out, DataLen)) {
        printf("Error, empty data or transmit failed, exit !\n");
        return -1;
    }
    return host_decode(WMX_LAW_U, (short *)out, (const unsigned char *)in, DataLen);
}

// src/g711codec.c:82,120 export these although the header does not declare them.
unsigned char linear2alaw(int pcm_val) {
    short s = (short)pcm_val;
    unsigned char c = 0;
    host_encode(WMX_LAW_A, &c, &s, 1);
    return c;
}
unsigned char linear2ulaw(int pcm_val) {
    short s = (short)pcm_val;
    unsigned char c = 0;
    host_encode(WMX_LAW_U, &c, &s, 1);
    return c;
}

}  // extern "C"
