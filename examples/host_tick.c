/* host_tick.c -- a C host of the daemon's whole tick for many mixers side by side: plain C99, the library's C ABI (wmx_tick_*) and the
 * HIP runtime API for the buffers, nothing else.
 *
 * What ONE wmix daemon does per WMIX_INTERVAL_MS = 20 ms (src/wmix.c:1347-1440 with wmix_shmem_write_circle, :528-780, inside) --
 *   task threads: wmix_load_data of every source into the play ring          wmx_tick_load
 *   play thread:  drain one package -> playPkgBuff_add -> sound card,        wmx_tick_play   (the group's far-end package is left on
 *                 playPkgBuff_get(AEC_INTERVALMS)                                             the device: wmx_tick_far)
 *   the room:     what the microphones pick up (this harness: local + the far-end delayed by 40 samples, halved -- the model of
 *                 tests/test_tick_gpu.py and oracle/loader.py tick_room), computed HERE on the host
 *   heartbeat:    ns -> aec_process2(far) -> agc -> vad in place, [rwTest: load the recording back], zoom to 1 x 8000
 *                                                                            wmx_tick_record
 * -- for n_groups daemons with n_src sources and n_rec record streams each, in the 1 x 8000 Hz format all three platform
 * directories of the reference ship.
 *
 *   host_tick src.i16 local.i16 out.i16 n_groups n_src n_rec n_ticks src_freq src_chn [--platform alsa|hi3516|t31] [--rwtest] [--bridge P]
 *             [--bridge-sizes a,b,c,...] [--speakers N[,floor[,shift]]] [--bridge-rtp seed]
 *
 * src.i16    int16 [n_ticks][n_groups][n_src][20 ms of (src_freq, src_chn)]   what the task threads play
 * local.i16  int16 [n_ticks][n_groups * n_rec][160]                          the rooms without their loudspeakers
 * out.i16    int16 [n_ticks][ n_groups play | n_groups far | n_groups * n_rec record ][160]
 * --platform: PLAT_AEC_INTERVALMS / PLAT_PLAY_CORRECT of platform/<name>/plat.h (400 ms / 3200 B, 700 / 0, 0 / 0; default alsa)
 * --rwtest:   wmix->rwTest (src/wmix.c:714-732)
 * --bridge P: the groups are n_groups / P conferences of P call legs (n_rec must be 1): every leg's heartbeat output is loaded into the
 *             rings of the other legs of its conference, so each leg is played everybody except itself (wmx_tick_bridge)
 * --bridge-sizes a,b,c,...: conferences of different sizes: the first a groups are conference 0, the next b conference 1, and so on;
 *             the groups that remain are idle legs, in no conference (wmx_tick_bridge_conferences; n_rec must be 1)
 * --speakers N[,floor[,shift]]: with --bridge or --bridge-sizes, only the loudest N legs of a conference are loaded into the others'
 *             rings, chosen on the device from every tick's heartbeat output (wmx_tick_bridge_speakers; floor 0 and shift 3 when not
 *             given); the JSON line then says how many legs were speaking in the last tick
 * --bridge-rtp seed: with --bridge-sizes, the conferences' legs are RTP/G.711 senders whose datagrams come early, late or not at all
 *             (bridge_rtp below): src.i16 and local.i16 are not read, nothing is recorded, and out.i16 receives the datagrams
 *             that go back to the legs, uint8 [n_ticks][n_groups][172]
 * Prints one JSON line.  tests/test_host_chain_gpu.py compares out.i16 with one oracle daemon per group.
 *
 * Build (what __graft_entry__.build() runs):
 *   gcc -std=c99 -O2 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/host_tick.c -o examples/host_tick \
 *       -Lwmix_amd -lwmix_amd -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$ORIGIN/../wmix_amd' -Wl,-rpath,/opt/rocm/lib
 */
#define _POSIX_C_SOURCE 200809L
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "wmix_amd.h"

#define PKG 160        /* int16 of one 20 ms package at 1 x 8000 Hz */
#define ECHO_DELAY 40  /* samples between loudspeaker and microphone in the harness' room */

static void *read_file(const char *path, size_t bytes) {
    FILE *f = fopen(path, "rb");
    void *p = malloc(bytes ? bytes : 1);
    if (!f || !p || fread(p, 1, bytes, f) != bytes) {
        fprintf(stderr, "host_tick: cannot read %zu bytes of %s\n", bytes, path);
        exit(2);
    }
    fclose(f);
    return p;
}

static double now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

#define HIP_OK(call)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            fprintf(stderr, "host_tick: %s: %s\n", #call, hipGetErrorString(e_));            \
            return 3;                                                                        \
        }                                                                                    \
    } while (0)
#define WMX_OK(call)                                                                         \
    do {                                                                                     \
        int rc_ = (call);                                                                    \
        if (rc_ != 0) {                                                                      \
            fprintf(stderr, "host_tick: %s = %d: %s\n", #call, rc_, wmx_last_error());       \
            return 4;                                                                        \
        }                                                                                    \
    } while (0)

/* --bridge-sizes a,b,c: consecutive groups.  The list goes to the library as it stands: what is wrong with it is the library's to say */
static int parse_sizes(const char *sizes, int32_t **off_out, int32_t **members_out) {
    int n_conf = 0;
    int32_t *conf_off = calloc(strlen(sizes) + 2, sizeof(int32_t));
    if (!conf_off) return -1;
    for (const char *p = sizes; *p;) {
        char *end = NULL;
        long v = strtol(p, &end, 10);
        if (end == p || (*end && *end != ',') || v < 0 || v > 1000000) v = -1, end = (char *)p + strcspn(p, ","); /* not a size */
        conf_off[n_conf + 1] = conf_off[n_conf] + (int32_t)v;
        n_conf++;
        p = *end ? end + 1 : end;
    }
    const int32_t total = conf_off[n_conf] > 0 ? conf_off[n_conf] : 0;
    int32_t *conf_members = calloc((size_t)total + 1, sizeof(int32_t));
    if (!conf_members) return -1;
    for (int32_t r = 0; r < total; r++) conf_members[r] = r; /* consecutive groups; one past n_groups - 1 is refused */
    *off_out = conf_off, *members_out = conf_members;
    return n_conf;
}

/* --bridge-rtp: a conference bridge of RTP/G.711 legs.  Every wmix_thread_rtp_recv_pcma keeps a cursor of its own and loads one package
 * per datagram that arrived (src/wmixTask.c:1266-1316), so a leg whose network delivers 0, 2 or 3 datagrams in a tick is a leg whose
 * cursor falls behind or runs ahead.  Per 20 ms tick, for G legs:
 *   the network:  up to RTP_SLOTS datagrams per leg, scripted from the seed (below)       hipMemcpy
 *   receive:      payload size by type, G711a2PCM, a zero row where nothing arrived        wmx_rtp_ingest_legs
 *   mix:          every leg's packages into the rings of the others of its conference,     wmx_mix_load_minus_legs on wmx_tick_mix(h)
 *                 each leg from its own cursor
 *   play thread:  drain one package per leg                                                wmx_tick_play
 *   send:         what a leg is played goes back to it as one RTP/PCMA datagram            wmx_rtp_egress
 * The tick has no stages and nothing is recorded.  The script: one 64-bit LCG; per tick and leg u = next % 8 -- 0, 1: nothing arrives;
 * 2: two datagrams in slots 0 and 1; 3: two in slots 0 and 2, recvfrom said -1 for slot 1; else one in slot 0 -- and per datagram that
 * arrives v = next % 16 (0: payload type 96, not G.711; 1: PCMU; else PCMA), then 160 payload bytes next & 255; seq counts per leg. */
#define RTP_SLOTS 3
#define RTP_BYTES 172
#define RTP_ROW 176   /* datagram rows on 4-byte boundaries */
#define PCM_ROW 164   /* PCM rows on 8-byte boundaries */
static uint64_t lcg_state;
static uint32_t lcg_next(void) {
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(lcg_state >> 33);
}

static int bridge_rtp(const char *out_path, unsigned long seed, int G, int T, int aec_ms, long correct, const char *platform, const char *sizes) {
    int32_t *conf_off = NULL, *conf_members = NULL;
    const int n_conf = parse_sizes(sizes, &conf_off, &conf_members);
    if (n_conf < 0) return 2;
    wmx_tick *h = NULL;
    wmx_rtp *snd = NULL;
    WMX_OK(wmx_tick_create(&h, G, 1, 1, 8000, 20, aec_ms, 5, 0));
    if (correct >= 0) WMX_OK(wmx_tick_set_play_correct(h, (uint32_t)correct));
    WMX_OK(wmx_tick_bridge_conferences(h, n_conf, conf_off, conf_members, NULL));
    WMX_OK(wmx_rtp_create(&snd, G, WMX_LAW_A));
    if (wmx_tick_package_samples(h) != PKG) return 5;
    const size_t in_bytes = (size_t)G * RTP_SLOTS * RTP_ROW;
    uint8_t *in = calloc(in_bytes, 1), *out = calloc((size_t)T * G * RTP_BYTES, 1);
    int32_t *recv = calloc((size_t)G * RTP_SLOTS, sizeof(int32_t));
    uint16_t *seq = calloc((size_t)G, sizeof(uint16_t));
    if (!in || !out || !recv || !seq) return 2;
    uint8_t *d_in = NULL, *d_out = NULL;
    int32_t *d_recv = NULL;
    uint32_t *d_len = NULL;
    int16_t *d_pcm = NULL, *d_play = NULL;
    HIP_OK(hipMalloc((void **)&d_in, in_bytes));
    HIP_OK(hipMalloc((void **)&d_out, (size_t)G * RTP_BYTES));
    HIP_OK(hipMalloc((void **)&d_recv, (size_t)G * RTP_SLOTS * sizeof(int32_t)));
    HIP_OK(hipMalloc((void **)&d_len, (size_t)G * RTP_SLOTS * sizeof(uint32_t)));
    HIP_OK(hipMalloc((void **)&d_pcm, (size_t)G * RTP_SLOTS * PCM_ROW * 2));
    HIP_OK(hipMalloc((void **)&d_play, (size_t)G * PKG * 2));
    HIP_OK(hipMemset(d_pcm, 0, (size_t)G * RTP_SLOTS * PCM_ROW * 2));
    lcg_state = seed;
    long arrived = 0;
    const double t0 = now_ms();
    for (int t = 0; t < T; t++) {
        /* the network */
        memset(in, 0xEE, in_bytes);
        for (int g = 0; g < G; g++) {
            const uint32_t u = lcg_next() % 8;
            int32_t *rv = recv + (size_t)g * RTP_SLOTS;
            rv[0] = u >= 2 ? RTP_BYTES : 0;
            rv[1] = u == 2 ? RTP_BYTES : (u == 3 ? -1 : 0);
            rv[2] = u == 3 ? RTP_BYTES : 0;
            for (int k = 0; k < RTP_SLOTS; k++) {
                if (rv[k] <= 0) continue;
                uint8_t *pk = in + ((size_t)g * RTP_SLOTS + k) * RTP_ROW;
                const uint32_t v = lcg_next() % 16;
                memset(pk, 0, 12);
                pk[0] = 2u << 6;
                pk[1] = (uint8_t)(0x80 | (v == 0 ? 96 : (v == 1 ? 0 : 8)));
                pk[2] = (uint8_t)(seq[g] >> 8), pk[3] = (uint8_t)seq[g];
                seq[g]++;
                for (int i = 0; i < 160; i++) pk[12 + i] = (uint8_t)(lcg_next() & 255);
                arrived++;
            }
        }
        HIP_OK(hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_recv, recv, (size_t)G * RTP_SLOTS * sizeof(int32_t), hipMemcpyHostToDevice));
        /* receive, mix, play, send */
        WMX_OK(wmx_rtp_ingest_legs(G, RTP_SLOTS, d_in, RTP_SLOTS * RTP_ROW, RTP_ROW, d_recv, d_pcm, RTP_SLOTS * PCM_ROW, PCM_ROW, d_len, NULL, NULL));
        WMX_OK(wmx_mix_load_minus_legs(wmx_tick_mix(h), d_pcm, PKG * 2, 8000, 1, 16, RTP_SLOTS * PCM_ROW, PCM_ROW, RTP_SLOTS, d_len, NULL, 1, NULL));
        WMX_OK(wmx_tick_play(h, d_play, PKG, NULL));
        uint32_t bytes = 0;
        WMX_OK(wmx_rtp_egress(snd, 1, 8000, d_play, PKG * 2, PKG, 1, 8000, d_out, RTP_BYTES, &bytes, NULL));
        if (bytes != RTP_BYTES) return 6;
        HIP_OK(hipMemcpy(out + (size_t)t * G * RTP_BYTES, d_out, (size_t)G * RTP_BYTES, hipMemcpyDeviceToHost));
    }
    const double wall = now_ms() - t0;
    uint32_t *dropped = calloc((size_t)G, sizeof(uint32_t));
    if (!dropped) return 2;
    WMX_OK(wmx_mix_export_leg_cursors(wmx_tick_mix(h), NULL, NULL, dropped, NULL));
    unsigned long n_dropped = 0;
    for (int g = 0; g < G; g++) n_dropped += dropped[g];
    uint64_t sum = 1469598103934665603ull; /* FNV-1a over the datagrams that went out */
    for (size_t i = 0; i < (size_t)T * G * RTP_BYTES; i++) sum = (sum ^ out[i]) * 1099511628211ull;
    wmx_rtp_destroy(snd);
    wmx_tick_destroy(h);
    FILE *f = fopen(out_path, "wb");
    int rc = (!f || fwrite(out, 1, (size_t)T * G * RTP_BYTES, f) != (size_t)T * G * RTP_BYTES) ? 7 : 0;
    if (f) fclose(f);
    printf("{\"groups\": %d, \"ticks\": %d, \"platform\": \"%s\", \"bridge_rtp_seed\": %lu, \"bridge_sizes\": [", G, T, platform, seed);
    for (int c = 0; c < n_conf; c++) printf("%s%d", c ? ", " : "", (int)(conf_off[c + 1] - conf_off[c]));
    printf("], \"datagrams_in\": %ld, \"dropped\": %lu, \"datagrams_fnv1a\": \"%016llx\", \"wall_ms\": %.3f, \"ms_per_tick\": %.4f, \"rc\": %d}\n",
           arrived, n_dropped, (unsigned long long)sum, wall, wall / T, rc);
    return rc;
}

int main(int argc, char **argv) {
    if (argc < 10) {
        fprintf(stderr, "usage: %s src.i16 local.i16 out.i16 n_groups n_src n_rec n_ticks src_freq src_chn [--platform name] [--rwtest] [--bridge P] [--bridge-sizes a,b,..] [--speakers N[,floor[,shift]]] [--bridge-rtp seed]\n", argv[0]);
        return 2;
    }
    const int G = atoi(argv[4]), n_src = atoi(argv[5]), R = atoi(argv[6]), T = atoi(argv[7]), sfreq = atoi(argv[8]), schn = atoi(argv[9]);
    int aec_ms = 400, rwtest = 0, bridge = 0;
    const char *bridge_sizes = NULL, *speakers = NULL, *rtp_seed = NULL;
    long correct = -1; /* -1: the library's default = platform/alsa */
    const char *platform = "alsa";
    for (int i = 10; i < argc; i++) {
        if (!strcmp(argv[i], "--rwtest")) {
            rwtest = 1;
        } else if (!strcmp(argv[i], "--bridge") && i + 1 < argc) {
            bridge = atoi(argv[++i]);
        } else if (!strcmp(argv[i], "--bridge-sizes") && i + 1 < argc) {
            bridge_sizes = argv[++i];
        } else if (!strcmp(argv[i], "--speakers") && i + 1 < argc) {
            speakers = argv[++i];
        } else if (!strcmp(argv[i], "--bridge-rtp") && i + 1 < argc) {
            rtp_seed = argv[++i];
        } else if (!strcmp(argv[i], "--platform") && i + 1 < argc) {
            platform = argv[++i];
            if (!strcmp(platform, "alsa")) {
                aec_ms = 400, correct = 3200;
            } else if (!strcmp(platform, "hi3516")) {
                aec_ms = 700, correct = 0;
            } else if (!strcmp(platform, "t31")) {
                aec_ms = 0, correct = 0;
            } else {
                fprintf(stderr, "host_tick: no platform directory '%s' in the reference\n", platform);
                return 2;
            }
        } else {
            fprintf(stderr, "host_tick: what is '%s'?\n", argv[i]);
            return 2;
        }
    }
    if (G < 1 || n_src < 1 || R < 1 || T < 1 || sfreq < 1000 || (schn != 1 && schn != 2)) return 2;
    if (rtp_seed) {
        if (!bridge_sizes || bridge || rwtest || speakers || R != 1) {
            fprintf(stderr, "host_tick: --bridge-rtp goes with --bridge-sizes and n_rec 1, and with none of --bridge, --rwtest, --speakers\n");
            return 2;
        }
        return bridge_rtp(argv[3], strtoul(rtp_seed, NULL, 10), G, T, aec_ms, correct, platform, bridge_sizes);
    }
    const size_t per = (size_t)sfreq / 1000 * 20 * schn;  /* int16 of one source's 20 ms */
    const size_t srow = per + 2 * (size_t)schn;            /* + the frame the up-sampling fill looks ahead to (src/wmix.c:1857) */
    const size_t S = (size_t)G * R;
    int16_t *src = read_file(argv[1], (size_t)T * G * n_src * per * 2);
    int16_t *local = read_file(argv[2], (size_t)T * S * PKG * 2);
    const size_t out_row = ((size_t)2 * G + S) * PKG;
    int16_t *out = calloc((size_t)T * out_row, 2);
    int16_t *farline = calloc((size_t)2 * G * PKG, 2); /* per group: the previous far-end package, then this one */
    int16_t *near = malloc(S * PKG * 2), *pad = calloc((size_t)G * n_src * srow, 2);
    if (!out || !farline || !near || !pad) return 2;

    wmx_tick *h = NULL;
    WMX_OK(wmx_tick_create(&h, G, R, 1, 8000, 20, aec_ms, 5, WMX_CHAIN_NS | WMX_CHAIN_AEC | WMX_CHAIN_AGC | WMX_CHAIN_VAD));
    if (correct >= 0) WMX_OK(wmx_tick_set_play_correct(h, (uint32_t)correct));
    if (rwtest) WMX_OK(wmx_tick_rw_test(h, 1));
    if (bridge) WMX_OK(wmx_tick_bridge(h, bridge));
    int n_conf = 0;
    int32_t *conf_off = NULL, *conf_members = NULL;
    if (bridge_sizes) {
        if ((n_conf = parse_sizes(bridge_sizes, &conf_off, &conf_members)) < 0) return 2;
        WMX_OK(wmx_tick_bridge_conferences(h, n_conf, conf_off, conf_members, NULL));
    }
    int spk_max = 0, spk_shift = 3;
    unsigned spk_floor = 0;
    if (speakers) { /* what is wrong with the numbers is the library's to say; what is not a number is not passed on */
        if (!bridge && !bridge_sizes) {
            fprintf(stderr, "host_tick: --speakers needs --bridge or --bridge-sizes\n");
            return 2;
        }
        int used = 0;
        const int got = sscanf(speakers, "%d%n,%u%n,%d%n", &spk_max, &used, &spk_floor, &used, &spk_shift, &used);
        if (got < 1 || speakers[used] != '\0') {
            fprintf(stderr, "host_tick: --speakers N[,floor[,shift]], not '%s'\n", speakers);
            return 2;
        }
        WMX_OK(wmx_tick_bridge_speakers(h, spk_max, spk_floor, spk_shift));
    }
    if (wmx_tick_package_samples(h) != PKG) return 5;
    int16_t *d_src = NULL, *d_play = NULL, *d_rec = NULL, *d_zoom = NULL;
    HIP_OK(hipMalloc((void **)&d_src, (size_t)G * n_src * srow * 2));
    HIP_OK(hipMalloc((void **)&d_play, (size_t)G * PKG * 2));
    HIP_OK(hipMalloc((void **)&d_rec, S * PKG * 2));
    HIP_OK(hipMalloc((void **)&d_zoom, S * PKG * 2));
    uint32_t head = UINT32_MAX, tick = 0; /* the sources' common cursor: NULL head = first call, like a task thread that just started */
    const double t0 = now_ms();
    for (int t = 0; t < T; t++) {
        int16_t *o = out + (size_t)t * out_row;
        /* the task threads */
        for (size_t r = 0; r < (size_t)G * n_src; r++) memcpy(pad + r * srow, src + ((size_t)t * G * n_src + r) * per, per * 2);
        HIP_OK(hipMemcpy(d_src, pad, (size_t)G * n_src * srow * 2, hipMemcpyHostToDevice));
        WMX_OK(wmx_tick_load(h, d_src, (uint32_t)(per * 2), sfreq, schn, 16, n_src, (long)(n_src * srow), (long)srow, 1, &head, &tick, NULL));
        /* the play thread */
        WMX_OK(wmx_tick_play(h, d_play, PKG, NULL));
        HIP_OK(hipMemcpy(o, d_play, (size_t)G * PKG * 2, hipMemcpyDeviceToHost));
        for (int g = 0; g < G; g++) memcpy(farline + (size_t)g * 2 * PKG, farline + (size_t)g * 2 * PKG + PKG, PKG * 2);
        HIP_OK(hipMemcpy2D(farline + PKG, 2 * PKG * 2, wmx_tick_far(h), PKG * 2, PKG * 2, (size_t)G, hipMemcpyDeviceToHost));
        for (int g = 0; g < G; g++) memcpy(o + ((size_t)G + g) * PKG, farline + (size_t)g * 2 * PKG + PKG, PKG * 2);
        /* the rooms */
        for (size_t s = 0; s < S; s++) {
            const int16_t *line = farline + (s / R) * 2 * PKG, *loc = local + ((size_t)t * S + s) * PKG;
            for (int i = 0; i < PKG; i++) {
                int v = loc[i] + (line[PKG + i - ECHO_DELAY] >> 1);
                near[s * PKG + i] = (int16_t)(v > 32767 ? 32767 : (v < -32768 ? -32768 : v));
            }
        }
        /* the heartbeats */
        HIP_OK(hipMemcpy(d_rec, near, S * PKG * 2, hipMemcpyHostToDevice));
        uint32_t zoomed = 0;
        WMX_OK(wmx_tick_record(h, d_rec, PKG, d_zoom, PKG, PKG * 2, &zoomed, NULL));
        if (zoomed != PKG * 2) return 6;
        HIP_OK(hipMemcpy(o + (size_t)2 * G * PKG, d_rec, S * PKG * 2, hipMemcpyDeviceToHost));
    }
    const double wall = now_ms() - t0;
    int speaking_legs = 0;
    if (spk_max) { /* who was loaded in the last tick */
        uint8_t *speaking = calloc((size_t)G, 1);
        if (!speaking) return 2;
        WMX_OK(wmx_tick_bridge_speaking(h, speaking, NULL, NULL));
        for (int g = 0; g < G; g++) speaking_legs += speaking[g] != 0;
        free(speaking);
    }
    wmx_tick_destroy(h);
    FILE *f = fopen(argv[3], "wb");
    int rc = (!f || fwrite(out, 2, (size_t)T * out_row, f) != (size_t)T * out_row) ? 7 : 0;
    if (f) fclose(f);
    printf("{\"groups\": %d, \"sources\": %d, \"record_streams\": %d, \"ticks\": %d, \"platform\": \"%s\", \"aec_delay_ms\": %d, \"rw_test\": %d, ", G,
           n_src, R, T, platform, aec_ms, rwtest);
    if (bridge) printf("\"bridge_parties\": %d, ", bridge);
    if (bridge_sizes) {
        printf("\"bridge_sizes\": [");
        for (int c = 0; c < n_conf; c++) printf("%s%d", c ? ", " : "", (int)(conf_off[c + 1] - conf_off[c]));
        printf("], ");
    }
    if (speakers) printf("\"speakers\": %d, \"speakers_floor\": %u, \"speakers_shift\": %d, \"speaking\": %d, ", spk_max, spk_floor, spk_shift, speaking_legs);
    printf("\"wall_ms\": %.3f, \"ms_per_tick\": %.4f, \"rc\": %d}\n", wall, wall / T, rc);
    return rc;
}
