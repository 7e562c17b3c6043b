/* host_conf.c -- a conference bridge of RTP/G.711 legs from plain C: the library's C ABI alone (wmx_conf_*), not even the HIP runtime API.
 *
 *   host_conf out.rtp n_legs n_ticks --sizes a,b,c --seed S [--slots K] [--speakers N[,floor[,shift]]] [--platform alsa|hi3516|t31]
 *             [--sequence G] [--conceal] [--audio-only] [--ulaw-every N] [--dtmf] [--denoise] [--level V] [--gate] [--echo D]
 *             [--prompt LEN,EVERY[,REPEAT[,GAP[,REDUCE]]]] [--record LEG[,CHN,FREQ[,SECONDS]]]... [--record-dir DIR]
 *
 * What the daemon runs as one receive thread and one send thread per leg plus the play thread (src/wmixTask.c:1266-1316, 1058-1143;
 * src/wmix.c:1347-1366), for n_legs legs per 20 ms tick: the host writes the datagrams that arrived into a slot's pinned rows, submits
 * the slot, and reads the datagrams to send from the slot's out rows once it has left the device.  The rows of tick t + 1 are written
 * while tick t is in flight (K slots, default 3; a slot is waited for only when its turn comes again).
 * --sizes a,b,c: conferences of a, b, c consecutive legs; legs behind them are in no conference.  --speakers: talker selection.
 * The network is the script of host_tick --bridge-rtp: one 64-bit LCG; per tick and leg u = next % 8 -- 0, 1: nothing arrives; 2: two
 * datagrams in slots 0 and 1; 3: two in slots 0 and 2, recvfrom said -1 for slot 1; else one in slot 0 -- and per datagram that arrives
 * v = next % 16 (0: payload type 96, not G.711; 1: PCMU; else PCMA), then 160 payload bytes next & 255; seq counts per leg.
 * --sequence G: the legs are reordered, de-duplicated and gap-filled by RTP sequence number (wmx_conf_sequence, gaps of up to G packets
 * become silence) and the JSON line also carries the five counters summed over the legs.  --audio-only: every datagram of the script is
 * PCMA (v == 0 too), so the script has no gap of its own: a datagram of payload type 96 consumes a sequence number and brings no audio,
 * which sequencing treats as a lost packet.
 * --conceal (only meaningful with --sequence G): the silence of a gap is synthesised from the leg's own history (wmx_conf_conceal) and
 * the JSON line also carries the packets concealed, summed over the legs.
 * --ulaw-every N: every N-th leg (N - 1, 2 N - 1, ...) negotiated PCMU: its G.711 datagrams carry payload type 0, it is decoded as
 * mu-law and answered in mu-law (wmx_conf_set_codecs: WMX_CODEC_PCMU, WMX_LAW_U); the other legs stay at the default.  The JSON line
 * then also carries the number of such legs and the refused counters summed over the legs (wmx_conf_export_codecs).
 * --dtmf: the handle listens to every leg's keypad with suppression on (wmx_conf_dtmf, event payload type 101); leg 0 presses `5` in
 * band for 100 ms and leg 1 sends `#` as RFC 4733 packets (ticks 5 .. 9), and the JSON line also carries the keys read back
 * (wmx_conf_export_dtmf): per report the leg, the key and whether it came from a packet.
 * --denoise: every leg's rows go through the leg's own fixed-point noise suppressor in front of talker selection and the mix
 * (wmx_conf_denoise); the JSON line then carries "denoise": 1.  It combines with every other flag.
 * --level V: every leg's rows go through the leg's own AGC with compression gain V dB, behind the suppressor and in front of talker
 * selection and the mix (wmx_conf_level); the JSON line then carries "level": V.  It combines with every other flag.
 * --gate: every leg's rows go through the leg's own voice-activity gate, behind the AGC and in front of talker selection and the mix
 * (wmx_conf_gate): a row is shifted right by the leg's `reduce`, which starts at 4 -- a call is heard in full from its fifth row; the JSON
 * line then carries "gate": 1 and the rows judged voice and not, summed over the legs ("voiced", "unvoiced": wmx_conf_export_gate).  It
 * combines with every other flag.
 * --echo D: every leg's rows go through the leg's own echo canceller between the suppressor and the AGC, with what the bridge sent to
 * that leg as the far end and D ms (0 .. 500) as every leg's reported delay (wmx_conf_echo); the JSON line then carries "echo": D and the
 * legs whose canceller has left its start-up ("echo_running": wmx_conf_export_echo).  It combines with every other flag.
 * --prompt LEN,EVERY[,REPEAT[,GAP[,REDUCE]]]: an announcement.  The handle gets a prompt store (wmx_conf_prompts) with one clip of LEN samples of
 * 1 x 8000 -- sample i is (next & 16383) - 8192 of a second LCG of the same kind, seeded with S + 1, so the network's script is the one
 * without the flag -- and at tick 0 every EVERY-th leg (EVERY - 1, 2 EVERY - 1, ...) starts playing it (wmx_conf_play): REPEAT passes
 * (default 1; 0: until the run ends) with GAP ticks of pause between two (default 0).  Each of those legs hears the clip on top of its
 * conference, or alone if it is in none.  The JSON line then carries "prompt": LEN, the legs playing ("prompt_legs") and the prompts that
 * ran to their end, summed over the legs ("prompt_done": wmx_conf_export_prompts).  With the fifth field the play is
 * wmx_conf_play_duck(..., REDUCE): while the clip makes calls the rest of the conference reaches the leg divided by REDUCE + 1 (0 .. 15,
 * the reference's `reduce`), and the JSON line also carries "prompt_reduce": REDUCE and the legs whose next tick would be ducked
 * ("prompt_ducking": wmx_conf_export_duck); four fields run what they ran before.  It combines with every other flag.
 * --record LEG[,CHN,FREQ[,SECONDS]] (may be repeated) and --record-dir DIR (default "."): what leg LEG HEARS -- its conference without
 * itself, its prompt on top; a leg that sits in a conference muted and unfed is the recorder of the whole conference -- is written to
 * DIR/leg<LEG>.wav as PCM of CHN x FREQ (default 1 x 8000; one format per handle, so every --record names the same), for SECONDS
 * seconds, 50 rows each (default 0: until the run ends).  The handle gets a store of as many taps as there are --record
 * (wmx_conf_recorders) and every listed leg starts at tick 0 (wmx_conf_record); the rows come back in the slot, beside the datagrams
 * (wmx_conf_rec, wmx_conf_rec_legs).  The file is the canonical 44-byte header and the rows as they come; the two lengths of the header
 * are patched in when the tap has written its last row.  The JSON line then carries "record_taps" and the rows written ("record_rows").
 * out.rtp receives n_ticks x n_legs datagrams of 172 bytes; one JSON line goes to stdout. */
#define _POSIX_C_SOURCE 200809L
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "wmix_amd.h"
#include "wmix_compat.h" /* linear2alaw / linear2ulaw for the key pressed in band */

#define RTP_SLOTS 3
#define RTP_BYTES 172

#define WMX_OK(call)                                                                         \
    do {                                                                                     \
        int rc_ = (call);                                                                    \
        if (rc_ != 0) {                                                                      \
            fprintf(stderr, "host_conf: %s = %d: %s\n", #call, rc_, wmx_last_error());       \
            return 4;                                                                        \
        }                                                                                    \
    } while (0)

static double now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

static uint64_t lcg_state;
static uint32_t lcg_next(void) {
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(lcg_state >> 33);
}

/* --record: one PCM WAV per tap.  The canonical header: RIFF <36 + data> WAVE fmt <16> PCM chn freq <bytes per second> <bytes per frame>
 * <16 bits> data <data>, little endian; written with both lengths 0 and patched when the tap ends */
#define MAX_RECORDS 64
struct recording {
    int leg, seconds;
    FILE *f;
    unsigned long rows, bytes;
};
static void put_le(uint8_t *p, uint32_t v, int n) {
    for (int i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8 * i));
}
static int wav_begin(FILE *f, int chn, int freq) {
    uint8_t hd[44];
    memcpy(hd, "RIFF\0\0\0\0WAVEfmt ", 16);
    put_le(hd + 16, 16, 4), put_le(hd + 20, 1, 2), put_le(hd + 22, (uint32_t)chn, 2), put_le(hd + 24, (uint32_t)freq, 4);
    put_le(hd + 28, (uint32_t)freq * (uint32_t)chn * 2u, 4), put_le(hd + 32, (uint32_t)chn * 2u, 2), put_le(hd + 34, 16, 2);
    memcpy(hd + 36, "data\0\0\0\0", 8);
    return fwrite(hd, 1, sizeof(hd), f) == sizeof(hd) ? 0 : -1;
}
static int wav_end(struct recording *r) {
    uint8_t len[4];
    int rc = 0;
    if (!r->f) return 0;
    put_le(len, 36u + (uint32_t)r->bytes, 4);
    if (fseek(r->f, 4, SEEK_SET) != 0 || fwrite(len, 1, 4, r->f) != 4) rc = -1;
    put_le(len, (uint32_t)r->bytes, 4);
    if (fseek(r->f, 40, SEEK_SET) != 0 || fwrite(len, 1, 4, r->f) != 4) rc = -1;
    if (fclose(r->f) != 0) rc = -1;
    r->f = NULL;
    return rc;
}

/* --sizes a,b,c: consecutive legs.  The list goes to the library as it stands: what is wrong with it is the library's to say */
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
    for (int32_t r = 0; r < total; r++) conf_members[r] = r;
    *off_out = conf_off, *members_out = conf_members;
    return n_conf;
}

/* one tick of the network into a slot's rows */
static int audio_only, ulaw_every; /* ulaw_every 0: no leg negotiated PCMU */
static int is_ulaw_leg(int g) { return ulaw_every > 0 && g % ulaw_every == ulaw_every - 1; }
/* --dtmf: in the ticks DTMF_FROM .. DTMF_FROM + DTMF_PACKETS - 1 leg 0 presses the key `5` in band -- 770 Hz + 1336 Hz, each sine the
 * integer oscillator y[n] = ((c y[n-1]) >> 14) - y[n-2] with c = 2 cos w and y[0] = 4000 sin w in Q14, carried from packet to packet --
 * and leg 1 sends the key `#` as RFC 4733 packets of payload type 101: one timestamp, the last with the end bit.  What the script
 * had drawn for these legs in these ticks is replaced; every other leg's script is as without the flag. */
#define DTMF_FROM 5
#define DTMF_PACKETS 5
#define DTMF_EVENT_PT 101
static int dtmf;
static int32_t osc[2][2] = {{0, -((4000 * 9315) >> 14)}, {0, -((4000 * 14206) >> 14)}}; /* y[n-1], y[n-2] */
static void dtmf_packets(uint8_t *pk0, int32_t *rv, int g, int t, uint16_t *seq) {
    static const int32_t coef[2] = {26956, 16325};
    rv[0] = RTP_BYTES, rv[1] = rv[2] = 0;
    memset(pk0, 0, RTP_BYTES);
    pk0[0] = 2u << 6;
    pk0[2] = (uint8_t)(*seq >> 8), pk0[3] = (uint8_t)*seq;
    (*seq)++;
    if (g == 0) {
        pk0[1] = (uint8_t)(0x80 | (is_ulaw_leg(0) ? 0 : 8));
        for (int i = 0; i < 160; i++) {
            int32_t v = 0;
            for (int f = 0; f < 2; f++) {
                const int32_t y = (int32_t)(((int64_t)coef[f] * osc[f][0]) >> 14) - osc[f][1];
                osc[f][1] = osc[f][0], osc[f][0] = y;
                v += y;
            }
            pk0[12 + i] = is_ulaw_leg(0) ? linear2ulaw(v) : linear2alaw(v);
        }
    } else {
        const uint32_t ts = 160u * DTMF_FROM, duration = 160u * (uint32_t)(t - DTMF_FROM + 1);
        const int last = t == DTMF_FROM + DTMF_PACKETS - 1;
        pk0[1] = (uint8_t)((t == DTMF_FROM ? 0x80 : 0) | DTMF_EVENT_PT);
        pk0[4] = (uint8_t)(ts >> 24), pk0[5] = (uint8_t)(ts >> 16), pk0[6] = (uint8_t)(ts >> 8), pk0[7] = (uint8_t)ts;
        pk0[12] = 11; /* `#` */
        pk0[13] = (uint8_t)((last ? 0x80 : 0) | 10);
        pk0[14] = (uint8_t)(duration >> 8), pk0[15] = (uint8_t)duration;
        rv[0] = 16;
    }
}

static long arrivals(uint8_t *in, int32_t *recv, int row, uint16_t *seq, int G, int t) {
    long arrived = 0;
    memset(in, 0xEE, (size_t)G * RTP_SLOTS * row);
    for (int g = 0; g < G; g++) {
        const uint16_t seq_was = seq[g];
        const long arrived_was = arrived;
        const uint32_t u = lcg_next() % 8;
        int32_t *rv = recv + (size_t)g * RTP_SLOTS;
        rv[0] = u >= 2 ? RTP_BYTES : 0;
        rv[1] = u == 2 ? RTP_BYTES : (u == 3 ? -1 : 0);
        rv[2] = u == 3 ? RTP_BYTES : 0;
        for (int k = 0; k < RTP_SLOTS; k++) {
            if (rv[k] <= 0) continue;
            uint8_t *pk = in + ((size_t)g * RTP_SLOTS + k) * row;
            const uint32_t v = lcg_next() % 16;
            memset(pk, 0, 12);
            pk[0] = 2u << 6;
            pk[1] = (uint8_t)(0x80 | (v == 0 && !audio_only ? 96 : (v == 1 || is_ulaw_leg(g) ? 0 : 8)));
            pk[2] = (uint8_t)(seq[g] >> 8), pk[3] = (uint8_t)seq[g];
            seq[g]++;
            for (int i = 0; i < 160; i++) pk[12 + i] = (uint8_t)(lcg_next() & 255);
            arrived++;
        }
        if (dtmf && g < 2 && t >= DTMF_FROM && t < DTMF_FROM + DTMF_PACKETS) {
            seq[g] = seq_was;
            dtmf_packets(in + (size_t)g * RTP_SLOTS * row, rv, g, t, &seq[g]);
            arrived = arrived_was + 1;
        }
    }
    return arrived;
}

/* the slot's recorded rows into their files: row i is valid exactly when rec_legs[i] >= 0, and is that leg's; a tap that has written
 * its last row (50 x SECONDS of them) is closed there */
static int collect_rows(wmx_conf *h, int k, struct recording *rec, int n_rec, int rec_row) {
    const int16_t *rows = wmx_conf_rec(h, k);
    const int32_t *legs = wmx_conf_rec_legs(h, k);
    int failed = 0;
    if (!rows || !legs) return 1;
    for (int i = 0; i < n_rec; i++) {
        if (legs[i] < 0) continue;
        for (int j = 0; j < n_rec; j++) {
            if (rec[j].leg != legs[i] || !rec[j].f) continue;
            if (fwrite((const uint8_t *)rows + (size_t)i * (size_t)rec_row, 1, (size_t)rec_row, rec[j].f) != (size_t)rec_row) failed = 1;
            rec[j].rows++, rec[j].bytes += (unsigned long)rec_row;
            if (rec[j].seconds > 0 && rec[j].rows == 50ul * (unsigned long)rec[j].seconds && wav_end(&rec[j]) != 0) failed = 1;
            break;
        }
    }
    return failed;
}

int main(int argc, char **argv) {
    const char *usage = "usage: %s out.rtp n_legs n_ticks --sizes a,b,c --seed S [--slots K] [--speakers N[,floor[,shift]]] [--platform alsa|hi3516|t31]"
                        " [--sequence G] [--conceal] [--audio-only] [--ulaw-every N] [--dtmf] [--denoise] [--level V] [--gate] [--echo D]"
                        " [--prompt LEN,EVERY[,REPEAT[,GAP[,REDUCE]]]] [--record LEG[,CHN,FREQ[,SECONDS]]]... [--record-dir DIR]\n";
    if (argc < 4) {
        fprintf(stderr, usage, argv[0]);
        return 2;
    }
    const int G = atoi(argv[2]), T = atoi(argv[3]);
    const char *sizes = NULL, *speakers = NULL, *platform = "alsa";
    unsigned long seed = 0;
    int slots = 3, have_seed = 0, max_gap = -1, conceal = 0, denoise = 0, level = -1, gate = 0, echo = -1; /* max_gap -1: sequencing off; level -1: levelling off; echo -1: off */
    long correct = -1; /* -1: the library's default = platform/alsa */
    long prompt_len = 0; /* 0: no prompt */
    int prompt_every = 0, prompt_repeat = 1, prompt_gap = 0, prompt_reduce = -1; /* -1: no fifth field, wmx_conf_play */
    static struct recording rec[MAX_RECORDS];
    int n_rec = 0, rec_chn = 0, rec_freq = 0;
    const char *rec_dir = ".";
    for (int i = 4; i < argc; i++) {
        if (!strcmp(argv[i], "--sizes") && i + 1 < argc) {
            sizes = argv[++i];
        } else if (!strcmp(argv[i], "--seed") && i + 1 < argc) {
            seed = strtoul(argv[++i], NULL, 10), have_seed = 1;
        } else if (!strcmp(argv[i], "--slots") && i + 1 < argc) {
            slots = atoi(argv[++i]);
        } else if (!strcmp(argv[i], "--speakers") && i + 1 < argc) {
            speakers = argv[++i];
        } else if (!strcmp(argv[i], "--sequence") && i + 1 < argc) {
            max_gap = atoi(argv[++i]);
            if (max_gap < 0) max_gap = WMX_MIX_MAX_LEG_PACKETS; /* not a gap: the library says so */
        } else if (!strcmp(argv[i], "--conceal")) {
            conceal = 1;
        } else if (!strcmp(argv[i], "--dtmf")) {
            dtmf = 1;
        } else if (!strcmp(argv[i], "--denoise")) {
            denoise = 1;
        } else if (!strcmp(argv[i], "--gate")) {
            gate = 1;
        } else if (!strcmp(argv[i], "--echo") && i + 1 < argc) {
            echo = atoi(argv[++i]);
            if (echo < 0) {
                fprintf(stderr, usage, argv[0]);
                return 2;
            }
        } else if (!strcmp(argv[i], "--prompt") && i + 1 < argc) {
            const int fields = sscanf(argv[++i], "%ld,%d,%d,%d,%d", &prompt_len, &prompt_every, &prompt_repeat, &prompt_gap, &prompt_reduce);
            if (fields < 5) prompt_reduce = -1;
            if (fields < 2 || prompt_len < 1 || prompt_every < 1) {
                fprintf(stderr, "host_conf: --prompt LEN,EVERY[,REPEAT[,GAP[,REDUCE]]], LEN >= 1, EVERY >= 1\n");
                return 2;
            }
        } else if (!strcmp(argv[i], "--record") && i + 1 < argc) {
            int leg = -1, chn = 1, freq = 8000, seconds = 0;
            const int fields = sscanf(argv[++i], "%d,%d,%d,%d", &leg, &chn, &freq, &seconds);
            if (fields < 1 || fields == 2 || leg < 0 || seconds < 0 || n_rec == MAX_RECORDS || (n_rec && (chn != rec_chn || freq != rec_freq))) {
                fprintf(stderr, "host_conf: --record LEG[,CHN,FREQ[,SECONDS]], at most %d of them and ONE format for all\n", MAX_RECORDS);
                return 2;
            }
            rec_chn = chn, rec_freq = freq; /* what is wrong with the format or the leg is the library's to say */
            rec[n_rec].leg = leg, rec[n_rec].seconds = seconds;
            n_rec++;
        } else if (!strcmp(argv[i], "--record-dir") && i + 1 < argc) {
            rec_dir = argv[++i];
        } else if (!strcmp(argv[i], "--level") && i + 1 < argc) {
            level = atoi(argv[++i]);
            if (level < 0) {
                fprintf(stderr, usage, argv[0]);
                return 2;
            }
        } else if (!strcmp(argv[i], "--audio-only")) {
            audio_only = 1;
        } else if (!strcmp(argv[i], "--ulaw-every") && i + 1 < argc) {
            ulaw_every = atoi(argv[++i]);
            if (ulaw_every < 1) {
                fprintf(stderr, "host_conf: --ulaw-every N, N >= 1\n");
                return 2;
            }
        } else if (!strcmp(argv[i], "--platform") && i + 1 < argc) {
            platform = argv[++i];
            if (!strcmp(platform, "alsa")) {
                correct = 3200;
            } else if (!strcmp(platform, "hi3516") || !strcmp(platform, "t31")) {
                correct = 0;
            } else {
                fprintf(stderr, "host_conf: no platform directory '%s' in the reference\n", platform);
                return 2;
            }
        } else {
            fprintf(stderr, "host_conf: what is '%s'?\n", argv[i]);
            return 2;
        }
    }
    if (!sizes || !have_seed) {
        fprintf(stderr, "host_conf: --sizes and --seed are needed\n");
        fprintf(stderr, usage, argv[0]);
        return 2;
    }
    if (G < 1 || T < 1) return 2;
    int max_speakers = 0, shift = 3;
    unsigned long floor_level = 0;
    if (speakers && sscanf(speakers, "%d,%lu,%d", &max_speakers, &floor_level, &shift) < 1) {
        fprintf(stderr, "host_conf: --speakers N[,floor[,shift]]\n");
        return 2;
    }
    int32_t *conf_off = NULL, *conf_members = NULL;
    const int n_conf = parse_sizes(sizes, &conf_off, &conf_members);
    if (n_conf < 0) return 2;

    wmx_conf *h = NULL;
    WMX_OK(wmx_conf_create(&h, G, slots, RTP_SLOTS, WMX_LAW_A));
    if (correct >= 0) WMX_OK(wmx_conf_set_play_correct(h, (uint32_t)correct));
    WMX_OK(wmx_conf_set_conferences(h, n_conf, conf_off, conf_members, NULL));
    if (speakers) WMX_OK(wmx_conf_speakers(h, max_speakers, (uint32_t)floor_level, shift));
    if (max_gap >= 0) WMX_OK(wmx_conf_sequence(h, 1, max_gap));
    if (conceal) WMX_OK(wmx_conf_conceal(h, 1));
    if (dtmf) WMX_OK(wmx_conf_dtmf(h, 1, 1, DTMF_EVENT_PT));
    if (denoise) WMX_OK(wmx_conf_denoise(h, 1));
    if (level >= 0) WMX_OK(wmx_conf_level(h, 1, level));
    if (gate) WMX_OK(wmx_conf_gate(h, 1));
    if (echo >= 0) WMX_OK(wmx_conf_echo(h, 1, echo));
    int n_prompt_legs = 0;
    if (prompt_len > 0) { /* what is wrong with REPEAT, GAP or REDUCE is the library's to say */
        int16_t *pcm = malloc((size_t)prompt_len * sizeof(int16_t));
        int clip = -1;
        if (!pcm) return 2;
        lcg_state = seed + 1;
        for (long i = 0; i < prompt_len; i++) pcm[i] = (int16_t)((int32_t)(lcg_next() & 16383u) - 8192);
        WMX_OK(wmx_conf_prompts(h, 1, prompt_len));
        WMX_OK(wmx_conf_add_clip(h, pcm, prompt_len, &clip));
        free(pcm);
        for (int g = prompt_every - 1; g < G; g += prompt_every) {
            const int32_t leg = g;
            if (prompt_reduce == -1)
                WMX_OK(wmx_conf_play(h, &leg, 1, clip, prompt_repeat, prompt_gap, NULL));
            else
                WMX_OK(wmx_conf_play_duck(h, &leg, 1, clip, prompt_repeat, prompt_gap, prompt_reduce, NULL));
            n_prompt_legs++;
        }
    }
    int n_ulaw = 0;
    for (int g = 0; g < G; g++) {
        const int32_t leg = g;
        if (!is_ulaw_leg(g)) continue;
        WMX_OK(wmx_conf_set_codecs(h, &leg, 1, WMX_CODEC_PCMU, WMX_LAW_U, NULL));
        n_ulaw++;
    }
    int rec_row = 0; /* the bytes of a recorded row */
    if (n_rec > 0) {
        WMX_OK(wmx_conf_recorders(h, n_rec, rec_chn, rec_freq));
        rec_row = wmx_conf_rec_row_bytes(h);
        for (int i = 0; i < n_rec; i++) {
            char path[4096];
            const int32_t leg = rec[i].leg;
            int32_t tap = -1;
            snprintf(path, sizeof(path), "%s/leg%d.wav", rec_dir, rec[i].leg);
            WMX_OK(wmx_conf_record(h, &leg, 1, 50 * rec[i].seconds, &tap, NULL));
            if (tap < 0 || tap >= n_rec) return 4;
            if (!rec[i].f && (!(rec[i].f = fopen(path, "wb")) || wav_begin(rec[i].f, rec_chn, rec_freq) != 0)) {
                fprintf(stderr, "host_conf: cannot write %s\n", path);
                return 7;
            }
        }
    }
    int rec_failed = 0;
    const int row = wmx_conf_in_row_bytes(h);
    uint8_t *out = calloc((size_t)T * G * RTP_BYTES, 1);
    uint16_t *seq = calloc((size_t)G, sizeof(uint16_t));
    int *tick_of = malloc((size_t)slots * sizeof(int)); /* the tick whose datagrams a slot still owes, or -1 */
    if (!out || !seq || !tick_of || row < RTP_BYTES) return 2;
    for (int k = 0; k < slots; k++) tick_of[k] = -1;
    lcg_state = seed;
    long arrived = 0;
    const double t0 = now_ms();
#define COLLECT(k)                                                                                              \
    do {                                                                                                        \
        if (tick_of[k] >= 0) {                                                                                  \
            WMX_OK(wmx_conf_wait(h, (k)));                                                                      \
            memcpy(out + (size_t)tick_of[k] * G * RTP_BYTES, wmx_conf_out(h, (k)), (size_t)G * RTP_BYTES);      \
            if (n_rec > 0) rec_failed |= collect_rows(h, (k), rec, n_rec, rec_row);                             \
            tick_of[k] = -1;                                                                                    \
        }                                                                                                       \
    } while (0)
    arrived += arrivals(wmx_conf_in(h, 0), wmx_conf_recv(h, 0), row, seq, G, 0);
    for (int t = 0; t < T; t++) {
        int k = -1;
        WMX_OK(wmx_conf_submit(h, &k, NULL));
        tick_of[k] = t;
        if (t + 1 < T) { /* the network of tick t + 1 while tick t is in flight; that slot's own earlier tick has to have left first */
            const int nk = wmx_conf_next_slot(h);
            COLLECT(nk);
            arrived += arrivals(wmx_conf_in(h, nk), wmx_conf_recv(h, nk), row, seq, G, t + 1);
        }
    }
    for (int i = 0, first = wmx_conf_next_slot(h); i < slots; i++) COLLECT((first + i) % slots); /* oldest first: the recorded rows are appended */
    const double wall = now_ms() - t0;
    unsigned long n_rec_rows = 0;
    for (int i = 0; i < n_rec; i++) { /* the taps that ran until the end */
        if (wav_end(&rec[i]) != 0) rec_failed = 1;
        n_rec_rows += rec[i].rows;
    }
    uint32_t *dropped = calloc((size_t)G, sizeof(uint32_t));
    if (!dropped) return 2;
    WMX_OK(wmx_conf_export_legs(h, NULL, NULL, dropped, NULL, NULL, NULL));
    unsigned long n_dropped = 0;
    for (int g = 0; g < G; g++) n_dropped += dropped[g];
    unsigned long seq_sum[5] = {0, 0, 0, 0, 0}; /* lost, late, dup, resync, overflow over the legs */
    if (max_gap >= 0) {
        uint32_t *cnt = calloc((size_t)G * 5, sizeof(uint32_t));
        if (!cnt) return 2;
        WMX_OK(wmx_conf_export_sequence(h, NULL, NULL, cnt, cnt + G, cnt + 2 * (size_t)G, cnt + 3 * (size_t)G, cnt + 4 * (size_t)G, NULL));
        for (int c = 0; c < 5; c++)
            for (int g = 0; g < G; g++) seq_sum[c] += cnt[(size_t)c * G + g];
        free(cnt);
    }
    unsigned long n_concealed = 0;
    if (conceal) {
        uint32_t *cnt = calloc((size_t)G, sizeof(uint32_t));
        if (!cnt) return 2;
        WMX_OK(wmx_conf_export_conceal(h, cnt, NULL));
        for (int g = 0; g < G; g++) n_concealed += cnt[g];
        free(cnt);
    }
    unsigned long n_refused = 0;
    if (ulaw_every > 0) {
        uint32_t *refused = calloc((size_t)G, sizeof(uint32_t));
        if (!refused) return 2;
        WMX_OK(wmx_conf_export_codecs(h, NULL, NULL, refused, NULL));
        for (int g = 0; g < G; g++) n_refused += refused[g];
        free(refused);
    }
    uint32_t *key_count = NULL; /* --dtmf: count and ring of every leg */
    uint8_t *key_ring = NULL;
    if (dtmf) {
        key_count = calloc((size_t)G, sizeof(uint32_t));
        key_ring = calloc((size_t)G, 8);
        if (!key_count || !key_ring) return 2;
        WMX_OK(wmx_conf_export_dtmf(h, key_count, key_ring, NULL));
    }
    unsigned long n_voiced = 0, n_unvoiced = 0;
    if (gate) {
        uint32_t *cnt = calloc(2 * (size_t)G, sizeof(uint32_t));
        if (!cnt) return 2;
        WMX_OK(wmx_conf_export_gate(h, NULL, cnt, cnt + G, NULL));
        for (int g = 0; g < G; g++) n_voiced += cnt[g], n_unvoiced += cnt[G + g];
        free(cnt);
    }
    int echo_running = 0;
    if (echo >= 0) {
        int32_t *startup = calloc((size_t)G, sizeof(int32_t));
        if (!startup) return 2;
        WMX_OK(wmx_conf_export_echo(h, startup, NULL, NULL, NULL, NULL));
        for (int g = 0; g < G; g++) echo_running += startup[g] == 0;
        free(startup);
    }
    unsigned long n_prompt_done = 0;
    if (prompt_len > 0) {
        uint32_t *done = calloc((size_t)G, sizeof(uint32_t));
        if (!done) return 2;
        WMX_OK(wmx_conf_export_prompts(h, NULL, NULL, NULL, done, NULL));
        for (int g = 0; g < G; g++) n_prompt_done += done[g];
        free(done);
    }
    int n_prompt_ducking = 0;
    if (prompt_len > 0 && prompt_reduce != -1) {
        uint8_t *divisor = calloc((size_t)G, 1);
        if (!divisor) return 2;
        WMX_OK(wmx_conf_export_duck(h, divisor, NULL));
        for (int g = 0; g < G; g++) n_prompt_ducking += divisor[g] > 1;
        free(divisor);
    }
    uint64_t sum = 1469598103934665603ull; /* FNV-1a over the datagrams that went out */
    for (size_t i = 0; i < (size_t)T * G * RTP_BYTES; i++) sum = (sum ^ out[i]) * 1099511628211ull;
    wmx_conf_destroy(h);
    FILE *f = fopen(argv[1], "wb");
    int rc = (!f || fwrite(out, 1, (size_t)T * G * RTP_BYTES, f) != (size_t)T * G * RTP_BYTES || rec_failed) ? 7 : 0;
    if (f) fclose(f);
    printf("{\"groups\": %d, \"ticks\": %d, \"platform\": \"%s\", \"bridge_rtp_seed\": %lu, \"bridge_sizes\": [", G, T, platform, seed);
    for (int c = 0; c < n_conf; c++) printf("%s%d", c ? ", " : "", (int)(conf_off[c + 1] - conf_off[c]));
    printf("], ");
    if (max_gap >= 0)
        printf("\"sequence\": %d, \"lost\": %lu, \"late\": %lu, \"dup\": %lu, \"resync\": %lu, \"overflow\": %lu, ", max_gap, seq_sum[0], seq_sum[1],
               seq_sum[2], seq_sum[3], seq_sum[4]);
    if (conceal) printf("\"conceal\": 1, \"concealed\": %lu, ", n_concealed);
    if (ulaw_every > 0) printf("\"ulaw_every\": %d, \"ulaw_legs\": %d, \"refused\": %lu, ", ulaw_every, n_ulaw, n_refused);
    if (dtmf) {
        printf("\"dtmf\": 1, \"dtmf_keys\": [");
        int first = 1;
        for (int g = 0; g < G; g++)
            for (uint32_t n = key_count[g] > 8 ? key_count[g] - 8 : 0; n < key_count[g]; n++, first = 0) {
                const uint8_t b = key_ring[(size_t)g * 8 + (n & 7)];
                printf("%s{\"leg\": %d, \"key\": \"%c\", \"packet\": %d}", first ? "" : ", ", g, "0123456789*#ABCD"[b & 15], b >> 7);
            }
        printf("], ");
    }
    if (denoise) printf("\"denoise\": 1, ");
    if (level >= 0) printf("\"level\": %d, ", level);
    if (gate) printf("\"gate\": 1, \"voiced\": %lu, \"unvoiced\": %lu, ", n_voiced, n_unvoiced);
    if (echo >= 0) printf("\"echo\": %d, \"echo_running\": %d, ", echo, echo_running);
    if (prompt_len > 0) printf("\"prompt\": %ld, \"prompt_legs\": %d, \"prompt_done\": %lu, ", prompt_len, n_prompt_legs, n_prompt_done);
    if (prompt_len > 0 && prompt_reduce != -1) printf("\"prompt_reduce\": %d, \"prompt_ducking\": %d, ", prompt_reduce, n_prompt_ducking);
    if (n_rec > 0) printf("\"record_taps\": %d, \"record_format\": [%d, %d], \"record_rows\": %lu, ", n_rec, rec_chn, rec_freq, n_rec_rows);
    printf("\"slots\": %d, \"speakers\": %d, \"datagrams_in\": %ld, \"dropped\": %lu, \"datagrams_fnv1a\": \"%016llx\", \"wall_ms\": %.3f, "
           "\"ms_per_tick\": %.4f, \"rc\": %d}\n",
           slots, max_speakers, arrived, n_dropped, (unsigned long long)sum, wall, wall / T, rc);
    return rc;
}
