// leg_dtmf_san.cpp -- the bridge's DTMF rule (wmix_amd/csrc/leg_dtmf.h) as a stand-alone CPU program, for AddressSanitizer +
// UndefinedBehaviorSanitizer (tools_dev/san/Makefile).  No HIP, no GPU.
//
//   leg_dtmf_san blocks   one result line per block read from stdin (160 samples): the eight powers, E, the digit or -1, and the
//                         largest |s| any of the eight recurrences reached
//   leg_dtmf_san ticks    a script from stdin.  "L event_pt suppress" starts a fresh leg.  "T max_packets have_calls calls", then
//                         max_packets recv, max_packets len, per slot the first 16 bytes of the datagram row and 160 samples: one tick,
//                         answered by a result line: the number of blocks, the four per-block digits, count, the eight ring bytes, and
//                         the max_packets x 160 samples of the rows afterwards
// The datagram rows are exactly 16 bytes long and the PCM rows exactly 160 samples: a read behind them is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "leg_dtmf.h"

using namespace wmx;

static bool read_row(int16_t *x) {
    for (int i = 0; i < kLegRow; i++) {
        int v;
        if (scanf("%d", &v) != 1) return false;
        x[i] = (int16_t)v;
    }
    return true;
}

static int blocks() {
    std::vector<int16_t> x(kLegRow);
    while (read_row(x.data())) {
        int64_t p[kDtmfFreqs], e = 0;
        const int32_t digit = leg_dtmf_block_digit(x.data(), p, &e);
        int64_t reach = 0;
        for (int f = 0; f < kDtmfFreqs; f++) {
            int32_t s1 = 0, s2 = 0;
            for (int n = 0; n < kLegRow; n++) {
                leg_dtmf_step(s1, s2, leg_dtmf_coef(f), x[n]);
                const int64_t a = s1 < 0 ? -(int64_t)s1 : (int64_t)s1;
                reach = a > reach ? a : reach;
            }
        }
        for (int f = 0; f < kDtmfFreqs; f++) printf("%lld ", (long long)p[f]);
        printf("%lld %d %lld\n", (long long)e, digit, (long long)reach);
    }
    return 0;
}

static int ticks() {
    LegDtmfState st{0u, 0u, 0u, 0u};
    unsigned event_pt = 101;
    int suppress = 0;
    char what[4];
    while (scanf("%3s", what) == 1) {
        if (what[0] == 'L') {
            if (scanf("%u %d", &event_pt, &suppress) != 2) return 2;
            st = LegDtmfState{0u, 0u, 0u, 0u};
            continue;
        }
        int max_packets, have_calls;
        unsigned calls;
        if (what[0] != 'T' || scanf("%d %d %u", &max_packets, &have_calls, &calls) != 3 || max_packets < 1 || max_packets > kLegMaxCalls) return 2;
        std::vector<int32_t> recv((size_t)max_packets);
        std::vector<uint32_t> len((size_t)max_packets);
        std::vector<uint8_t> pk((size_t)max_packets * kDtmfMinEventBytes);
        std::vector<int16_t> pcm((size_t)max_packets * kLegRow);
        for (int32_t &r : recv)
            if (scanf("%d", &r) != 1) return 2;
        for (uint32_t &l : len)
            if (scanf("%u", &l) != 1) return 2;
        for (int k = 0; k < max_packets; k++) {
            for (uint32_t i = 0; i < kDtmfMinEventBytes; i++) {
                unsigned b;
                if (scanf("%u", &b) != 1) return 2;
                pk[(size_t)k * kDtmfMinEventBytes + i] = (uint8_t)b;
            }
            if (!read_row(pcm.data() + (size_t)k * kLegRow)) return 2;
        }
        int32_t digits[kLegMaxCalls];
        const uint32_t n = leg_dtmf_tick(st, pk.data(), (long)kDtmfMinEventBytes, recv.data(), pcm.data(), kLegRow, len.data(), max_packets,
                                         have_calls != 0, calls, event_pt, suppress != 0, digits);
        printf("%u %d %d %d %d %u", n, digits[0], digits[1], digits[2], digits[3], st.count);
        uint8_t ring[8];
        memcpy(ring, &st.ring, 8);  // the bytes as the device stores them
        for (int i = 0; i < 8; i++) printf(" %u", ring[i]);
        for (int16_t s : pcm) printf(" %d", s);
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "blocks")) return blocks();
    if (argc > 1 && !strcmp(argv[1], "ticks")) return ticks();
    fprintf(stderr, "usage: leg_dtmf_san blocks | ticks  < cases\n");
    return 2;
}
