// leg_plc_san.cpp -- the bridge's concealment rule (wmix_amd/csrc/leg_plc.h) as a stand-alone CPU program, for AddressSanitizer +
// UndefinedBehaviorSanitizer (tools_dev/san/Makefile).  No HIP, no GPU.
//
//   leg_plc_san           the built-in sweep: every call list of 0 .. 4 calls, each a silence call or a data call (call j names slot
//                         j mod 3 of three; slot 2 is not readable), over eight histories -- zero, the extremes -32768 and +32767 (the
//                         overflow bounds), square waves of period 40, 50 and 120 at full scale and two of random samples; per case an
//                         input line and a result line
//   leg_plc_san cases     one result line per case read from stdin: max_packets calls, max_packets lens, 320 samples of history,
//                         max_packets x 160 samples of rows
// An input line: "in" and the case in the stdin format.  A result line: count, len_out[4], concealed, the 320 samples of history
// afterwards, count x 160 emitted samples.  Every case also checks what any tick satisfies; a violation is counted and fails the run.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "leg_plc.h"

using namespace wmx;

static long bad = 0;

static void one(int max_packets, uint32_t calls, const uint32_t *len, const int16_t *hist, const int16_t *rows, bool echo) {
    if (echo) {
        printf("in %d %u", max_packets, calls);
        for (int k = 0; k < max_packets; k++) printf(" %u", len[k]);
        for (int i = 0; i < kPlcHist; i++) printf(" %d", hist[i]);
        for (int i = 0; i < max_packets * kLegRow; i++) printf(" %d", rows[i]);
        printf("\n");
    }
    LegPlcState st;
    for (int i = 0; i < kPlcHist; i++) st.hist[i] = hist[i];
    st.concealed = 0;
    // exactly as many rows as there are calls: a write behind them is the sanitizer's to report
    const uint32_t count = leg_calls_walked(calls);
    std::vector<int16_t> out((size_t)count * kLegRow, (int16_t)0x5A5A);
    uint32_t len_out[kLegMaxCalls];
    leg_plc_tick(st, rows, kLegRow, len, max_packets, calls, out.data(), len_out);
    printf("%u %u %u %u %u %u", count, len_out[0], len_out[1], len_out[2], len_out[3], st.concealed);
    for (int i = 0; i < kPlcHist; i++) printf(" %d", st.hist[i]);
    for (uint32_t i = 0; i < count * kLegRow; i++) printf(" %d", out[i]);
    printf("\n");
    // what any tick satisfies: the history afterwards is the tail of (history, emitted rows), so a list without calls changes nothing;
    // concealed counts the silence calls
    for (int i = 0; i < kPlcHist; i++) {
        const int at = (int)count * kLegRow + i;  // in the sequence history ++ rows
        const int16_t want = at < kPlcHist ? hist[at] : out[(size_t)(at - kPlcHist)];
        if (st.hist[i] != want) bad++;
    }
    uint32_t readable = 0, silent = 0;
    for (int k = 0; k < max_packets; k++) readable |= leg_row_readable(len[k]) << k;
    for (uint32_t j = 0; j < count; j++) silent += leg_calls_adds_nothing(calls, j, readable) ? 1u : 0u;
    if (st.concealed != silent) bad++;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

int main(int argc, char **argv) {
    if (argc > 1) {
        int max_packets;
        unsigned calls;
        while (scanf("%d %u", &max_packets, &calls) == 2) {
            if (max_packets < 1 || max_packets > kLegMaxCalls) return 2;
            uint32_t len[kLegMaxCalls] = {0u, 0u, 0u, 0u};
            std::vector<int16_t> hist(kPlcHist), rows((size_t)max_packets * kLegRow);
            int v;
            for (int k = 0; k < max_packets; k++)
                if (scanf("%u", &len[k]) != 1) return 2;
            for (int16_t &s : hist) {
                if (scanf("%d", &v) != 1) return 2;
                s = (int16_t)v;
            }
            for (int16_t &s : rows) {
                if (scanf("%d", &v) != 1) return 2;
                s = (int16_t)v;
            }
            one(max_packets, calls, len, hist.data(), rows.data(), false);
        }
    } else {
        const int K = 3;
        const uint32_t len[kLegMaxCalls] = {kLegRowBytes, kLegRowBytes, 0u, 0u};
        for (int hk = 0; hk < 8; hk++) {
            int16_t hist[kPlcHist];
            const int period = hk == 3 ? 40 : (hk == 4 ? 50 : 120);
            for (int i = 0; i < kPlcHist; i++)
                hist[i] = hk == 0   ? (int16_t)0
                          : hk == 1 ? (int16_t)-32768
                          : hk == 2 ? (int16_t)32767
                          : hk <= 5 ? (int16_t)(i % period < period / 2 ? 32767 : -32768)
                                    : (int16_t)(rnd() & 0xFFFFu);
            for (uint32_t count = 0; count <= (uint32_t)kLegMaxCalls; count++)
                for (uint32_t pick = 0; pick < (1u << count); pick++) {
                    uint32_t calls = 0;
                    for (uint32_t j = 0; j < count; j++) calls = leg_calls_push(calls, (pick >> j) & 1u ? 0u : j % 3u, (pick >> j) & 1u);
                    int16_t rows[K * kLegRow];
                    for (int16_t &s : rows) s = (int16_t)(rnd() & 0xFFFFu);
                    one(K, calls, len, hist, rows, true);
                }
        }
    }
    if (bad) fprintf(stderr, "%ld values break what every tick satisfies\n", bad);
    return bad ? 1 : 0;
}
