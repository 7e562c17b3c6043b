// leg_calls_san.cpp -- the walk over a leg's rows of a tick (leg_calls_walk, wmix_amd/csrc/leg_calls.h) as a stand-alone CPU program, for
// AddressSanitizer + UndefinedBehaviorSanitizer (tools_dev/san/Makefile).  No HIP, no GPU.
//
//   leg_calls_san         every case, one result line each: list count data
// First the list form, four slots: every count 0 .. 7, every (slot, silence) of the four entries (entry j is bits 3 j .. 3 j + 2 of a
// number 0 .. 4095: two bits of slot, one of silence), every readable mask 0 .. 15 -- in that nesting, the mask innermost.  Then the
// slot-order form: every readable mask 0 .. 15, every max_packets 1 .. 4, max_packets innermost.  A slot that is not readable holds one
// of the lengths that are not 320.  Every case also checks what any walk satisfies; a violation is counted and fails the run.
#include <cstdint>
#include <cstdio>
#include "leg_calls.h"

using namespace wmx;

static long bad = 0;

static void one(uint32_t mask, bool have_calls, uint32_t calls, int max_packets) {
    static const uint32_t kNot[kLegMaxCalls] = {0u, kLegRowBytes - 1u, kLegRowBytes + 1u, (uint32_t)kLegRow};
    // exactly max_packets entries: a read behind them is the sanitizer's to report
    uint32_t *len = new uint32_t[max_packets];
    for (int k = 0; k < max_packets; k++) len[k] = (mask >> k) & 1u ? kLegRowBytes : kNot[(mask + (uint32_t)k) % kLegMaxCalls];
    const LegWalk w = leg_calls_walk(len, have_calls, calls, max_packets);
    delete[] len;
    printf("%u %u %u\n", w.list, w.count, w.data);
    // what any walk satisfies: at most four calls, no data bit at or behind the count, a data call names a readable slot below
    // max_packets, and without a list every call is a data call
    if (w.count > (uint32_t)kLegMaxCalls || (w.data >> w.count) != 0u || w.readable != (mask & ((1u << max_packets) - 1u))) bad++;
    for (uint32_t j = 0; j < w.count; j++)
        if (((w.data >> j) & 1u) && (!((w.readable >> leg_calls_slot(w.list, j)) & 1u) || leg_calls_silence(w.list, j))) bad++;
    if (!have_calls && w.data != (1u << w.count) - 1u) bad++;
}

int main() {
    for (uint32_t count = 0; count < 8; count++)
        for (uint32_t entries = 0; entries < 4096; entries++) {
            uint32_t calls = count;
            for (uint32_t j = 0; j < (uint32_t)kLegMaxCalls; j++) calls |= ((entries >> (3u * j)) & 7u) << (4u + 4u * j);
            for (uint32_t mask = 0; mask < 16; mask++) one(mask, true, calls, kLegMaxCalls);
        }
    for (uint32_t mask = 0; mask < 16; mask++)
        for (int max_packets = 1; max_packets <= kLegMaxCalls; max_packets++) one(mask, false, 0xFFFFFFFFu, max_packets);
    if (bad) fprintf(stderr, "%ld cases break what every walk satisfies\n", bad);
    return bad ? 1 : 0;
}
