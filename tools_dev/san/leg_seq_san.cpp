// leg_seq_san.cpp -- the bridge's sequence rule (wmix_amd/csrc/leg_seq.h) and the cursor rule over a call list
// (leg_cursor_span_calls, wmix_amd/csrc/leg_cursor.h) as a stand-alone CPU program, for AddressSanitizer + UndefinedBehaviorSanitizer
// (tools_dev/san/Makefile).  No HIP, no GPU.
//
//   leg_seq_san           the sweep: four slots, each absent or next + o for o in {-17, -16, -2, -1, 0, 1, 2, 3, 4, 5, 40000}, every
//                         max_gap 0 .. 3, synced and unsynced, next in {0, 65534}; one result line per case in sweep order
//   leg_seq_san cases     one result line per case read from stdin: max_gap synced next s0 s1 s2 s3 (s < 0: the slot is absent)
// A result line: calls discard synced next lost late dup resync overflow.  Every case also runs its call list through
// leg_cursor_span_calls and checks what any list must satisfy; a violation is counted and fails the run.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include "leg_cursor.h"
#include "leg_seq.h"

using namespace wmx;

static long bad = 0;

static void one(uint32_t max_gap, uint32_t synced, uint32_t next, const long s[4]) {
    LegSeqState st{synced, next, 0u, 0u, 0u, 0u, 0u};
    uint32_t seq[kLegMaxCalls] = {0u, 0u, 0u, 0u}, ok = 0;
    for (int k = 0; k < kLegMaxCalls; k++)
        if (s[k] >= 0) seq[k] = (uint32_t)s[k] & 0xFFFFu, ok |= 1u << k;
    const LegSeqTick r = leg_seq_tick(st, seq, ok, max_gap);
    printf("%u %u %u %u %u %u %u %u %u\n", r.calls, r.discard, st.synced, st.next, st.lost, st.late, st.dup, st.resync, st.overflow);
    // what any list satisfies: at most four calls, data calls name distinct ok slots that are not discarded, every ok slot is a data
    // call or discarded, the silence calls are the packets counted lost
    const uint32_t n = leg_calls_count(r.calls);
    uint32_t used = 0, silent = 0;
    if (n > (uint32_t)kLegMaxCalls || (r.calls >> (4u + 4u * n)) != 0u) bad++;
    for (uint32_t j = 0; j < n && j < (uint32_t)kLegMaxCalls; j++) {
        if (leg_calls_silence(r.calls, j)) {
            silent++;
            continue;
        }
        const uint32_t k = leg_calls_slot(r.calls, j);
        if ((used >> k) & 1u) bad++;
        used |= 1u << k;
    }
    if ((used & r.discard) || (used | r.discard) != ok || silent != st.lost) bad++;
    if (n && leg_calls_silence(r.calls, n - 1)) bad++;  // no trailing silence
    // the list through the cursor rule: the calls made, and the slots and the silence mask in list order
    const LegMixState ms{3200u, 1000000u, 3200u, 16000u};
    const LegSpanCalls sp = leg_cursor_span_calls(ms, 160u, leg_cursor_fresh(), r.calls);
    if (sp.span.count != n || sp.span.dropped != 0u || (n && sp.span.after.tick != ms.tick + ms.play_correct + 320u * n)) bad++;
    for (uint32_t j = 0; j < n && j < (uint32_t)kLegMaxCalls; j++)
        if (((sp.silence >> j) & 1u) != leg_calls_silence(r.calls, j) || ((sp.span.slots >> (2u * j)) & 3u) != leg_calls_slot(r.calls, j)) bad++;
}

int main(int argc, char **argv) {
    if (argc > 1) {
        unsigned max_gap, synced, next;
        long s[4];
        while (scanf("%u %u %u %ld %ld %ld %ld", &max_gap, &synced, &next, &s[0], &s[1], &s[2], &s[3]) == 7) one(max_gap, synced, next, s);
    } else {
        const long off[] = {-17, -16, -2, -1, 0, 1, 2, 3, 4, 5, 40000};
        const int n_opt = 1 + (int)(sizeof(off) / sizeof(off[0]));  // option 0: absent
        for (uint32_t max_gap = 0; max_gap < 4; max_gap++)
            for (uint32_t synced = 0; synced < 2; synced++)
                for (uint32_t next : {0u, 65534u})
                    for (int a = 0; a < n_opt; a++)
                        for (int b = 0; b < n_opt; b++)
                            for (int c = 0; c < n_opt; c++)
                                for (int d = 0; d < n_opt; d++) {
                                    const int pick[4] = {a, b, c, d};
                                    long s[4];
                                    for (int k = 0; k < 4; k++) s[k] = pick[k] ? (long)(((long)next + off[pick[k] - 1] + 65536) % 65536) : -1;
                                    one(max_gap, synced, next, s);
                                }
    }
    if (bad) fprintf(stderr, "%ld cases break what every call list satisfies\n", bad);
    return bad ? 1 : 0;
}
