// leg_record_san.cpp -- the recording taps of the bridge (wmix_amd/csrc/leg_record.h) as a stand-alone CPU program, for AddressSanitizer
// + UndefinedBehaviorSanitizer (tools_dev/san/Makefile).  No HIP, no GPU.
//
//   leg_record_san MAX_TAPS < script      one command per line:
//     start TICKS N LEG..   the N legs start, TICKS rows each (all or nothing)   -> "taps K.." or "refused"
//     stop N LEG..          those legs' taps are free; N = -1: every tap
//     reset N LEG..         the same with written = 0
//     tick                  one tick of every tap                                -> "rows LEG.." (the leg per tap, -1 for none)
// and behind every command one line with the state: leg left written per tap.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "leg_record.h"

using namespace wmx;

int main(int argc, char **argv) {
    const int max_taps = argc > 1 ? atoi(argv[1]) : 0;
    if (max_taps < 1) return 2;
    std::vector<LegRecord> taps((size_t)max_taps, leg_record_free(0u));
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "tick")) {
            printf("rows");
            for (LegRecord &r : taps) printf(" %d", (int)leg_record_tick(r));
            printf("\n");
        } else {
            int ticks = 0, n = 0;
            if (!strcmp(cmd, "start") && scanf("%d", &ticks) != 1) return 2;
            if (scanf("%d", &n) != 1) return 2;
            std::vector<int32_t> legs((size_t)(n > 0 ? n : 0)), out(legs.size());
            for (int32_t &g : legs)
                if (scanf("%d", &g) != 1) return 2;
            if (!strcmp(cmd, "start")) {
                if (leg_record_assign(taps.data(), max_taps, legs.data(), (int)legs.size(), out.data())) {
                    printf("taps");
                    for (size_t i = 0; i < legs.size(); i++) {
                        taps[(size_t)out[i]] = leg_record_start(legs[i], (uint32_t)ticks);
                        printf(" %d", (int)out[i]);
                    }
                    printf("\n");
                } else {
                    printf("refused\n");
                }
            } else {
                const bool keep = !strcmp(cmd, "stop");
                if (!keep && strcmp(cmd, "reset")) return 2;
                for (LegRecord &r : taps) {
                    bool listed = n < 0;
                    for (int32_t g : legs) listed = listed || (r.leg >= 0 && r.leg == g);
                    if (listed) r = keep ? leg_record_stop(r) : leg_record_reset();
                }
            }
        }
        for (const LegRecord &r : taps) printf("%d %u %u  ", (int)r.leg, r.left, r.written);
        printf("| %d\n", leg_record_any(taps.data(), max_taps) ? 1 : 0);
    }
    return 0;
}
