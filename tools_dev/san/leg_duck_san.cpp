// leg_duck_san.cpp -- the duck of one leg of the bridge (leg_prompt_ducks beside leg_prompt_tick, wmix_amd/csrc/leg_prompt.h, REDUCE) as a
// stand-alone CPU program, for AddressSanitizer + UndefinedBehaviorSanitizer (tools_dev/san/Makefile).  No HIP, no GPU.
//
//   leg_duck_san < cases      one case per line: samples repeat gap reduce ticks stop_at again_at again_reduce head_off tick play_correct
// leg_prompt_san's leg, played with `reduce`.  stop_at >= 0: the leg is stopped in front of that tick.  again_at >= 0: in front of that
// tick the leg is played anew, the same clip, repeat and gap, with again_reduce.  One result line per tick: the divisor the tick's load
// of the legs applies (evaluated on the state as the tick finds it), the call (n start from), the state behind it (clip pos left done
// wait, the pause of gap, head tick, reduce) and the gap word as it lies in the entry.
#include <cstdint>
#include <cstdio>
#include "leg_prompt.h"

using namespace wmx;

int main() {
    unsigned samples, repeat, gap, reduce, again_reduce, head_off, tick, correct;
    int ticks, stop_at, again_at;
    while (scanf("%u %u %u %u %d %d %d %u %u %u %u", &samples, &repeat, &gap, &reduce, &ticks, &stop_at, &again_at, &again_reduce, &head_off, &tick,
                 &correct) == 11) {
        BridgeMixState m{head_off, tick, correct, 16000u};
        LegPrompt p = leg_prompt_play(0, repeat, gap, leg_prompt_idle(0u).done, reduce);
        for (int t = 0; t < ticks; t++) {
            if (t == stop_at) p = leg_prompt_idle(p.done);
            if (t == again_at) p = leg_prompt_play(0, repeat, gap, p.done, again_reduce);
            const uint32_t ducks = leg_prompt_ducks(p, samples);
            const PromptCall c = leg_prompt_tick(m, samples, p);
            printf("%u %u %u %u %d %u %u %u %u %u %u %u %u %u\n", ducks, c.n, c.start, c.from, (int)p.clip, p.pos, p.left, p.done, p.wait,
                   leg_prompt_gap(p), p.head, p.tick, leg_prompt_divisor(p) - 1u, p.gap);
            m.head_off = (m.head_off + 320u) % m.ring_bytes;
            m.tick += 320u;
        }
    }
    return 0;
}
