// leg_prompt_san.cpp -- the prompt rule of one leg of the bridge (leg_prompt_tick, wmix_amd/csrc/leg_prompt.h) as a stand-alone CPU
// program, for AddressSanitizer + UndefinedBehaviorSanitizer (tools_dev/san/Makefile).  No HIP, no GPU.
//
//   leg_prompt_san < cases      one case per line: samples repeat gap ticks stop_at head_off tick play_correct pos0
// A leg plays clip 0 of `samples` samples (repeat passes, gap ticks of pause) from tick 0 on a ring of 16 000 bytes whose play head
// starts at (head_off, tick); behind every tick the play thread drains 320 bytes.  stop_at >= 0: the leg is stopped in front of that
// tick.  pos0: the state's pos in front of tick 0 -- 0 is what a play leaves; anything else is a state no play makes (pos0 >= samples:
// one the clip table does not bear out, as when a clip fails the kernel's clamp against the arena).  One result line per tick: the call
// (n start from) and the state behind it (clip pos left done wait gap head tick).
#include <cstdint>
#include <cstdio>
#include "leg_prompt.h"

using namespace wmx;

int main() {
    unsigned samples, repeat, gap, head_off, tick, correct, pos0;
    int ticks, stop_at;
    while (scanf("%u %u %u %d %d %u %u %u %u", &samples, &repeat, &gap, &ticks, &stop_at, &head_off, &tick, &correct, &pos0) == 9) {
        BridgeMixState m{head_off, tick, correct, 16000u};
        LegPrompt p = leg_prompt_play(0, repeat, gap, leg_prompt_idle(0u).done);
        p.pos = pos0;
        for (int t = 0; t < ticks; t++) {
            if (t == stop_at) p = leg_prompt_idle(p.done);
            const PromptCall c = leg_prompt_tick(m, samples, p);
            printf("%u %u %u %d %u %u %u %u %u %u %u\n", c.n, c.start, c.from, (int)p.clip, p.pos, p.left, p.done, p.wait, p.gap, p.head, p.tick);
            m.head_off = (m.head_off + 320u) % m.ring_bytes;
            m.tick += 320u;
        }
    }
    return 0;
}
