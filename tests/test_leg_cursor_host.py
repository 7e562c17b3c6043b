"""The per-leg cursor rule on the CPU (wmix_amd/csrc/leg_cursor.h): what wmx_mix_load_minus_legs applies on the device for every
leg and packet.  A small C++ driver, compiled with g++ against the header the kernel includes and linked with the oracle's
orc_load_data (oracle/orc_mix.c), drives both with the same sequences -- play heads that move by random amounts, legs that fall
behind and jump, legs that run ahead up to the overrun bound, a jump that lands on the ring's start -- for play_correct 0 and the
alsa value, rings of 16 000 and 64 000 bytes and random package sizes.  After every call the cursors are equal and the ring was
written from the start the rule names; beyond the bound the drop flag equals the rule as include/wmix_amd.h states it, computed from
the oracle's end cursor.  Sanitizer flags as tools_dev/san/Makefile sets them: a finding kills the driver and fails the test."""
import os
import subprocess

from conftest import ROOT

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "leg_cursor.h"
extern "C" {
#include "orc_mix.h"
}

using namespace wmx;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static long bad = 0, calls = 0, jumps = 0, jumps_to_start = 0, drops = 0, at_bound = 0, ahead = 0, spans = 0;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (bad < 10) fprintf(stderr, __VA_ARGS__);   \
            bad++;                                        \
        }                                                 \
    } while (0)

struct Bench {
    orc_mix_ring r;
    std::vector<uint8_t> store;
    std::vector<int16_t> src;
    Bench(int chn, int freq, uint32_t play_correct) : store((size_t)chn * 2 * freq + 64), src(40000, (int16_t)7) {
        orc_mix_ring_init(&r, store.data(), chn, freq);
        r.play_correct = play_correct;
    }
    LegMixState ms() const { return LegMixState{r.head_off, r.tick, r.play_correct, r.size}; }
    void play(uint32_t bytes) {  // the drain's bookkeeping (src/wmix.c:1347-1366)
        r.head_off = (r.head_off + bytes) % r.size;
        r.tick += bytes;
    }
    // one call of `bytes` source bytes (ring format: n_out = bytes / 2) through both; returns whether it was made
    bool call(LegCursor &c, uint32_t bytes, const char *what) {
        const uint32_t n_out = bytes / 2, samples = r.size / 2;
        int16_t *ring = (int16_t *)r.buff;
        const LegCall got = leg_cursor_call(ms(), n_out, c);
        uint32_t tk = c.tick;
        const uint32_t head = orc_load_data(&r, src.data(), bytes, (uint16_t)r.freq, (uint8_t)r.chn, 16, c.head, 1, &tk);
        const bool want_drop = (uint32_t)(tk - r.tick) > r.size;  // the end cursor more than one ring ahead of the mixer's tick
        calls++;
        CHECK(got.drop == want_drop, "%s: drop %d, the rule gives %d (end tick %u, mixer tick %u, ring %u)\n", what, (int)got.drop,
              (int)want_drop, tk, r.tick, r.size);
        if (want_drop) {
            drops++;
            CHECK(got.after.head == c.head && got.after.tick == c.tick, "%s: a dropped call moved the cursor\n", what);
            memset(r.buff, 0, r.size);  // the call is not made
            return false;
        }
        CHECK(got.after.head == head && got.after.tick == tk, "%s: cursor (%u, %u), the oracle's (%u, %u)\n", what, got.after.head,
              got.after.tick, head, tk);
        const bool jumped = c.head == UINT32_MAX || c.tick < r.tick;
        jumps += jumped;
        jumps_to_start += jumped && got.start == 0 && r.head_off + r.play_correct >= r.size;
        at_bound += (uint32_t)(tk - r.tick) == r.size;
        ahead += (uint32_t)(tk - r.tick) > r.size / 2;
        // the ring was written from the start the rule names, n_out samples, nowhere else at the edges
        CHECK(got.start < r.size && got.start % 2 == 0, "%s: start %u\n", what, got.start);
        if (got.start < r.size) {
            const uint32_t s0 = got.start / 2;
            CHECK(ring[s0] == 7 && ring[(s0 + n_out - 1) % samples] == 7, "%s: the span does not start at %u\n", what, got.start);
            if (n_out < samples)
                CHECK(ring[(s0 + n_out) % samples] == 0 && ring[(s0 + samples - 1) % samples] == 0, "%s: written outside the span\n", what);
            for (uint32_t i = 0; i < n_out; i++) ring[(s0 + i) % samples] = 0;
        }
        c = got.after;
        return true;
    }
    // one launch's worth: leg_cursor_span against the calls one by one
    void burst(LegCursor &c, uint32_t bytes, uint32_t valid, int max_packets, bool contiguous) {
        const LegSpan sp = leg_cursor_span(ms(), bytes / 2, c, valid, max_packets);
        uint32_t made = 0, slots = 0, dropped = 0, start = 0;
        bool stopped = false;
        for (int k = 0; k < max_packets; k++) {
            if (!((valid >> k) & 1u)) continue;
            if (stopped) {
                dropped++;
                continue;
            }
            const LegCall one = leg_cursor_call(ms(), bytes / 2, c);
            if (!call(c, bytes, "burst")) {
                stopped = true;
                dropped++;
                continue;
            }
            if (made == 0) start = one.start;
            if (contiguous) CHECK(one.start == (start + made * bytes) % r.size, "burst: call %u is not behind the one before\n", made);
            slots |= (uint32_t)k << (2 * made);
            made++;
        }
        spans++;
        CHECK(sp.count == made && sp.slots == slots && sp.dropped == dropped && (made == 0 || sp.start == start) && sp.after.head == c.head &&
                  sp.after.tick == c.tick,
              "burst: span (%u calls, slots %x, %u dropped), one by one (%u, %x, %u)\n", sp.count, sp.slots, sp.dropped, made, slots, dropped);
    }
};

static void random_run(int chn, int freq, uint32_t play_correct, uint32_t tick0, int steps) {
    Bench b(chn, freq, play_correct);
    b.r.tick = tick0;
    const int n_legs = 6;
    LegCursor leg[n_legs];
    for (LegCursor &c : leg) c = leg_cursor_fresh();
    const uint32_t frame = (uint32_t)chn * 2;
    for (int i = 0; i < steps; i++) {
        const uint32_t what = rnd() % 16;
        const uint32_t bytes = frame * (1 + rnd() % (rnd() % 4 ? 400 : 2000));  // package size: up to 800 bytes, now and then 4 000
        LegCursor &c = leg[rnd() % n_legs];
        if (what < 5) {
            b.play(frame * (rnd() % 200));          // the play head moves on a little
        } else if (what == 5) {
            b.play(frame * (rnd() % (b.r.size / frame)));  // ... or a long way: every leg is behind afterwards
        } else if (what == 6) {
            c = leg_cursor_fresh();                 // a new call in the slot
        } else if (what == 7) {
            for (int k = 0; k < 60; k++)            // a leg that runs ahead until the bound stops it
                if (!b.call(c, bytes, "ahead")) break;
        } else if (what < 11) {
            b.burst(c, bytes, rnd() % 16, 1 + (int)(rnd() % 4), tick0 < 0x80000000u);
        } else {
            b.call(c, bytes, "call");
        }
    }
}

int main() {
    const int formats[][2] = {{1, 8000}, {1, 32000}, {2, 16000}};  // rings of 16 000, 64 000 and 64 000 bytes
    for (const auto &f : formats) {
        const uint32_t size = (uint32_t)f[0] * 2 * f[1], alsa = (uint32_t)(f[0] * f[1] * 16 / 8 / 5);
        for (uint32_t pc : {0u, alsa}) {
            random_run(f[0], f[1], pc, 0, 20000);
            random_run(f[0], f[1], pc, 0xFFFF0000u, 4000);  // the mixer's tick wraps: the same uint32 arithmetic
            // a leg that runs ahead to exactly one ring in front of the mixer's tick: that call is made, the next is not
            Bench b(f[0], f[1], pc);
            LegCursor c = leg_cursor_fresh();
            const uint32_t pkg = size / 50;
            const long before = at_bound;
            int made = 0;
            while (b.call(c, pkg, "to the bound")) made++;
            CHECK(made == (int)((size - pc) / pkg) && at_bound == before + 1, "to the bound: %d calls made\n", made);
            // the leg falls behind while the head moves to where head + play_correct is the ring's end: it jumps to the ring's start
            b.play(size + size - pc - b.r.head_off % size);
            CHECK((b.r.head_off + pc) % size == 0, "head %u\n", b.r.head_off);
            const LegCall j = leg_cursor_call(b.ms(), pkg / 2, c);
            CHECK(!j.drop && j.start == (pc ? 0u : b.r.head_off) && j.after.head == (j.start + pkg) % size, "the jump starts at %u\n", j.start);
            b.call(c, pkg, "jump to the start");
        }
    }
    printf("%ld calls and %ld bursts, %ld differ; %ld jumps (%ld to the ring's start), %ld more than half a ring ahead, %ld at the bound, %ld dropped\n",
           calls, spans, bad, jumps, jumps_to_start, ahead, at_bound, drops);
    return bad ? 1 : 0;
}
"""

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Werror"]


def test_the_leg_cursor_rule_equals_the_oracles_load_data_call_by_call(tmp_path):
    src, obj, exe = tmp_path / "leg_cursor_driver.cpp", tmp_path / "orc_mix.o", tmp_path / "leg_cursor_driver"
    src.write_text(DRIVER)
    oracle = os.path.join(ROOT, "oracle")
    subprocess.check_call(["gcc", "-std=c99"] + SAN + ["-c", os.path.join(oracle, "orc_mix.c"), "-o", str(obj)])
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-Wno-unused-function", "-I" + os.path.join(ROOT, "wmix_amd", "csrc"), "-I" + oracle,
                                                         "-o", str(exe), str(src), str(obj)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert " 0 differ" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    # the sequences reached what they are for
    count = lambda tail: int(r.stdout.split(tail)[0].split()[-1].lstrip("("))  # noqa: E731
    assert count(" jumps") > 1000 and count(" to the ring's start") > 10 and count(" more than half") > 1000
    assert count(" at the bound") >= 6 and count(" dropped") > 100
