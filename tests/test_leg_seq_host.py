"""The bridge's sequence rule on the CPU (wmix_amd/csrc/leg_seq.h: what wmx_rtp_sequence_legs applies on the device per leg and tick)
and the cursor rule over a call list (leg_cursor_span_calls, wmix_amd/csrc/leg_cursor.h).  tools_dev/san/leg_seq_san.cpp, a stand-alone
program compiled with g++ against the headers the kernels include and with AddressSanitizer + UndefinedBehaviorSanitizer, evaluates the
header; tests/leg_seq_model.py, written from the rule's text, is what it must equal: known answers, then every case of a sweep over
four slots -- call list, the slots discarded (the rewritten d_len), state and counters."""
import itertools
import os
import subprocess

import pytest

from conftest import ROOT
from leg_seq_model import LegSeq, pack

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Werror",
       "-Wno-unused-function"]
CSRC = os.path.join(ROOT, "wmix_amd", "csrc")
OFFSETS = [-17, -16, -2, -1, 0, 1, 2, 3, 4, 5, 40000]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("leg_seq") / "leg_seq_san"
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tools_dev", "san", "leg_seq_san.cpp")])
    return str(exe)


def run(program, args, stdin=None):
    r = subprocess.run([program] + args, input=stdin, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    return [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]


def header(program, cases):
    """cases: (max_gap, synced, next, [s0 .. s3 or None]) -> per case (calls, discard mask, synced, next, lost, late, dup, resync, overflow)"""
    text = "".join("%d %d %d %s\n" % (g, sy, nx, " ".join(str(-1 if s is None else s) for s in (list(sl) + [None] * 4)[:4])) for g, sy, nx, sl in cases)
    return run(program, ["cases"], text)


def model(max_gap, synced, nxt, slots):
    leg = LegSeq(synced, nxt)
    calls, gone = leg.tick(list(slots), max_gap)
    return (pack(calls), sum(1 << k for k in gone)) + leg.state()


D, S = (lambda k: ("D", k)), ("S", None)
#        max_gap synced next  slots                 calls                 next after  counters                          slots discarded
KNOWN = [
    (3, 1, 10, [10, 11, None, None], [D(0), D(1)], 12, {}, []),
    (3, 1, 10, [11, 10], [D(1), D(0)], 12, {}, []),
    (3, 1, 10, [10, 10], [D(0)], 11, {"dup": 1}, [1]),
    (3, 1, 10, [12], [S, S, D(0)], 13, {"lost": 2}, []),
    (3, 1, 10, [9], [], 10, {"late": 1}, [0]),
    (3, 1, 10, [14], [D(0)], 15, {"resync": 1}, []),
    (3, 1, 10, [13, 14], [S, S, S, D(0)], 14, {"lost": 3, "overflow": 1}, [1]),
    (3, 1, 10, [10, 500], [D(0), D(1)], 501, {"resync": 1}, []),
    (3, 1, 10, [65000], [D(0)], 65001, {"resync": 1}, []),
    (3, 1, 10, [65529], [D(0)], 65530, {"resync": 1}, []),  # 17 back: not late
    (3, 1, 65535, [0, 65535], [D(1), D(0)], 1, {}, []),
    (3, 0, 0, [None, 500, 499], [D(1)], 501, {"late": 1}, [2]),
    (0, 1, 10, [12], [D(0)], 13, {"resync": 1}, []),
]


def test_known_answers(program):
    got = header(program, [(g, sy, nx, sl) for g, sy, nx, sl, _, _, _, _ in KNOWN])
    for (g, sy, nx, sl, calls, after, counters, gone), row in zip(KNOWN, got):
        want = (pack(calls), sum(1 << k for k in gone), 1, after) + tuple(counters.get(c, 0) for c in ("lost", "late", "dup", "resync", "overflow"))
        assert row == want, (sl, "max_gap", g, "next", nx, "header", row, "table", want)
        assert model(g, sy, nx, (sl + [None] * 4)[:4]) == want, (sl, "the model")


def test_no_slot_ok_is_no_call_and_no_change(program):
    assert header(program, [(3, 0, 77, []), (3, 1, 77, [None] * 4)]) == [(0, 0, 0, 77, 0, 0, 0, 0, 0), (0, 0, 1, 77, 0, 0, 0, 0, 0)]


def test_every_case_of_the_sweep_equals_the_model(program):
    got = run(program, [])
    options = [None] + OFFSETS
    n, kinds = 0, dict.fromkeys(("lost", "late", "dup", "resync", "overflow"), 0)
    for max_gap in range(4):
        for synced in (0, 1):
            for nxt in (0, 65534):
                for pick in itertools.product(options, repeat=4):
                    slots = [None if o is None else (nxt + o) % 65536 for o in pick]
                    want = model(max_gap, synced, nxt, slots)
                    assert got[n] == want, ("max_gap", max_gap, "synced", synced, "next", nxt, "slots", slots, "header", got[n], "model", want)
                    for i, c in enumerate(kinds):
                        kinds[c] += want[4 + i] > 0
                    n += 1
    assert n == len(got) == 4 * 2 * 2 * 12 ** 4
    assert all(v > 1000 for v in kinds.values()), kinds  # the sweep reaches every counter


SPAN_DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include "leg_cursor.h"
using namespace wmx;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
int main() {
    long bad = 0, spans = 0, jumps = 0, drops = 0, partial = 0;
    const uint32_t rings[] = {16000u, 64000u};
    for (uint32_t ring : rings)
        for (uint32_t pc : {0u, ring / 5}) {
            LegMixState ms{0u, rnd() % 2 ? 0u : 0xFFFF0000u, pc, ring};
            LegCursor leg[6];
            for (LegCursor &c : leg) c = leg_cursor_fresh();
            for (int i = 0; i < 40000; i++) {
                const uint32_t what = rnd() % 8, n_out = 1 + rnd() % (rnd() % 4 ? 400 : 2000);
                LegCursor &c = leg[rnd() % 6];
                if (what < 3) {  // the play head moves on a little, or a long way
                    const uint32_t bytes = 2 * (what == 0 ? rnd() % (ring / 2) : rnd() % 200);
                    ms.head_off = (ms.head_off + bytes) % ring;
                    ms.tick += bytes;
                    continue;
                }
                if (what == 3) {
                    c = leg_cursor_fresh();
                    continue;
                }
                // every valid slot in slot order, no silence: the list leg_cursor_span walks
                const int max_packets = 1 + (int)(rnd() % 4);
                const uint32_t valid = rnd() % 16;
                uint32_t calls = 0, n = 0;
                for (int k = 0; k < max_packets; k++)
                    if ((valid >> k) & 1u) calls |= (uint32_t)k << (4 + 4 * n), n++;
                calls |= n;
                const LegSpan a = leg_cursor_span(ms, n_out, c, valid, max_packets);
                const LegSpanCalls b = leg_cursor_span_calls(ms, n_out, c, calls);
                spans++;
                jumps += n && (c.head == UINT32_MAX || c.tick < ms.tick);
                drops += a.dropped > 0;
                partial += a.dropped > 0 && a.count > 0;
                if (a.count != b.span.count || a.slots != b.span.slots || a.dropped != b.span.dropped || (a.count && a.start != b.span.start) ||
                    a.after.head != b.span.after.head || a.after.tick != b.span.after.tick || b.silence != 0u) {
                    if (bad++ < 10) fprintf(stderr, "valid %x of %d: span (%u, %x, %u), calls (%u, %x, %u)\n", valid, max_packets, a.count, a.slots,
                                            a.dropped, b.span.count, b.span.slots, b.span.dropped);
                }
                // a list with silence in it moves the cursor like the same number of data calls, and reports which were silent
                const uint32_t mask = rnd() % 16;
                uint32_t with = calls;
                for (uint32_t j = 0; j < n; j++)
                    if ((mask >> j) & 1u) with |= 1u << (6 + 4 * j);
                const LegSpanCalls s = leg_cursor_span_calls(ms, n_out, c, with);
                if (s.span.count != a.count || s.span.dropped != a.dropped || s.span.after.head != a.after.head || s.span.after.tick != a.after.tick ||
                    s.silence != (mask & ((1u << a.count) - 1u)) || s.span.slots != a.slots)
                    bad++;
                c = a.after;
            }
        }
    printf("%ld spans, %ld differ; %ld jumps, %ld dropped, %ld of them in part\n", spans, bad, jumps, drops, partial);
    return bad ? 1 : 0;
}
"""


def test_span_calls_on_the_valid_slots_in_slot_order_is_leg_cursor_span(tmp_path):
    src, exe = tmp_path / "span_calls_driver.cpp", tmp_path / "span_calls_driver"
    src.write_text(SPAN_DRIVER)
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-I" + CSRC, "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert " 0 differ" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    count = lambda tail: int(r.stdout.split(tail)[0].split()[-1])  # noqa: E731
    assert count(" spans") > 50000 and count(" jumps") > 1000 and count(" dropped") > 100 and count(" of them in part") > 20
