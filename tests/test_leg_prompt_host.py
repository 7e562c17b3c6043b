"""The bridge's prompt rule on the CPU (wmix_amd/csrc/leg_prompt.h: what wmx_mix_load_prompts applies on the device per leg and tick).
tools_dev/san/leg_prompt_san.cpp, a stand-alone program compiled with g++ against the header the kernel includes and with
AddressSanitizer + UndefinedBehaviorSanitizer, evaluates the header; tests/leg_prompt_model.py, written from the rule's text, is what it
must equal, state for state and call for call, tick by tick.  Integers."""
import os
import subprocess

import pytest

from conftest import ROOT
from leg_prompt_model import NULL_HEAD, ROW, LegPrompt

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Werror",
       "-Wno-unused-function"]
CSRC = os.path.join(ROOT, "wmix_amd", "csrc")
RING = 16000
CLIPS, REPEATS, GAPS, TICKS = (1, 159, 160, 161, 477, 8037), (1, 3, 0), (0, 1, 7), 130
STOP_AT = 123  # an endless prompt is stopped here; 8037 samples are 51 ticks, so its third pass is cut
# where the play head stands at tick 0: the ring's start; near its end, so that head + play_correct lies behind it; and a tick counter
# about to wrap.  play_correct: the platform's 200 ms, and 0
HEADS = ((0, 0, 3200), (15680, 640000, 3200), (4800, 0xFFFFFFFF - 5000, 3200), (320, 320, 0))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("leg_prompt") / "leg_prompt_san"
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tools_dev", "san", "leg_prompt_san.cpp")])
    return str(exe)


def header(program, cases):
    """cases: (samples, repeat, gap, ticks, stop_at, head_off, tick, play_correct, pos0) -> per case, per tick, the eleven integers"""
    text = "".join("%d %d %d %d %d %d %d %d %d\n" % c for c in cases)
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    lines = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(lines) == sum(c[3] for c in cases)
    out, at = [], 0
    for c in cases:
        out.append(lines[at:at + c[3]])
        at += c[3]
    return out


def model(samples, repeat, gap, ticks, stop_at, head_off, tick, correct, pos0=0):
    p, out = LegPrompt(), []
    p.play(0, repeat, gap)
    p.pos = pos0
    for t in range(ticks):
        if t == stop_at:
            p.stop()
        call = p.step((head_off, tick, correct, RING), samples)
        n, at, start = (call[0], call[1], call[3]) if call else (0, 0, 0)
        out.append((n, start, at) + p.state())
        head_off, tick = (head_off + 320) % RING, (tick + 320) & 0xFFFFFFFF
    return out


def cases():
    return [(s, r, g, TICKS, STOP_AT if r == 0 else -1) + h + (0,) for s in CLIPS for r in REPEATS for g in GAPS for h in HEADS]


def test_the_header_equals_the_model_state_for_state(program):
    cs = cases()
    assert TICKS >= 120 and len(cs) == 6 * 3 * 3 * len(HEADS)
    for case, got in zip(cs, header(program, cs)):
        want = model(*case)
        for t, (g, w) in enumerate(zip(got, want)):
            assert g == w, (case, "tick", t, g, w)


def test_what_the_cases_reach(program):
    """the sweep is only worth its name if it meets every arm of the rule: waits, passes that end, prompts that end, an endless one that
    is stopped, no call that ends more than a ring ahead of the play head -- and the reference's reset behind every pass: at every
    play_correct (3 200, the handle's default, above all) and every gap (0, 1 and 7 alike) the first call of EVERY pass starts at
    head + play_correct, so the pause between two passes is the gap and not what the lead of the pass before leaves of it; inside a
    pass the cursor is kept"""
    cs = cases()
    jumps = waits = ends = stopped = kept = later_passes = 0
    for case, got in zip(cs, header(program, cs)):
        samples, repeat, gap, ticks, stop_at, head_off, tick, correct, _ = case
        wraps = tick + 320 * ticks + RING >= 1 << 32  # the reference's plain uint32 comparison misjudges a cursor there: its quirk
        before = (0, 0, repeat, 0, 0, gap, NULL_HEAD, 0)
        calls = 0
        for t, line in enumerate(got):
            n, start, at, state = line[0], line[1], line[2], line[3:]
            mix_tick = (tick + 320 * t) & 0xFFFFFFFF
            if n:
                calls += 1
                assert n == min(ROW, samples - at) and 0 <= start < RING and start % 2 == 0
                handed = before[6:8]
                jumped = handed[0] == NULL_HEAD or handed[1] < mix_tick  # the reference's own comparison, in uint32
                ahead = (head_off + 320 * t) % RING + correct
                if at == 0:  # the first call of a pass, the first pass or a later one: a fresh cursor
                    assert handed == (NULL_HEAD, 0) and start == (ahead if ahead < RING else 0), (case, t, handed, start)
                    jumps += 1
                    later_passes += t > 0 and correct == 3200 and gap in (1, 7)
                elif not wraps:  # inside a pass the lead is kept: no jump
                    assert not jumped and start == handed[0], (case, t, handed, start)
                    kept += 1
                if state[0] >= 0 and state[6] != NULL_HEAD and not wraps:
                    ahead = (state[7] - mix_tick) & 0xFFFFFFFF
                    assert ahead <= correct + 320 <= RING, "the lap rule would fire"
            waits += before[4] > 0 and t != stop_at
            if before[4] > 0 and t != stop_at:
                assert n == 0 and state[4] == before[4] - 1
            ends += state[3] > before[3]
            stopped += t == stop_at and before[0] == 0
            before = state
        last = got[-1][3:]
        if repeat:
            passes_ticks = repeat * ((samples + ROW - 1) // ROW) + (repeat - 1) * gap
            if passes_ticks <= ticks:
                assert last[0] == -1 and last[3] == 1 and calls == repeat * ((samples + ROW - 1) // ROW)
            else:  # three passes of 51 ticks: still in its third
                assert last[0] == 0 and last[3] == 0 and last[2] == 1
        else:
            assert last[0] == -1 and last[3] == 0
    assert min(jumps, waits, ends, stopped, kept, later_passes) > 50, (jumps, waits, ends, stopped, kept, later_passes)


def test_a_state_the_table_does_not_bear_out_goes_idle(program):
    """pos >= samples is the arm that protects the kernel when a clip fails its clamp against the arena (it then has no samples): the
    header goes idle without a call and without counting a prompt, as the model does; a pos inside the clip that no play left plays on
    from there"""
    cs = [(477, 2, 3, 6, -1, 0, 0, 3200, pos0) for pos0 in (477, 478, 500, 0xFFFFFFFF)]
    cs += [(0, r, g, 6, -1, 320, 320, 3200, pos0) for r in (0, 1, 3) for g in (0, 7) for pos0 in (0, 1, 160)]  # a clip of no samples
    inside = [(477, 2, 1, 12, -1, 0, 0, 3200, pos0) for pos0 in (1, 159, 320, 476)]
    got = header(program, cs + inside)
    for case, lines in zip(cs + inside, got):
        assert lines == model(*case), case
    for lines in got[:len(cs)]:
        assert all(line == (0, 0, 0, -1, 0, 0, 0, 0, 0, NULL_HEAD, 0) for line in lines)
    for case, lines in zip(inside, got[len(cs):]):
        assert lines[0][:3] == (min(ROW, 477 - case[8]), 3200, case[8]) and lines[-1][3] == -1 and lines[-1][6] == 1
