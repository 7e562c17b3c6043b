"""The duck of a leg under its prompt on the CPU (wmix_amd/csrc/leg_prompt.h, REDUCE: leg_prompt_ducks is what the legs' load evaluates
on the device per leg and tick).  tools_dev/san/leg_duck_san.cpp, a stand-alone program compiled with g++ against the header the kernel
includes and with AddressSanitizer + UndefinedBehaviorSanitizer, evaluates the header; tests/leg_duck_model.py, written from the rule's
text over tests/leg_prompt_model.py, is what it must equal, state for state and divisor for divisor, tick by tick.  Integers."""
import os
import subprocess

import pytest

from conftest import ROOT
from leg_duck_model import DuckPrompt
from leg_prompt_model import LegPrompt

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Werror",
       "-Wno-unused-function"]
CSRC = os.path.join(ROOT, "wmix_amd", "csrc")
RING, TICKS, STOP_AT = 16000, 40, 9
CLIPS, REPEATS, GAPS, REDUCES = (1, 160, 161, 800), (1, 3, 0), (0, 1, 7), (0, 1, 2, 15)
HEADS = ((0, 0, 3200), (15680, 640000, 3200))
# a play over a play, in front of this tick, with this reduce: into a pass and into a gap (800 samples, gap 7: ticks 5 .. 11 are the gap)
AGAIN = ((3, 5), (8, 0), (8, 3), (3, 0))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("leg_duck") / "leg_duck_san"
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tools_dev", "san", "leg_duck_san.cpp")])
    return str(exe)


def header(program, cases):
    """cases: (samples, repeat, gap, reduce, ticks, stop_at, again_at, again_reduce, head_off, tick, play_correct) -> per case, per
    tick, the fourteen integers"""
    text = "".join("%d %d %d %d %d %d %d %d %d %d %d\n" % c for c in cases)
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    lines = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(lines) == sum(c[4] for c in cases)
    out, at = [], 0
    for c in cases:
        out.append(lines[at:at + c[4]])
        at += c[4]
    return out


def model(samples, repeat, gap, reduce, ticks, stop_at, again_at, again_reduce, head_off, tick, correct, cls=DuckPrompt):
    """-> per tick (the divisor of the tick's load, n, start, from) + the state + (reduce,)"""
    p, out = cls(), []
    duck = cls is DuckPrompt
    p.play(0, repeat, gap, *((reduce,) if duck else ()))
    for t in range(ticks):
        if t == stop_at:
            p.stop()
        if t == again_at:
            p.play(0, repeat, gap, *((again_reduce,) if duck else ()))
        ducks = p.ducks(samples) if duck else 1
        call = p.step((head_off, tick, correct, RING), samples)
        n, at, start = (call[0], call[1], call[3]) if call else (0, 0, 0)
        out.append((ducks, n, start, at) + p.state() + ((p.reduce,) if duck else (0,)))
        head_off, tick = (head_off + 320) % RING, (tick + 320) & 0xFFFFFFFF
    return out


def cases():
    cs = [(s, r, g, d, TICKS, STOP_AT if r == 0 else -1, -1, 0) + h for s in CLIPS for r in REPEATS for g in GAPS for d in REDUCES for h in HEADS]
    cs += [(800, 3, 7, d, TICKS, -1, at, d2) + h for d in REDUCES for at, d2 in AGAIN for h in HEADS]
    cs += [(800, 3, 0, 2, TICKS, 7, -1, 0) + HEADS[0], (161, 0, 1, 15, TICKS, 4, -1, 0) + HEADS[1]]  # a stop in mid pass
    return cs


def test_the_header_equals_the_model_state_and_divisor(program):
    cs = cases()
    assert len(cs) == 4 * 3 * 3 * 4 * 2 + 4 * 4 * 2 + 2
    for case, got in zip(cs, header(program, cs)):
        want = model(*case)
        for t, (g, w) in enumerate(zip(got, want)):
            assert g[:13] == w, (case, "tick", t, g, w)
            # the entry's gap word: the pause below, reduce above, nothing else
            assert g[13] == g[9] | (g[12] << 16), (case, t, g)


def test_with_reduce_0_every_state_is_the_plain_models(program):
    """reduce 0 is the play there was before: the states, the gap word as it lies in the entry included, equal tests/leg_prompt_model.py's
    and no tick is ducked"""
    cs = [c for c in cases() if c[3] == 0 and c[7] == 0]
    assert len(cs) >= 4 * 3 * 3 * 2
    for case, got in zip(cs, header(program, cs)):
        want = model(*case, cls=LegPrompt)
        for t, (g, w) in enumerate(zip(got, want)):
            assert g[:13] == w and g[13] == w[9] and g[0] == 1, (case, t, g, w)


def test_what_the_cases_reach(program):
    """a tick is ducked exactly when the prompt makes a call in it and was played with reduce > 0, and then by reduce + 1: so the
    first tick behind a gap is ducked, no tick inside a gap is, none behind a stop or the end of the last pass is, and a play over a
    play ducks by the new divisor from its first tick on"""
    cs = cases()
    after_gap = in_gap = after_stop = after_end = replaced = 0
    for case, got in zip(cs, header(program, cs)):
        samples, repeat, gap, reduce, ticks, stop_at, again_at, again_reduce = case[:8]
        in_force, waited = reduce, 0
        for t, line in enumerate(got):
            if t == stop_at:
                in_force = 0
            if t == again_at:
                in_force = again_reduce
                replaced += line[0] == again_reduce + 1 > 1 and again_reduce != reduce
            ducks, n, state = line[0], line[1], line[4:]
            assert ducks == (in_force + 1 if n else 1), (case, t, line)
            if in_force and n == 0 and state[0] >= 0:
                in_gap += 1
                waited = 1
            if in_force and n and waited:
                after_gap += 1
                waited = 0
            after_stop += stop_at >= 0 and t >= stop_at and reduce > 0
            if state[0] < 0 and t != stop_at:
                in_force = 0
                after_end += reduce > 0 and ducks == 1
    assert min(after_gap, in_gap, after_stop, after_end, replaced) > 10, (after_gap, in_gap, after_stop, after_end, replaced)
