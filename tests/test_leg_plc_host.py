"""The bridge's concealment rule on the CPU (wmix_amd/csrc/leg_plc.h: what wmx_rtp_conceal_legs applies on the device per leg and tick).
tools_dev/san/leg_plc_san.cpp, a stand-alone program compiled with g++ against the header the kernel includes and with AddressSanitizer +
UndefinedBehaviorSanitizer, evaluates the header; tests/leg_plc_model.py, written from the rule's text, is what it must equal: known
answers, the program's built-in sweep, then a sweep of random (history, list, rows) cases -- emitted rows, d_len_out, history and
counter.  Integers, np.array_equal."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from leg_plc_model import BLEND, HIST, ROW, SHAPES, D, LegPlc, S, alaw_decode, audio, gen_case, pack, run_lengths, ulaw_decode, unpack

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Werror",
       "-Wno-unused-function"]
CSRC = os.path.join(ROOT, "wmix_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("leg_plc") / "leg_plc_san"
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tools_dev", "san", "leg_plc_san.cpp")])
    return str(exe)


def run(program, args, stdin=None):
    r = subprocess.run([program] + args, input=stdin, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    return r.stdout.splitlines()


def result(line):
    """a result line -> (count, len_out [4], concealed, history [320], emitted rows [count, 160])"""
    v = np.array(line.split(), np.int64)
    count = int(v[0])
    assert len(v) == 6 + HIST + count * ROW
    return count, v[1:5].astype(np.uint32), int(v[5]), v[6:6 + HIST].astype(np.int16), v[6 + HIST:].astype(np.int16).reshape(count, ROW)


def case_text(calls, rows, lens, hist):
    return "%d %d %s %s %s\n" % (len(lens), pack(calls), " ".join(map(str, lens)), " ".join(map(str, hist)), " ".join(map(str, rows[:, :ROW].ravel())))


def header(program, cases):
    """cases: (calls, rows [K, 160], lens [K], hist [320]) -> per case what result() returns"""
    return [result(line) for line in run(program, ["cases"], "".join(case_text(*c) for c in cases))]


def model(calls, rows, lens, hist):
    leg = LegPlc(hist)
    out, len_out = leg.tick(rows, lens, calls)
    return len(calls), len_out, leg.concealed, leg.hist.astype(np.int16), out[:len(calls)], leg.lags


def same(got, want, what):
    assert got[0] == want[0] and got[2] == want[2], (what, "count / concealed", got[0], got[2], want[0], want[2])
    assert np.array_equal(got[1], want[1]), (what, "d_len_out", got[1], want[1])
    assert np.array_equal(got[4], want[4]), (what, "rows", np.argwhere(got[4] != want[4])[:6])
    assert np.array_equal(got[3], want[3]), (what, "history", np.flatnonzero(got[3] != want[3])[:6])


def tiled(period, n=HIST, seed=3):
    """-> (n samples, exactly periodic, that end with a whole period; the period): one period of integers, tiled"""
    one = np.random.default_rng(seed).integers(-20000, 20000, size=period).astype(np.int16)
    return np.tile(one, n // period + 1)[-n:], one


def gain(k):
    return np.maximum(0, 32768 - 68 * np.asarray(k, np.int64))


def test_a_period_of_50_gives_lag_50_and_its_tiled_continuation(program):
    hist, one = tiled(50)
    x = np.random.default_rng(4).integers(-30000, 30000, size=(1, ROW)).astype(np.int16)
    case = ([S, D(0)], x, np.array([320], np.uint32), hist)
    got, want = header(program, [case])[0], model(*case)
    same(got, want, "S D")
    assert want[5] == [50]  # 50 and 100 score alike: the smaller lag
    k = np.arange(ROW + BLEND, dtype=np.int64)
    cont = (np.tile(one, 4)[:ROW + BLEND].astype(np.int64) * gain(k)) >> 15
    assert np.array_equal(got[4][0], cont[:ROW].astype(np.int16)) and got[2] == 1
    i = np.arange(BLEND, dtype=np.int64)
    assert np.array_equal(got[4][1][:BLEND], ((x[0, :BLEND].astype(np.int64) * i + cont[ROW:] * (BLEND - i)) >> 5).astype(np.int16))
    assert np.array_equal(got[4][1][BLEND:], x[0, BLEND:])
    assert np.array_equal(got[3], np.concatenate([got[4][0], got[4][1]]))


def test_an_all_zero_history_gives_zeros(program):
    x = alaw_decode(np.arange(160) % 256).reshape(1, ROW)
    case = ([S, S, D(0)], x, np.array([320], np.uint32), np.zeros(HIST, np.int16))
    got, want = header(program, [case])[0], model(*case)
    same(got, want, "S S D on zeros")
    assert want[5] == [40] and not got[4][:2].any() and got[2] == 2
    i = np.arange(BLEND, dtype=np.int64)
    assert np.array_equal(got[4][2][:BLEND], ((x[0, :BLEND].astype(np.int64) * i) >> 5).astype(np.int16)) and np.array_equal(got[4][2][BLEND:], x[0, BLEND:])


def test_a_run_of_three_uses_one_lag_and_k_counts_through(program):
    hist, one = tiled(64)
    x = ulaw_decode(np.arange(160) % 256).reshape(1, ROW)
    case = ([S, S, S, D(0)], x, np.array([320], np.uint32), hist)
    got, want = header(program, [case])[0], model(*case)
    same(got, want, "S S S D")
    assert want[5] == [64] and got[2] == 3
    k = np.arange(3 * ROW + BLEND, dtype=np.int64)
    cont = (np.tile(one, 9)[:3 * ROW + BLEND].astype(np.int64) * gain(k)) >> 15
    assert np.array_equal(got[4][:3].ravel(), cont[:3 * ROW].astype(np.int16)) and got[4][2].any()
    assert gain(481) > 0 and gain(482) == 0  # the gain runs out just behind the longest run
    i = np.arange(BLEND, dtype=np.int64)
    assert np.array_equal(got[4][3][:BLEND], ((x[0, :BLEND].astype(np.int64) * i + cont[3 * ROW:] * (BLEND - i)) >> 5).astype(np.int16))
    assert np.array_equal(got[4][3][BLEND:], x[0, BLEND:])


def test_a_second_run_re_estimates_its_lag_from_what_the_first_run_left(program):
    hist, _ = tiled(50)
    # the packet between the runs has another period than the concealed row in front of it: the second run sees both
    x = np.stack([tiled(83, ROW, seed=9)[0], np.zeros(ROW, np.int16)])
    case = ([S, D(0), S, D(1)], x, np.array([320, 320], np.uint32), hist)
    got, want = header(program, [case])[0], model(*case)
    same(got, want, "S D S D")
    assert len(want[5]) == 2 and want[5][0] == 50 and want[5][1] != 50 and got[2] == 2
    # the second run's history is the first run's output: its synthesis starts from row 1 as emitted
    lag = want[5][1]
    h0 = np.concatenate([got[4][0], got[4][1]]).astype(np.int64)
    k = np.arange(ROW, dtype=np.int64)
    assert np.array_equal(got[4][2], ((h0[HIST - lag + k % lag] * gain(k)) >> 15).astype(np.int16))


def test_the_built_in_sweep_equals_the_model(program):
    lines = run(program, [])
    assert len(lines) == 2 * 8 * 31 and all(line.startswith("in ") for line in lines[0::2])
    for given, line in zip(lines[0::2], lines[1::2]):
        v = np.array(given.split()[1:], np.int64)
        k, word = int(v[0]), int(v[1])
        lens, hist, rows = v[2:2 + k].astype(np.uint32), v[2 + k:2 + k + HIST].astype(np.int16), v[2 + k + HIST:].astype(np.int16).reshape(k, ROW)
        same(result(line), model(unpack(word), rows, lens, hist), ("built in", word, hist[:4]))


def test_every_case_of_the_random_sweep_equals_the_model(program):
    rng = np.random.default_rng(2026)
    cases, runs, shapes, unreadable = [], {1: 0, 2: 0, 3: 0}, dict.fromkeys(SHAPES, 0), 0
    for n in range(2400):
        k = int(rng.integers(1, 5))
        shape = SHAPES[n % len(SHAPES)]
        calls, rows, lens = gen_case(rng, k, shape)
        hist = audio(rng, HIST) if rng.integers(0, 8) else np.zeros(HIST, np.int16)
        cases.append((calls, rows, lens, hist))
        shapes[shape] += 1
        unreadable += any(kind == "D" and (s >= k or lens[s] != 320) for kind, s in calls)
        for r in run_lengths(calls, lens):
            runs[min(r, 3)] += 1
    assert all(v >= 200 for v in shapes.values()) and unreadable >= 100, (shapes, unreadable)
    assert all(v >= 100 for v in runs.values()), runs
    got = header(program, cases)
    assert len(got) == len(cases) >= 2000
    concealed = 0
    for n, (case, g) in enumerate(zip(cases, got)):
        want = model(*case)
        same(g, want, ("case", n, case[0]))
        concealed += want[2]
    assert concealed > 1000
