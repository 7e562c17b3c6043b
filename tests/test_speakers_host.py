"""The talker-selection rule on the CPU (wmix_amd/csrc/speakers.h, what mix.hip's selection kernel calls from its lanes): a stand-alone
C++ driver around speakers_step, built with g++ -- plain, and with the address and undefined-behaviour sanitizers -- replays scenarios
written by this file, and every tick's env / speaking / mute_out must equal the numpy model of tests/speakers_model.py.  Random layouts,
and the hand-made cases whose outcome is also asserted by value."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from speakers_model import SpeakersModel, level_of, row_of_level

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#include "speakers.h"

// scenario file: n_groups n_ticks, then per tick: max floor shift n_el n_conf has_mute n_reset | reset rings | per conference: n, rings |
// [mute by ring] | rows by ring.  Prints per tick: env by ring, speaking by ring, mute_out by ring.
int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    int n_groups = 0, n_ticks = 0;
    if (!f || fscanf(f, "%d %d", &n_groups, &n_ticks) != 2) return 2;
    std::vector<uint32_t> env((size_t)n_groups, 0);
    std::vector<uint8_t> speaking((size_t)n_groups), mute_out((size_t)n_groups), mute((size_t)n_groups);
    for (int t = 0; t < n_ticks; t++) {
        int max_speakers, shift, n_el, n_conf, has_mute, n_reset;
        unsigned floor;
        if (fscanf(f, "%d %u %d %d %d %d %d", &max_speakers, &floor, &shift, &n_el, &n_conf, &has_mute, &n_reset) != 7) return 3;
        if (!wmx::speakers_params_ok(max_speakers, shift) || !wmx::speakers_len_ok(2u * (unsigned)n_el)) return 4;
        for (int i = 0; i < n_reset; i++) {
            int r;
            if (fscanf(f, "%d", &r) != 1) return 3;
            env[(size_t)r] = 0;
        }
        std::vector<int32_t> off(1, 0), members;
        for (int c = 0; c < n_conf; c++) {
            int n;
            if (fscanf(f, "%d", &n) != 1) return 3;
            for (int i = 0; i < n; i++) {
                int r;
                if (fscanf(f, "%d", &r) != 1) return 3;
                members.push_back(r);
            }
            off.push_back((int32_t)members.size());
        }
        for (int r = 0; r < n_groups && has_mute; r++) {
            int v;
            if (fscanf(f, "%d", &v) != 1) return 3;
            mute[(size_t)r] = (uint8_t)v;
        }
        std::vector<int16_t> rows((size_t)n_groups * n_el);  // exactly the rows: a read past one is the sanitizer's to find
        for (auto &x : rows) {
            int v;
            if (fscanf(f, "%d", &v) != 1) return 3;
            x = (int16_t)v;
        }
        wmx::speakers_step(n_groups, n_conf, off.data(), members.data(), rows.data(), n_el, (uint32_t)n_el, has_mute ? mute.data() : nullptr,
                           max_speakers, floor, shift, env.data(), speaking.data(), mute_out.data());
        for (int r = 0; r < n_groups; r++) printf("%u ", env[(size_t)r]);
        for (int r = 0; r < n_groups; r++) printf("%d ", speaking[(size_t)r]);
        for (int r = 0; r < n_groups; r++) printf("%d ", mute_out[(size_t)r]);
        printf("\n");
    }
    // the bounds the entry points check with
    if (wmx::speakers_params_ok(0, 3) || wmx::speakers_params_ok(33, 3) || wmx::speakers_params_ok(1, -1) || wmx::speakers_params_ok(1, 32)) return 5;
    if (!wmx::speakers_params_ok(1, 0) || !wmx::speakers_params_ok(32, 31)) return 5;
    if (!wmx::speakers_len_ok(2 * 131071u) || wmx::speakers_len_ok(2 * 131072u)) return 5;
    if (wmx::speakers_abs16(INT16_MIN) != 32768u || 131071ull * 32768ull > UINT32_MAX || 131072ull * 32768ull <= UINT32_MAX) return 5;
    printf("done\n");
    return 0;
}
"""

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module", params=[["-O2"], SAN], ids=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("speakers")
    src = d / "speakers_driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function"] + request.param +
                          ["-I" + os.path.join(ROOT, "wmix_amd", "csrc"), "-o", str(exe), str(src)])
    count = [0]

    def run(n_groups, ticks):
        """ticks: dicts(layout, rows [n_groups, n_el] int16, max, floor, shift, mute=None, reset=()) -> per tick (env, speaking, mute_out),
        after asserting that the header and the model agree on every tick"""
        lines = ["%d %d" % (n_groups, len(ticks))]
        for tk in ticks:
            rows = np.asarray(tk["rows"], np.int16)
            assert rows.shape[0] == n_groups
            mute, reset = tk.get("mute"), list(tk.get("reset", ()))
            lines.append("%d %d %d %d %d %d %d" % (tk["max"], tk["floor"], tk["shift"], rows.shape[1], len(tk["layout"]), mute is not None, len(reset)))
            lines.append(" ".join(map(str, reset)))
            for mem in tk["layout"]:
                lines.append(" ".join(map(str, [len(mem)] + list(mem))))
            if mute is not None:
                lines.append(" ".join(str(int(v)) for v in mute))
            lines.append(" ".join(map(str, rows.reshape(-1).tolist())))
        count[0] += 1
        path = d / ("scenario_%d.txt" % count[0])
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        out = r.stdout.strip().splitlines()
        assert out[-1] == "done" and len(out) == len(ticks) + 1
        model, res = SpeakersModel(n_groups), []
        for t, tk in enumerate(ticks):
            got = np.array(out[t].split(), dtype=np.int64).reshape(3, n_groups)
            model.reset(tk.get("reset", ()))
            sp, mo = model.step(tk["layout"], tk["rows"], tk["max"], tk["floor"], tk["shift"], tk.get("mute"))
            assert np.array_equal(got[0], model.env.astype(np.int64)), ("env, tick", t)
            assert np.array_equal(got[1], sp) and np.array_equal(got[2], mo), ("speaking, tick", t)
            assert np.array_equal(got[1] + got[2], np.ones(n_groups, np.int64))
            res.append((got[0].copy(), got[1].copy(), got[2].copy()))
        return res

    return run


E = 16  # elements per row in the hand-made cases


def rows_of(levels, n_el=E):
    return np.stack([row_of_level(int(v), n_el) for v in levels])


def tick(layout, levels, mx, floor=0, shift=3, mute=None, reset=(), n_el=E):
    return dict(layout=layout, rows=rows_of(levels, n_el), max=mx, floor=floor, shift=shift, mute=mute, reset=reset)


def random_layout(rng, n_groups):
    rings = rng.permutation(n_groups).tolist()
    layout = []
    while rings and len(layout) < 12:
        n = int(rng.choice([0, 1, 2, 2, 3, 4, 5, 8, 9, 17, 32]))
        n = min(n, len(rings))
        layout.append([rings.pop() for _ in range(n)])
    return layout


def test_random_layouts(driver):
    rng = np.random.default_rng(31)
    n_groups = 90
    for n_el in (1, 7, 160):
        ticks, layout = [], random_layout(rng, n_groups)
        for t in range(10):
            if t in (4, 7):
                layout = random_layout(rng, n_groups)
            rows = rng.integers(-32768, 32768, size=(n_groups, n_el)).astype(np.int16)
            rows[rng.random(n_groups) < 0.3] = 0             # silent legs: ties at the held envelope and at 0
            rows[rng.random(n_groups) < 0.2] >>= 6
            mute = (rng.random(n_groups) < 0.15).astype(np.uint8) if t % 3 else None
            level_pool = [level_of(r) for r in rows]
            ticks.append(dict(layout=layout, rows=rows, max=int(rng.integers(1, 33)), floor=int(rng.choice([0, 1, sorted(level_pool)[n_groups // 2], 1 << 31])),
                              shift=int(rng.integers(0, 32)), mute=mute, reset=rng.choice(n_groups, 3, replace=False).tolist() if t == 5 else ()))
        res = driver(n_groups, ticks)
        assert any(sp.any() for _, sp, _ in res) and any(not sp.all() for _, sp, _ in res)


def test_a_tie_goes_to_the_earlier_list_position_not_the_lower_ring(driver):
    (env, sp, mo), = driver(6, [tick([[5, 2]], [0, 0, 700, 0, 0, 700], 1)])
    assert sp.tolist() == [0, 0, 0, 0, 0, 1] and mo.tolist() == [1, 1, 1, 1, 1, 0] and env[5] == env[2] == 700


def test_an_envelope_equal_to_the_floor_is_eligible(driver):
    (env, sp, _), = driver(2, [tick([[0, 1]], [100, 99], 2, floor=100)])
    assert sp.tolist() == [1, 0] and env.tolist() == [100, 99]


def test_floor_zero_and_silence_choose_the_first_by_list_order(driver):
    (env, sp, _), = driver(6, [tick([[4, 0, 3, 1, 5]], [0] * 6, 2, floor=0)])
    assert sp.tolist() == [1, 0, 0, 0, 1, 0] and not env.any()


def test_a_row_of_minus_32768(driver):
    rows = np.zeros((2, 160), np.int16)
    rows[0] = -32768
    rows[1] = 32767
    (env, sp, _), = driver(2, [dict(layout=[[1, 0]], rows=rows, max=1, floor=0, shift=3)])
    assert env.tolist() == [160 * 32768, 160 * 32767] and sp.tolist() == [1, 0]


def test_decay_shift_0_holds_nothing_and_31_nearly_everything(driver):
    for shift, held in ((0, 0), (31, 5000), (1, 2500)):
        res = driver(2, [tick([[0, 1]], [5000, 10], 1, shift=shift), tick([[0, 1]], [0, 10], 1, shift=shift)])
        assert res[1][0].tolist() == [held, 10] and res[1][1].tolist() == ([1, 0] if held > 10 else [0, 1])
    big = 3 << 30  # above 2^31 a shift of 31 takes 1 off
    res = driver(2, [dict(layout=[[0, 1]], rows=np.full((2, 98304), -32768, np.int16), max=2, floor=0, shift=31),
                     dict(layout=[[0, 1]], rows=np.zeros((2, 98304), np.int16), max=2, floor=0, shift=31)])
    assert res[0][0].tolist() == [big, big] and res[1][0].tolist() == [big - 1, big - 1]


def test_a_talker_that_falls_silent_is_held_and_then_dropped_on_the_tick_the_decay_says(driver):
    ticks = [tick([[0, 1, 2]], [8000 if t == 0 else 0, 3000, 5], 1, shift=3) for t in range(14)]
    res = driver(3, ticks)
    e, drop = 8000, None
    for t in range(1, 14):
        e -= e >> 3
        assert res[t][0][0] == e
        if drop is None and e < 3000:  # at 3 000 exactly position 0 would still win the tie
            drop = t
    assert drop == 8
    for t in range(14):
        assert res[t][1].tolist() == ([1, 0, 0] if t < drop else [0, 1, 0]), t


def test_a_host_muted_loudest_leg_never_speaks_but_its_envelope_is_tracked(driver):
    mute = np.array([0, 1, 0], np.uint8)
    res = driver(3, [tick([[0, 1, 2]], [40, 9000, 30], 1, mute=mute), tick([[0, 1, 2]], [40, 0, 30], 1, mute=mute), tick([[0, 1, 2]], [40, 0, 30], 1)])
    assert res[0][1].tolist() == [1, 0, 0] and res[0][0].tolist() == [40, 9000, 30]
    assert res[1][1].tolist() == [1, 0, 0] and res[1][0][1] == 9000 - (9000 >> 3)
    assert res[2][1].tolist() == [0, 1, 0]  # unmuted in the middle of a sentence: selected at once, on the held envelope


def test_max_speakers_of_the_conference_size_or_more_selects_every_eligible_leg(driver):
    mute = np.array([0, 0, 1, 0], np.uint8)
    for mx in (4, 5, 32):
        (_, sp, _), = driver(4, [tick([[3, 2, 1, 0]], [7, 0, 50, 9], mx, floor=1, mute=mute)])
        assert sp.tolist() == [1, 0, 0, 1]  # ring 1 is below the floor, ring 2 muted


def test_a_one_member_conference_and_an_idle_ring_keep_their_envelope(driver):
    res = driver(5, [tick([[0, 1], [2, 3, 4]], [10, 20, 30, 40, 50], 2), tick([[0, 1], [2], []], [1, 2, 3, 4, 5], 2, shift=1)])
    assert res[1][0].tolist() == [5, 10, 30, 40, 50]  # rings 2 (alone), 3 and 4 (idle): untouched, neither decayed nor raised
    assert res[1][1].tolist() == [1, 1, 0, 0, 0] and res[1][2].tolist() == [0, 0, 1, 1, 1]
