"""Talker selection over leg packets on the CPU (wmix_amd/csrc/speakers.h: speakers_level_legs, speakers_step_legs -- what mix.hip's
select_speakers_legs_kernel states): a stand-alone C++ driver, built with g++ and the address and undefined-behaviour sanitizers,
replays scenarios written by this file, and every tick's env / speaking / mute_out must equal the numpy model of
tests/speakers_legs_model.py.  Random layouts, and the hand-made cases whose outcome is also asserted by value."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from speakers_legs_model import SpeakersLegsModel
from speakers_model import SpeakersModel, row_of_level

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#include "speakers.h"

// scenario file: n_groups n_ticks, then per tick: max floor shift n_el K packet_stride n_conf has_mute | per conference: n, rings |
// [mute by ring] | len by ring and slot | the rows, slot k of ring r at (r * K + k) * packet_stride, exactly up to the last element of the
// last row.  Prints per tick: env by ring, speaking by ring, mute_out by ring.
int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    int n_groups = 0, n_ticks = 0;
    if (!f || fscanf(f, "%d %d", &n_groups, &n_ticks) != 2) return 2;
    std::vector<uint32_t> env((size_t)n_groups, 0), env1;
    std::vector<uint8_t> speaking((size_t)n_groups), mute_out((size_t)n_groups), mute((size_t)n_groups), sp1((size_t)n_groups), mo1((size_t)n_groups);
    for (int t = 0; t < n_ticks; t++) {
        int max_speakers, shift, n_el, K, pstride, n_conf, has_mute;
        unsigned floor;
        if (fscanf(f, "%d %u %d %d %d %d %d %d", &max_speakers, &floor, &shift, &n_el, &K, &pstride, &n_conf, &has_mute) != 8) return 3;
        if (!wmx::speakers_params_ok(max_speakers, shift) || !wmx::speakers_len_ok(2u * (unsigned)n_el) || K < 1 || K > wmx::kSpeakersMaxLegPackets) return 4;
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
        std::vector<uint32_t> len((size_t)n_groups * K);
        bool all_calls = true;
        for (auto &x : len) {
            if (fscanf(f, "%u", &x) != 1) return 3;
            all_calls = all_calls && x == 2u * (unsigned)n_el;
        }
        std::vector<int16_t> rows(((size_t)n_groups * K - 1) * pstride + n_el);  // exactly the rows: a read past one is the sanitizer's to find
        for (auto &x : rows) {
            int v;
            if (fscanf(f, "%d", &v) != 1) return 3;
            x = (int16_t)v;
        }
        env1 = env;
        wmx::speakers_step_legs(n_groups, n_conf, off.data(), members.data(), rows.data(), (long)K * pstride, pstride, K, len.data(), 2u * (unsigned)n_el,
                                has_mute ? mute.data() : nullptr, max_speakers, floor, shift, env.data(), speaking.data(), mute_out.data());
        if (K == 1 && all_calls) {  // one slot, always a call: the row-per-leg rule
            wmx::speakers_step(n_groups, n_conf, off.data(), members.data(), rows.data(), pstride, (uint32_t)n_el, has_mute ? mute.data() : nullptr,
                               max_speakers, floor, shift, env1.data(), sp1.data(), mo1.data());
            if (env1 != env || sp1 != speaking || mo1 != mute_out) return 6;
        }
        for (int r = 0; r < n_groups; r++) printf("%u ", env[(size_t)r]);
        for (int r = 0; r < n_groups; r++) printf("%d ", speaking[(size_t)r]);
        for (int r = 0; r < n_groups; r++) printf("%d ", mute_out[(size_t)r]);
        printf("\n");
    }
    printf("done\n");
    return 0;
}
"""

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("speakers_legs")
    src = d / "speakers_legs_driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function"] + SAN +
                          ["-I" + os.path.join(ROOT, "wmix_amd", "csrc"), "-o", str(exe), str(src)])
    count = [0]

    def run(n_groups, ticks):
        """ticks: dicts(layout, rows [n_groups, K, n_el] int16, lens [n_groups, K], max, floor, shift, mute=None, pad=0) -> per tick (env,
        speaking, mute_out), after asserting that the header and the model agree on every tick"""
        lines = ["%d %d" % (n_groups, len(ticks))]
        for tk in ticks:
            rows, lens = np.asarray(tk["rows"], np.int16), np.asarray(tk["lens"], np.uint32)
            n, K, n_el = rows.shape
            assert n == n_groups and lens.shape == (n, K)
            pstride, mute = n_el + tk.get("pad", 0), tk.get("mute")
            padded = np.full((n, K, pstride), 32767, np.int16)  # what lies between the rows is loud: reading it would show
            padded[:, :, :n_el] = rows
            lines.append("%d %d %d %d %d %d %d %d" % (tk["max"], tk["floor"], tk["shift"], n_el, K, pstride, len(tk["layout"]), mute is not None))
            for mem in tk["layout"]:
                lines.append(" ".join(map(str, [len(mem)] + list(mem))))
            if mute is not None:
                lines.append(" ".join(str(int(v)) for v in mute))
            lines.append(" ".join(map(str, lens.reshape(-1).tolist())))
            lines.append(" ".join(map(str, padded.reshape(-1)[:(n * K - 1) * pstride + n_el].tolist())))
        count[0] += 1
        path = d / ("scenario_%d.txt" % count[0])
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, (r.stdout + r.stderr)[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        out = r.stdout.strip().splitlines()
        assert out[-1] == "done" and len(out) == len(ticks) + 1
        model, res = SpeakersLegsModel(n_groups), []
        for t, tk in enumerate(ticks):
            got = np.array(out[t].split(), dtype=np.int64).reshape(3, n_groups)
            n_el = np.asarray(tk["rows"]).shape[2]
            sp, mo = model.step_legs(tk["layout"], tk["rows"], tk["lens"], 2 * n_el, tk["max"], tk["floor"], tk["shift"], tk.get("mute"))
            assert np.array_equal(got[0], model.env.astype(np.int64)), ("env, tick", t)
            assert np.array_equal(got[1], sp) and np.array_equal(got[2], mo), ("speaking, tick", t)
            res.append((got[0].copy(), got[1].copy(), got[2].copy()))
        return res

    return run


E = 16  # elements per row in the hand-made cases
CALL = 2 * E


def legs(levels, lens):
    """levels [n][K] -> rows [n, K, E]; lens as given"""
    rows = np.stack([np.stack([row_of_level(int(v), E) for v in leg]) for leg in levels])
    return dict(rows=rows, lens=np.asarray(lens, np.uint32))


def tick(layout, levels, lens, mx, floor=0, shift=3, mute=None, pad=0):
    return dict(layout=layout, max=mx, floor=floor, shift=shift, mute=mute, pad=pad, **legs(levels, lens))


def random_layout(rng, n_groups):
    rings = rng.permutation(n_groups).tolist()
    layout = []
    for n in rng.permutation([0, 1, 2, 2, 3, 4, 5, 8, 9, 17, 32]).tolist():
        n = min(int(n), len(rings))
        layout.append([rings.pop() for _ in range(n)])
    return layout


def test_random_layouts(driver):
    """conferences of 0, 1, 2 .. 32 members, 1 .. 4 slots, d_len values that are 0, the call's length, and neither"""
    rng = np.random.default_rng(41)
    n_groups = 90
    for K, n_el, pad in ((1, 7, 0), (2, 160, 1), (3, 160, 4), (4, 9, 3)):
        ticks, layout = [], random_layout(rng, n_groups)
        assert sorted(len(m) for m in layout)[-1] == 32 and {0, 1, 2} <= {len(m) for m in layout}
        for t in range(8):
            if t == 4:
                layout = random_layout(rng, n_groups)
            rows = rng.integers(-32768, 32768, size=(n_groups, K, n_el)).astype(np.int16)
            rows[rng.random(n_groups) < 0.3] = 0
            rows[rng.random(n_groups) < 0.2] >>= 6
            lens = np.array([0, 2 * n_el, 2 * n_el, 2 * n_el - 2, 2 * n_el + 2, 1], np.uint32)[rng.integers(0, 6, size=(n_groups, K))]
            mute = (rng.random(n_groups) < 0.15).astype(np.uint8) if t % 3 else None
            floor = int(rng.choice([0, 1, int(np.abs(rows[:, 0].astype(np.int64)).sum(1)[n_groups // 2]), 1 << 31]))
            ticks.append(dict(layout=layout, rows=rows, lens=lens, max=int(rng.integers(1, 33)), floor=floor, shift=int(rng.integers(0, 32)), mute=mute,
                              pad=pad))
        res = driver(n_groups, ticks)
        assert any(sp.any() for _, sp, _ in res) and any(not sp.all() for _, sp, _ in res)


def test_a_leg_with_no_call_has_level_0_whatever_its_rows_hold(driver):
    res = driver(3, [tick([[0, 1, 2]], [[900, 900], [50, 0], [10, 20]], [[0, CALL + 2], [CALL, 0], [CALL, CALL]], 1),
                     tick([[0, 1, 2]], [[900, 900], [0, 0], [0, 0]], [[0, 0], [0, 0], [0, 0]], 1, shift=1)])
    assert res[0][0].tolist() == [0, 50, 20] and res[0][1].tolist() == [0, 1, 0]
    assert res[1][0].tolist() == [0, 25, 10] and res[1][1].tolist() == [0, 1, 0]  # nobody calls: everybody decays, nobody jumps


def test_a_call_only_in_the_last_slot_counts(driver):
    (env, sp, mo), = driver(2, [tick([[0, 1]], [[5000, 5000, 5000, 70], [60, 0, 0, 0]], [[0, 1, CALL - 2, CALL], [CALL, 0, 0, 0]], 1)])
    assert env.tolist() == [70, 60] and sp.tolist() == [1, 0] and mo.tolist() == [0, 1]


def test_equal_levels_in_two_slots_are_that_level(driver):
    (env, sp, _), = driver(2, [tick([[1, 0]], [[300, 300, 10], [300, 0, 0]], [[CALL, CALL, CALL], [CALL, 0, 0]], 1)])
    assert env.tolist() == [300, 300] and sp.tolist() == [0, 1]  # and the tie between the legs goes to list position 0, ring 1


def test_a_row_of_minus_32768_in_a_later_slot(driver):
    rows = np.zeros((2, 2, 160), np.int16)
    rows[0, 1] = -32768
    rows[1, 0] = 32767
    (env, sp, _), = driver(2, [dict(layout=[[1, 0]], rows=rows, lens=np.array([[0, 320], [320, 320]], np.uint32), max=1, floor=0, shift=3)])
    assert env.tolist() == [160 * 32768, 160 * 32767] and sp.tolist() == [1, 0]


def test_ties_between_list_positions_go_to_the_earlier_one(driver):
    (env, sp, _), = driver(6, [tick([[5, 2, 4]], [[0, 0]] * 2 + [[0, 700]] + [[0, 0]] + [[700, 1]] + [[700, 700]],
                                    [[CALL, CALL]] * 2 + [[7, CALL]] + [[CALL, CALL]] * 3, 2)])
    assert sp.tolist() == [0, 0, 1, 0, 0, 1] and env[[5, 2, 4]].tolist() == [700, 700, 700]


def test_one_slot_that_is_always_a_call_is_the_row_per_leg_rule(driver):
    """max_packets == 1: the driver itself compares speakers_step_legs with speakers_step (exit status 6); here also with that model"""
    rng = np.random.default_rng(43)
    n_groups, layout = 40, [[3, 1], [30, 10, 20], list(range(39, 31, -1)), [0], []]
    ticks = [dict(layout=layout, rows=rng.integers(-3000, 3000, size=(n_groups, 1, 160)).astype(np.int16) >> int(rng.integers(0, 8)),
                  lens=np.full((n_groups, 1), 320, np.uint32), max=2, floor=4000, shift=2, mute=None, pad=t % 2) for t in range(6)]
    res = driver(n_groups, ticks)
    old = SpeakersModel(n_groups)
    for t, tk in enumerate(ticks):
        sp, _ = old.step(layout, tk["rows"][:, 0], 2, 4000, 2)
        assert np.array_equal(res[t][1], sp) and np.array_equal(res[t][0], old.env.astype(np.int64))
