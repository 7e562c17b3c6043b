"""The algebra of the bridge load on the CPU (wmix_amd/csrc/mix_minus.h): ring q of a conference of P participants must end as
what P - 1 ordered wmix_load_data calls (every source but its own) leave there.  volumeAdd (src/wmix.c:1617-1636) is a saturating,
order-dependent add, so "total minus own" is wrong; the header composes clamp maps instead: prefix map F_q = f_(q-1) o .. o f_0,
suffix map G_q = f_(P-1) o .. o f_(q+1), ring_q <- G_q(F_q(ring_q)).  A small C++ driver, compiled with g++ against the header the
kernel includes (sanitizer flags as tools_dev/san/Makefile sets them: a finding kills the driver and fails the test), compares
that with the sequential volumeAdd loop.  Equality, no tolerance."""
import os
import subprocess

from conftest import ROOT

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mix_minus.h"

using namespace wmx;

// src/wmix.c:1617-1636, restated
static int16_t volume_add(int16_t a, int16_t b) {
    if (a == 0) return b;
    if (b == 0) return a;
    const int32_t s = (int32_t)a + b;
    return (int16_t)(s < -32768 ? -32768 : (s > 32767 ? 32767 : s));
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
static int16_t uniform(int scale) { return (int16_t)((int)(rnd() % (uint32_t)(2 * scale + 1)) - scale); }

struct Maps {
    std::vector<ClampMap> F, G;
    Maps(const int16_t *c, int P) : F(P), G(P) {
        ClampMap f = clamp_map_identity();
        for (int q = 0; q < P; q++) {  // F_q = f_(q-1) o .. o f_0
            F[q] = f;
            f = clamp_map_then_add(f, c[q]);
        }
        ClampMap g = clamp_map_identity();
        for (int q = P - 1; q >= 0; q--) {  // G_q = f_(P-1) o .. o f_(q+1)
            G[q] = g;
            g = clamp_map_add_then(c[q], g);
        }
    }
};

static int16_t sequential(const int16_t *c, int P, int q, int16_t x) {
    for (int s = 0; s < P; s++)
        if (s != q) x = volume_add(x, c[s]);
    return x;
}

static long bad = 0, shortcut_wrong = 0, checked = 0;

static void check_column(const int16_t *c, const int16_t *x, int P) {
    const Maps m(c, P);
    int32_t total = 0;
    for (int s = 0; s < P; s++) total += c[s];
    for (int q = 0; q < P; q++) {
        const int16_t want = sequential(c, P, q, x[q]);
        const int16_t got = clamp_map_apply(m.G[q], clamp_map_apply(m.F[q], x[q]));
        if (got != want) {
            if (bad < 10) fprintf(stderr, "P=%d q=%d x=%d: got %d, sequential volumeAdd gives %d\n", P, q, x[q], got, want);
            bad++;
        }
        const int32_t sc = clamp_i32((int32_t)x[q] + total - c[q], -32768, 32767);
        shortcut_wrong += sc != want;
        checked++;
    }
}

int main() {
    const int parties[] = {2, 3, 8, 16, 32};
    const int scales[] = {3000, 12000, 20000};
    int16_t c[32], x[32];
    for (int P : parties) {
        // random columns; the rings start non-zero and different per q
        for (int scale : scales) {
            for (int n = 0; n < 20000; n++) {
                for (int q = 0; q < P; q++) {
                    c[q] = uniform(scale);
                    for (;;) {
                        x[q] = uniform(scale);
                        bool ok = x[q] != 0;
                        for (int r = 0; r < q; r++) ok = ok && x[r] != x[q];
                        if (ok) break;
                    }
                }
                check_column(c, x, P);
            }
        }
        // columns of all 32767, all -32768, all 0
        const int16_t flat[] = {32767, -32768, 0};
        for (int16_t v : flat) {
            for (int n = 0; n < 2000; n++) {
                for (int q = 0; q < P; q++) {
                    c[q] = v;
                    x[q] = (int16_t)(uniform(30000) | 1) + (int16_t)(2 * q);
                }
                check_column(c, x, P);
            }
        }
        // exhaustively over every int16 ring value for a handful of fixed source columns
        for (int col = 0; col < 6; col++) {
            for (int q = 0; q < P; q++) {
                switch (col) {
                    case 0: c[q] = uniform(3000); break;
                    case 1: c[q] = uniform(12000); break;
                    case 2: c[q] = uniform(20000); break;
                    case 3: c[q] = 32767; break;
                    case 4: c[q] = -32768; break;
                    default: c[q] = (q & 1) ? -32768 : 32767; break;
                }
            }
            const Maps m(c, P);
            for (int v = -32768; v <= 32767; v++) {
                for (int q = 0; q < P; q++) {
                    const int16_t want = sequential(c, P, q, (int16_t)v);
                    const int16_t got = clamp_map_apply(m.G[q], clamp_map_apply(m.F[q], (int16_t)v));
                    if (got != want) {
                        if (bad < 10) fprintf(stderr, "exhaustive P=%d col=%d q=%d x=%d: got %d want %d\n", P, col, q, v, got, want);
                        bad++;
                    }
                    checked++;
                }
            }
        }
    }
    printf("checked %ld ring samples, %ld differ; clip(total - own) would have been wrong on %ld of the random ones\n", checked, bad,
           shortcut_wrong);
    return bad ? 1 : 0;
}
"""


def test_prefix_and_suffix_clamp_maps_equal_the_sequential_volume_add(tmp_path):
    src = tmp_path / "mix_minus_driver.cpp"
    exe = tmp_path / "mix_minus_driver"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-Wall", "-Werror", "-Wno-unused-function", "-I" + os.path.join(ROOT, "wmix_amd", "csrc"), "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert " 0 differ" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    # the feature is not a relabelled subtraction: on these inputs the shortcut is wrong somewhere
    assert int(r.stdout.split("wrong on")[1].split()[0]) > 0
