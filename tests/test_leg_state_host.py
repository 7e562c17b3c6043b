"""Where the columns of a per-leg state table lie, on the CPU (LegLayout, wmix_amd/csrc/leg_state.h: what rtp.hip, mix.hip and conf.hip
hand their kernels pointers from and reset by).  tools_dev/san/leg_state_san.cpp, a stand-alone program compiled with g++ against the
header the handles include and with AddressSanitizer + UndefinedBehaviorSanitizer, prints offsets, runs and the verdict of the layout
rule for the bridge's eight tables as the header lists them and for four tables that break the rule, at 1 .. 17 legs; the few lines of
numpy below, written from the header's text and DESIGN.md section 3l, are what it must equal."""
import os
import subprocess

import numpy as np

from conftest import ROOT

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Werror",
       "-Wno-unused-function"]
CSRC = os.path.join(ROOT, "wmix_amd", "csrc")

# (bytes per leg, fill byte) per column: senders, sequence, codec (sent law 1), concealment, DTMF, cursors, talkers, gate
PRODUCTION = [[(4, 0)] * 2, [(4, 0)] * 7, [(4, 0), (1, 0), (1, 1)], [(640, 0), (4, 0)], [(8, 0), (4, 0), (4, 0), (4, 0)],
              [(4, 0xFF), (4, 0), (4, 0)], [(4, 0), (1, 0)], [(4, 0), (4, 0)]]
BROKEN = [[(1, 0), (4, 0)], [(4, 0), (2, 0), (4, 0)], [(12, 0), (16, 0)], [(8, 0), (4, 0), (8, 0)]]


def model(t, cols, n):
    """-> the program's lines for table t at n legs"""
    size, fill = np.array(cols).T
    front = np.concatenate([[0], np.cumsum(size)])  # bytes per leg in front of column c; the last: of the whole table
    need = 2 ** np.floor(np.log2(np.minimum(size, 16))).astype(int)  # min(bytes, 16) rounded down to a power of two
    lines = ["T %d %d %d %d" % (t, n, len(cols), int((front[:-1] % need == 0).all()))]
    for c in range(len(cols)):
        run = {}
        for same_width in (False, True):
            e = c + 1
            while e < len(cols) and fill[e] == fill[c] and (not same_width or size[e] == size[c]):
                e += 1
            run[same_width] = e
        lines.append("C %d %d %d %d %d" % (size[c], fill[c], front[c] * n, run[False], run[True]))
    return lines + ["S %d" % (front[-1] * n)]


def test_every_table_at_every_leg_count_equals_the_model(tmp_path):
    exe = tmp_path / "leg_state_san"
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tools_dev", "san", "leg_state_san.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    got = r.stdout.splitlines()
    want = [line for t, cols in enumerate(PRODUCTION + BROKEN) for n in range(1, 18) for line in model(t, cols, n)]
    assert len(got) == len(want)
    differ = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not differ, ("line", differ[0], "header", got[differ[0]], "model", want[differ[0]], "of", len(differ))
    # every production table passes the layout rule and every broken one is refused, at every leg count
    verdict = np.array([line.split()[1:] for line in got if line.startswith("T")], dtype=np.int64).reshape(len(PRODUCTION + BROKEN), 17, 4)
    assert (verdict[:len(PRODUCTION), :, 3] == 1).all() and (verdict[len(PRODUCTION):, :, 3] == 0).all()
