"""The bridge's recording taps on the CPU (wmix_amd/csrc/leg_record.h: what wmx_rtp_record / _record_stop / _reset_record do on the
host and wmx_rtp_record_rings applies on the device per tap and tick).  tools_dev/san/leg_record_san.cpp, a stand-alone program compiled
with g++ against the header the kernel includes and with AddressSanitizer + UndefinedBehaviorSanitizer, evaluates the header over a
script; tests/leg_record_model.py, written from the rule's text, is what it must equal, state for state, command by command.  Integers."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from leg_record_model import RecordModel, Refused

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Werror",
       "-Wno-unused-function"]
CSRC = os.path.join(ROOT, "wmix_amd", "csrc")
TAPS = 3

# (command, ...): start ticks legs | stop legs-or-None | reset legs-or-None | tick
SCRIPT = [
    ("tick",),                        # nothing running
    ("start", 2, [4]),                # ticks = 2: tap 0
    ("start", 0, [1]),                # until stopped: tap 1
    ("tick",),
    ("start", 1, [4]),                # a second start of the same leg: in place, written = 0, and now ticks = 1
    ("tick",),                        # leg 4's last row: tap 0 frees itself behind it, written 1
    ("tick",),                        # leg 1 alone
    ("start", 2, [7, 2]),             # the freed tap 0 is taken again, by another leg, the lowest first; leg 2 takes the LAST free tap
    ("start", 1, [5]),                # refused: no free tap; nothing changes
    ("start", 3, [1, 5]),             # refused as a whole: leg 1 has a tap, leg 5 finds none -- leg 1 is NOT restarted
    ("start", 5, [2, 2]),             # a leg listed twice has one tap
    ("tick",),
    ("stop", [1]),                    # stopped mid-story: written stays
    ("tick",),                        # leg 7's second and last
    ("reset", [2, 6]),                # reset of the tap's leg (and of a leg that has none): free, written = 0
    ("tick",),                        # nothing running again
    ("start", 0, [3, 6, 0]),          # every tap at once
    ("tick",), ("tick",),
    ("stop", None),                   # every tap
    ("tick",),
    ("start", 1, [9]), ("tick",), ("tick",),
    ("reset", None),                  # every tap: written = 0 everywhere
]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("leg_record") / "leg_record_san"
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tools_dev", "san", "leg_record_san.cpp")])
    return str(exe)


def as_text(script):
    lines = []
    for c in script:
        if c[0] == "tick":
            lines.append("tick")
        elif c[0] == "start":
            lines.append("start %d %d %s" % (c[1], len(c[2]), " ".join(map(str, c[2]))))
        else:
            lines.append("%s %s" % (c[0], "-1" if c[1] is None else "%d %s" % (len(c[1]), " ".join(map(str, c[1])))))
    return "\n".join(lines) + "\n"


def header(program, script, taps=TAPS):
    """-> per command (what it answered or None, the state per tap as (leg, left, written), any tap running)"""
    r = subprocess.run([program, str(taps)], input=as_text(script), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    out, answer = [], None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] in ("rows", "taps"):
            answer = [int(v) for v in w[1:]]
        elif w[0] == "refused":
            answer = "refused"
        else:
            v = [int(x) for x in w[:-2]]
            out.append((answer, [tuple(v[i:i + 3]) for i in range(0, len(v), 3)], int(w[-1])))
            answer = None
    assert len(out) == len(script)
    return out


def model(script, taps=TAPS):
    m, out = RecordModel(taps), []
    for c in script:
        answer = None
        if c[0] == "tick":
            answer = m.tick()
        elif c[0] == "start":
            try:
                answer = m.start(c[2], c[1])
            except Refused:
                answer = "refused"
        else:
            getattr(m, c[0])(c[1])
        e = m.export()
        out.append((answer, list(zip(e["leg"].tolist(), e["left"].tolist(), e["written"].tolist())), int(m.running())))
    return out


def test_the_header_equals_the_model_state_for_state(program):
    got, want = header(program, SCRIPT), model(SCRIPT)
    for i, (c, g, w) in enumerate(zip(SCRIPT, got, want)):
        assert g == w, (i, c, g, w)


def test_what_the_script_reaches(program):
    """the script is only worth its name if it meets every arm of the rule"""
    got = header(program, SCRIPT)
    at = {i: g for i, g in enumerate(got)}
    assert at[0] == ([-1, -1, -1], [(-1, 0, 0)] * 3, 0)
    assert at[1][0] == [0] and at[2][0] == [1]
    assert at[4][0] == [0] and at[4][1][0] == (4, 1, 0)  # restarted in place
    assert at[5][0] == [4, 1, -1] and at[5][1][0] == (-1, 0, 1)  # ticks = 1: one row, then free, written counted
    assert at[7][0] == [0, 2] and at[7][2] == 1  # the freed tap, lowest first, and the last free tap
    assert at[8][0] == "refused" and at[8][1] == at[7][1]
    assert at[9][0] == "refused" and at[9][1] == at[7][1]
    assert at[10][0] == [2, 2] and at[10][1][2] == (2, 5, 0)
    assert at[12][1][1] == (-1, 0, 4)  # stopped: written stays
    assert at[13][0] == [7, -1, 2] and at[13][1][0] == (-1, 0, 2)  # ticks = 2: two rows
    assert at[14][1][2] == (-1, 0, 0) and at[15][2] == 0
    assert at[17][1] == [(3, 0, 1), (6, 0, 1), (0, 0, 1)]  # ticks = 0 stays 0
    assert got[-1][1] == [(-1, 0, 0)] * 3


def test_random_scripts(program):
    """drawn scripts over 1, 2 and 5 taps: the header and the model agree on every state"""
    rng = np.random.default_rng(7)
    for taps in (1, 2, 5):
        script = []
        for _ in range(400):
            u = int(rng.integers(0, 10))
            legs = [int(g) for g in rng.integers(0, 8, size=int(rng.integers(0, 4)))]
            if u < 5:
                script.append(("tick",))
            elif u < 8:
                script.append(("start", int(rng.integers(0, 4)), legs))
            else:
                script.append((("stop", "reset")[u - 8], None if rng.integers(0, 5) == 0 else legs))
        got, want = header(program, script, taps), model(script, taps)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (taps, i, script[i], g, w)
        assert any(g[0] == "refused" for g in got)
