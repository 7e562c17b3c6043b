"""The control plane of one leg's echo canceller on the CPU (AecmCtl, wmix_amd/csrc/aecm_ctl.h: the text aecm_legs_kernel runs per leg on
the device) against the oracle's handle.  tools_dev/san/leg_echo_san.cpp, a stand-alone program compiled with g++ against the header
the kernel includes and with AddressSanitizer + UndefinedBehaviorSanitizer, drives it with ragged call patterns -- per tick the leg's
0 .. 4 rows first, then the tick's far row -- and prints ec_startup, known_delay and the far ring's rd / wr / wrap behind every call;
the oracle's handle (orc_aecm_init(1, 8000, 20)), called alike with speech-like audio, must show the same words behind every call.
Six patterns of 60 ticks at reported delays of 0, 20, 200 and 500 ms; on the oracle alone: the set reaches the end of start-up, an
empty far ring (the farendOld replay), a full one and a change of known_delay."""
import os
import subprocess

import numpy as np

from conftest import ROOT
from leg_echo_inputs import DELAYS, TICKS, patterns, talk
from leg_echo_model import Leg

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Werror",
       "-Wno-unused-function"]
CSRC = os.path.join(ROOT, "wmix_amd", "csrc")


def oracle_words(lib, delay, rows_per_tick, far, near):
    """the oracle's handle over one script -> [ec_startup, known_delay, rd, wr, wrap] behind every call, and the far ring's fill
    behind every call"""
    leg, words, fill, n = Leg(lib, delay), [], [], 0

    def note():
        m = leg.mirror()
        words.append([m.ec_startup, m.known_delay, m.farend.rd, m.farend.wr, m.farend.diff_wrap])
        fill.append(m.farend.avail_read())

    for t, rows in enumerate(rows_per_tick):
        for _ in range(rows):
            leg.process(near[n % len(near)])
            n += 1
            note()
        leg.far(far[t])
        note()
    leg.close()
    return words, fill


def test_every_call_leaves_the_words_of_the_oracles_handle(tmp_path, oracle_port):
    exe = tmp_path / "leg_echo_san"
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tools_dev", "san", "leg_echo_san.cpp")])
    scripts = [(name, delay, rows) for name, rows in patterns().items() for delay in DELAYS]
    text = "".join("%d %s\n" % (delay, " ".join(map(str, rows))) for _, delay, rows in scripts)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    got = [np.array(part.split(), dtype=np.int64).reshape(-1, 5) for part in r.stdout.split("end\n")[:-1]]
    assert len(got) == len(scripts)
    far = talk(TICKS * 160, 1).reshape(TICKS, 160)
    near = talk(4 * TICKS * 160, 2, amp=1500).reshape(-1, 160)
    seen = {"startup_ends": False, "ring_empty": False, "ring_full": False, "known_delay_moves": False}
    for (name, delay, rows), have in zip(scripts, got):
        want, fill = oracle_words(oracle_port, delay, rows, far, near)
        want = np.array(want, np.int64)
        assert have.shape == want.shape == (sum(rows) + TICKS, 5), (name, delay)
        differ = np.flatnonzero((have != want).any(axis=1))
        assert differ.size == 0, (name, delay, "call", int(differ[0]), "header", have[differ[0]], "oracle", want[differ[0]])
        past = want[:, 0] == 0
        seen["startup_ends"] |= bool(past.any())
        seen["ring_empty"] |= bool((np.array(fill)[past] == 0).any())
        seen["ring_full"] |= 4000 in fill
        seen["known_delay_moves"] |= len(set(want[:, 1])) > 1
    assert all(seen.values()), seen
