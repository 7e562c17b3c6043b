"""The walk over a leg's rows of a tick on the CPU (leg_calls_walk, wmix_amd/csrc/leg_calls.h: what the concealment, the DTMF and the
denoising kernel of the bridge's legs and the host forms of the first two apply per leg and tick).  tools_dev/san/leg_calls_san.cpp, a
stand-alone program compiled with g++ against the header the kernels include and with AddressSanitizer + UndefinedBehaviorSanitizer,
evaluates the header on every case; the few lines of numpy below, written from the header's text, are what it must equal."""
import os
import subprocess

import numpy as np

from conftest import ROOT

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Werror",
       "-Wno-unused-function"]
CSRC = os.path.join(ROOT, "wmix_amd", "csrc")


def model_list_form():
    """-> (list, count, data) of every (count 0 .. 7, entries 0 .. 4095, readable mask 0 .. 15), the mask innermost"""
    count, entries, mask = (a.ravel() for a in np.meshgrid(np.arange(8), np.arange(4096), np.arange(16), indexing="ij"))
    calls, data, walked = count.copy(), np.zeros_like(count), np.minimum(count, 4)
    for j in range(4):
        slot, silence = (entries >> 3 * j) & 3, (entries >> (3 * j + 2)) & 1
        calls |= (slot | silence << 2) << (4 + 4 * j)
        data |= ((j < walked) & (silence == 0) & ((mask >> slot) & 1 == 1)).astype(count.dtype) << j
    return np.stack([calls, walked, data], axis=1)


def model_slot_order():
    """-> (list, count, data) of every (readable mask 0 .. 15, max_packets 1 .. 4), max_packets innermost"""
    rows = []
    for mask in range(16):
        for max_packets in range(1, 5):
            slots = [k for k in range(max_packets) if (mask >> k) & 1]
            rows.append((len(slots) | sum(k << (4 + 4 * j) for j, k in enumerate(slots)), len(slots), (1 << len(slots)) - 1))
    return np.array(rows)


def test_every_case_of_the_walk_equals_the_model(tmp_path):
    exe = tmp_path / "leg_calls_san"
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tools_dev", "san", "leg_calls_san.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    got = np.array(r.stdout.split(), dtype=np.int64).reshape(-1, 3)
    want = np.concatenate([model_list_form(), model_slot_order()])
    assert got.shape == want.shape == (8 * 4096 * 16 + 16 * 4, 3)
    differ = np.flatnonzero((got != want).any(axis=1))
    assert differ.size == 0, ("case", int(differ[0]), "header", got[differ[0]], "model", want[differ[0]], "of", differ.size)
    # the sweep reaches every answer: each count, each mask of data calls, lists cut at four
    assert set(want[:, 1]) == {0, 1, 2, 3, 4} and set(want[:, 2]) == set(range(16))
