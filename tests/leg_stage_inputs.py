"""What the kernel tests of the bridge's per-leg stages feed the kernels and their models (tests/test_nsx_legs_gpu.py,
test_agc_legs_gpu.py; tests/leg_gate_inputs.py takes the row schedule for the gate's): seeded random rows at levels from 3 to 30 000,
0 .. max_packets rows per leg and tick, lens other than 0 and 320 among them, one leg that never gets a row, and random call lists.
numpy only: no oracle, no GPU, nothing of wmix_amd."""
import numpy as np

ROW = 160
N, TICKS, IDLE_LEG = 37, 40, 5
OTHER_LENS = (0, 0, 0, 172, 318, 322, 640, 160)  # what a slot that holds no row says
AMPS = (3, 40, 400, 3000, 12000, 30000)


def signal(rng, g, n):
    """n samples of leg g: noise at the leg's level under a tone that comes and goes"""
    t = np.arange(n)
    x = rng.normal(0, AMPS[g % len(AMPS)], n) + 0.5 * AMPS[(g + 2) % len(AMPS)] * np.sin(2 * np.pi * (200 + 37 * g) * t / 8000) * (t % 4000 < 2000)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def random_list(rng, lens, k_slots):
    """a call list over one leg's slots: a permuted subset of the readable slots, silence calls between them, now and then a data call
    naming a slot that holds no row or lies beyond max_packets; often filled up to four calls"""
    readable = [k for k in range(k_slots) if lens[k] == 320]
    rng.shuffle(readable)
    calls = [("D", k) for k in readable[:len(readable) if rng.integers(0, 2) else int(rng.integers(0, len(readable) + 1))]]
    unreadable = [k for k in range(4) if k >= k_slots or lens[k] != 320]
    if unreadable and len(calls) < 4 and rng.integers(0, 3) == 0:
        calls.insert(int(rng.integers(0, len(calls) + 1)), ("D", int(rng.choice(unreadable))))
    target = 4 if rng.integers(0, 2) else int(rng.integers(len(calls), 5))
    while len(calls) < target:
        calls.insert(int(rng.integers(0, len(calls) + 1)), ("S", None))
    return calls


def script(seed, k_slots, with_lists, n=N, ticks=TICKS, pad=8):
    """-> per tick (plane int16 [n, k_slots, 160 + pad], lens uint32 [n, k_slots], lists or None)"""
    rng = np.random.default_rng(seed)
    src = [signal(rng, g, ticks * k_slots * ROW) for g in range(n)]
    at, out = [0] * n, []
    for t in range(ticks):
        plane = rng.integers(-32768, 32768, size=(n, k_slots, ROW + pad)).astype(np.int16)  # rows not taken hold anything
        lens = rng.choice(OTHER_LENS, size=(n, k_slots)).astype(np.uint32)
        for g in range(n):
            if g == IDLE_LEG:
                continue
            for k in rng.permutation(k_slots)[:int(rng.integers(0, k_slots + 1))]:
                lens[g, k] = 320
                plane[g, k, :ROW] = src[g][at[g]:at[g] + ROW]
                at[g] += ROW
        lists = [random_list(rng, lens[g], k_slots) for g in range(n)] if with_lists else None
        if with_lists:
            lists[IDLE_LEG] = [c for c in lists[IDLE_LEG] if c[0] == "S"]
        out.append((plane, lens, lists))
    return out
