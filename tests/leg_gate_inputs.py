"""What the tests of the per-leg voice-activity gate feed the kernel and its model: the alternating-spurts signal and the ragged script
of tests/test_vad_legs_gpu.py.  numpy, tests/conf_inputs.py's signals and the row schedule of tests/leg_stage_inputs.py only: no
oracle, no GPU, nothing of wmix_amd."""
import numpy as np

from conf_inputs import alaw_decode, voiced
from leg_stage_inputs import OTHER_LENS, ROW, random_list

N, TICKS = 70, 40          # one full workgroup and one of 6 lanes
SPURT = 25                 # rows of noise, then as many of noise plus voice
QUIET_LEG, NOISE_LEG, CODES_LEG = 3, 10, 17
LAST_GROUP = range(64, N)  # the second workgroup's legs
EMPTY_EVERY = 5            # in ticks t % 5 == 2 none of them brings a row


def spurts(rows, phase=0, seed=1):
    """rows x 160 samples: SPURT rows of N(0, 50) noise alternating with SPURT rows of that noise plus voiced(4000, ...); `phase` rows
    into the period, 0 = the start of a stretch of noise alone"""
    noise = np.random.default_rng(seed).normal(0, 50, rows * ROW)
    voice = voiced(4000, rows + phase)[phase * ROW:].astype(np.float64)
    on = np.repeat(((np.arange(rows) + phase) // SPURT) % 2 == 1, ROW)
    return np.clip(np.round(noise + on * voice), -32768, 32767).astype(np.int16)


def leg_signal(g, rows, seed):
    """leg g's stream of rows: the spurts at a phase of its own; one leg quiet, one stationary noise of sigma 400, one random A-law codes"""
    rng = np.random.default_rng(1000 * seed + g)
    if g == QUIET_LEG:
        return rng.integers(-8, 9, rows * ROW).astype(np.int16)
    if g == NOISE_LEG:
        return np.clip(np.round(rng.normal(0, 400.0, rows * ROW)), -32768, 32767).astype(np.int16)
    if g == CODES_LEG:
        return alaw_decode(rng.integers(0, 256, rows * ROW))
    return spurts(rows, phase=(7 * g) % (2 * SPURT), seed=1000 * seed + g)


def script(seed, k_slots, with_lists, n=N, ticks=TICKS, pad=0):
    """-> per tick (plane int16 [n, k_slots, 160 + pad], lens uint32 [n, k_slots], lists or None): every leg brings 0 .. k_slots rows
    from a seeded schedule, at seeded slots; a slot without a row says some other length and holds anything"""
    rng = np.random.default_rng(seed)
    src = [leg_signal(g, ticks * k_slots, seed) for g in range(n)]
    at, out = [0] * n, []
    for t in range(ticks):
        plane = rng.integers(-32768, 32768, size=(n, k_slots, ROW + pad)).astype(np.int16)  # sentinels: rows not taken hold anything
        lens = rng.choice(OTHER_LENS, size=(n, k_slots)).astype(np.uint32)
        for g in range(n):
            count = int(rng.integers(0, k_slots + 1))
            if g in LAST_GROUP and t % EMPTY_EVERY == 2:
                count = 0
            for k in sorted(rng.permutation(k_slots)[:count]):
                lens[g, k] = 320
                plane[g, k, :ROW] = src[g][at[g]:at[g] + ROW]
                at[g] += ROW
        lists = [random_list(rng, lens[g], k_slots) for g in range(n)] if with_lists else None
        out.append((plane, lens, lists))
    return out


CASES = [(3, False), (4, False), (3, True), (4, True)]  # (max_packets, with call lists)


def case_seed(k_slots, with_lists):
    return 100 * k_slots + int(with_lists)
