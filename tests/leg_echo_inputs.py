"""Inputs of the echo-control tests of the bridge's legs (tests/test_leg_echo_ctl_host.py, test_aecm_legs_gpu.py): a speech-like far
end, and the per-leg call patterns -- how many near rows a leg brings in each of 60 ticks.  The canceller's delay estimator needs a
far end that is not periodic: stationary noise and a tiled excerpt do not converge, syllables with gliding pitch do."""
import numpy as np

TICKS = 60
DELAYS = (0, 20, 200, 500)  # reported delays, ms


def talk(n, seed, amp=4000):
    """n samples at 8 kHz, int16: N(0, 20) noise under syllables of 640 .. 2400 samples, each a harmonic series on a pitch of 90 ..
    250 Hz that glides linearly by -15 .. +15 %, the harmonics below 3 600 Hz weighted by two formants (300 .. 900 and 1000 .. 2800 Hz)
    with random phases, 160-sample raised-cosine edges, the peak at amp * uniform(0.5, 1); 320 .. 2400 samples of pause between them"""
    rng = np.random.default_rng(seed)
    out = rng.normal(0.0, 20.0, n)
    at = int(rng.integers(0, 800))
    edge = 0.5 - 0.5 * np.cos(np.pi * np.arange(160) / 160)
    while at < n:
        m = int(rng.integers(640, 2401))
        f0, glide = rng.uniform(90, 250), rng.uniform(-0.15, 0.15)
        c1, c2 = rng.uniform(300, 900), rng.uniform(1000, 2800)
        t = np.arange(m)
        pitch = f0 * (1 + glide * t / m)
        phase = 2 * np.pi * np.cumsum(pitch) / 8000.0
        syl = np.zeros(m)
        for h in range(1, int(3600 / (f0 * (1 + abs(glide)))) + 1):
            f = h * f0
            if f >= 3600:
                break
            w = np.exp(-((f - c1) / 200) ** 2) + 0.5 * np.exp(-((f - c2) / 300) ** 2) + 0.02
            syl += w * np.sin(h * phase + rng.uniform(0, 2 * np.pi))
        env = np.ones(m)
        env[:160], env[-160:] = edge, edge[::-1]
        syl *= env
        syl *= amp * rng.uniform(0.5, 1) / max(np.abs(syl).max(), 1e-9)
        k = min(m, n - at)
        out[at:at + k] += syl[:k]
        at += m + int(rng.integers(320, 2401))
    return np.clip(np.rint(out), -32768, 32767).astype(np.int16)


def patterns(seed=7):
    """the call patterns: name -> near rows per tick, TICKS entries of 0 .. 4"""
    rng = np.random.default_rng(seed)
    p = {"one": [1] * TICKS,
         "random": [int(v) for v in rng.integers(0, 4, TICKS)],
         "30_empty": [0] * 30 + [1] * 30,
         "two": [2] * TICKS,
         "4_0": ([4] * 5 + [0] * 5) * 6,
         "gap_burst": [1] * 20 + [0] * 8 + [3, 3, 2] + [1] * 29}
    assert all(len(v) == TICKS and 0 <= min(v) and max(v) <= 4 for v in p.values())
    return p
