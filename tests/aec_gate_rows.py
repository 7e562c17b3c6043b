"""Rows for the tests of the float AEC's sdSum / seSum gate (wmix_amd/csrc/aec_gate.h): test_aec_decisions.py on the host,
test_aec_near_gate_gpu.py on the device.  A row is 65 non-negative float32 terms of sd and of se plus the divergeState in front of the
block; the reference (oracle/orc_aec.c:241-256) adds each in index order and compares."""
import numpy as np

F32 = np.float32


def reference(sd, se, prev):
    """(diverge, reset) as the reference takes them: ordered float32 sums, float32 products"""
    with np.errstate(all="ignore"):
        sd_sum = np.cumsum(sd, axis=1, dtype=F32)[:, -1]
        se_sum = np.cumsum(se, axis=1, dtype=F32)[:, -1]
        f = np.where(prev != 0, F32(1.05), F32(1.0)).astype(F32)
        diverge = (f * se_sum).astype(F32) > sd_sum
        reset = se_sum > (F32(19.95) * sd_sum).astype(F32)
    return diverge.astype(np.int32), reset.astype(np.int32)


def random_rows(n, seed):
    """se / sd log-uniform over [1e-3, 1e3], magnitudes 1e-20 .. 1e20, the 65 terms of a row spread over three decades"""
    rng = np.random.default_rng(seed)
    shape = 10.0 ** rng.uniform(-3, 0, (n, 65))
    mag = 10.0 ** rng.uniform(-20, 20, (n, 1))
    ratio = 10.0 ** rng.uniform(-3, 3, (n, 1))
    sd = (shape * mag).astype(F32)
    se = (10.0 ** rng.uniform(-3, 0, (n, 65)) * mag * ratio)
    se = (se * (sd.astype(np.float64).sum(1, keepdims=True) * ratio / se.sum(1, keepdims=True))).astype(F32)  # sum(se) / sum(sd) = ratio
    prev = rng.integers(0, 2, n).astype(np.int32)
    return sd, se, prev


def _near_threshold(rng, factor, prev, ulps):
    """rows whose ordered sums put `factor * seSum` (prev 0 / 1: the divergence test) or seSum against 19.95 * sdSum (factor None: the
    reset test) within a few ulp of equality, on both sides: the last term of se is moved float by float"""
    sd_rows, se_rows = [], []
    for u in ulps:
        sd = (10.0 ** rng.uniform(-2, 0, 65)).astype(F32)
        sd_sum = np.cumsum(sd, dtype=F32)[-1]
        target = sd_sum / F32(factor) if factor is not None else F32(19.95) * sd_sum
        se = (10.0 ** rng.uniform(-2, 0, 65)).astype(np.float64)
        se = (se * (float(target) * 0.6 / se[:64].sum())).astype(F32)  # the first 64 terms carry 0.6 of the target ...
        head = np.cumsum(se[:64], dtype=F32)[-1]
        last = F32(target) - head  # ... the last one the rest, so that the ordered sum lands on the target
        se[64] = last
        for _ in range(abs(u)):
            se[64] = np.nextafter(se[64], F32(np.inf) if u > 0 else F32(0), dtype=F32)
        sd_rows.append(sd)
        se_rows.append(se)
    return np.stack(sd_rows), np.stack(se_rows), np.full(len(ulps), prev, np.int32)


def crafted_rows(seed=3):
    """{kind: (sd, se, prev)}: every row must come back undecided or right, and at least one row of each kind undecided"""
    rng = np.random.default_rng(seed)
    kinds = {}
    x = (10.0 ** rng.uniform(-6, 6, (8, 1)) * rng.uniform(0.1, 1, (8, 65))).astype(F32)
    kinds["se == sd"] = (x, x.copy(), np.array([0, 1] * 4, np.int32))
    ulps = [-4, -3, -2, -1, 0, 1, 2, 3, 4]
    kinds["f = 1.0 within 4 ulp"] = _near_threshold(rng, 1.0, 0, ulps)
    kinds["f = 1.05 within 4 ulp"] = _near_threshold(rng, F32(1.05), 1, ulps)
    kinds["19.95 within 4 ulp"] = _near_threshold(rng, None, 0, ulps)
    y = rng.uniform(0.1, 1, (4, 65)).astype(F32)
    nan_sd, nan_se = y.copy(), y.copy() * F32(3)
    nan_sd[0, 5] = np.nan
    nan_se[1, 64] = np.nan
    nan_sd[2, 0] = nan_se[2, 0] = np.nan
    nan_se[3, 63] = np.nan
    kinds["NaN"] = (nan_sd, nan_se, np.array([0, 1, 0, 1], np.int32))
    inf_sd, inf_se = y.copy(), y.copy() * F32(3)
    inf_sd[0, 7] = np.inf
    inf_se[1, 64] = np.inf
    inf_sd[2, 1] = inf_se[2, 2] = np.inf
    inf_se[3, :] = F32(3e38)  # finite terms, infinite sum
    kinds["infinity"] = (inf_sd, inf_se, np.array([0, 1, 1, 0], np.int32))
    z = np.zeros((2, 65), F32)
    kinds["all zeros"] = (z, z.copy(), np.array([0, 1], np.int32))
    sub = (rng.uniform(0, 1, (4, 65)) * 1e-42).astype(F32)
    kinds["subnormal sums"] = (sub, (sub * F32(30)).astype(F32), np.array([0, 1, 0, 1], np.int32))
    return kinds
