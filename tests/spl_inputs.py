"""Arguments and references for the fixed-point primitives (wmix_amd/csrc/spl_dev.h, spl_fx.h) and the SPL real FFTs, shared by
tests/test_spl_primitives_oracle.py (CPU: the references against the oracle and the real reference) and
tests/test_spl_primitives_gpu.py (the device against the references).  No reference here is the code under test: each is the oracle
(oracle/orc_*.c), math.isqrt, or numpy integers with the two's-complement wrap spelled out, written from the WebRTC text the headers
cite (spl_inl.h, division_operations.c, spl_sqrt.c, digital_agc.h, signal_processing_library.h).

Every array of int32 operands is held as int64 while it is computed with and narrowed by s32 / u32 / s16 / u16 below, which is what
the C conversions of the callee's parameters do.  Argument sets and references are computed once per process (functools.lru_cache)
and handed out read-only."""
import ctypes as C
import functools
import math

import numpy as np

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
# wmx_debug_spl kinds (include/wmix_amd.h)
KINDS = {"norm_w16": 0, "norm_w32": 1, "norm_u32": 2, "size_in_bits": 3, "div_w32_w16": 4, "div_u32_u16": 5, "sqrt_floor": 6,
         "spl_sqrt": 7, "mul_rsft_round": 8, "agc_scalediff32": 9, "agc_mul32": 10, "spl_scalediff32": 11, "pk_abs16": 12,
         "pk_max_u16": 13}
WAVE_KINDS = {"wave_sum": 16, "wave_max": 17, "wave_min": 18, "wave_umax": 19, "wave_umin": 20}
# kinds of orc_spl_sweep (oracle/orc_spl.c) and ref_spl_sweep (oracle/ref_shim.c)
ORC_SWEEP = {"norm_w32": 0, "norm_u32": 1, "div_w32_w16": 2, "spl_sqrt": 3}
REF_SWEEP = {"sqrt_floor": 0, "spl_sqrt": 1, "div_w32_w16": 2, "div_u32_u16": 3}


# ---------------------------------------------------------------- two's-complement conversions on int64 carriers
def s32(x):
    return ((np.asarray(x, np.int64) + 2**31) & 0xFFFFFFFF) - 2**31


def u32(x):
    return np.asarray(x, np.int64) & 0xFFFFFFFF


def s16(x):
    return ((np.asarray(x, np.int64) + 2**15) & 0xFFFF) - 2**15


def u16(x):
    return np.asarray(x, np.int64) & 0xFFFF


def _frozen(a, dtype=np.int32):
    a = np.ascontiguousarray(a, dtype=dtype)
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------- argument sets
@functools.lru_cache(None)
def edge32():
    """0, +-1, INT32_MIN, INT32_MAX and 2^k - 1, 2^k, 2^k + 1 with both signs for k = 1 .. 31, as far as int32 holds them (2^31 and
    2^31 + 1 exist only negated / not at all); sorted, unique.  Read as uint32 bit patterns they include 0xFFFFFFFF, 0x80000000 and
    0x80000001."""
    v = {0, 1, -1, INT32_MIN, INT32_MAX}
    for k in range(1, 32):
        for d in (-1, 0, 1):
            v.update((2**k + d, -(2**k + d)))
    return _frozen(sorted(x for x in v if INT32_MIN <= x <= INT32_MAX), np.int64)


@functools.lru_cache(None)
def edge16():
    v = {0, 1, -1, -32768, 32767}
    for k in range(1, 16):
        for d in (-1, 0, 1):
            v.update((2**k + d, -(2**k + d)))
    return _frozen(sorted(x for x in v if -32768 <= x <= 32767), np.int64)


@functools.lru_cache(None)
def all16():
    return _frozen(np.arange(-32768, 32768), np.int64)


@functools.lru_cache(None)
def rand32(seed):
    """2^20 seeded random 32-bit words"""
    return _frozen(np.random.default_rng(seed).integers(INT32_MIN, INT32_MAX + 1, size=1 << 20, dtype=np.int64), np.int64)


def _grid(a, b):
    """every pair: a varies slowest"""
    return np.repeat(a, b.size), np.tile(b, a.size)


DIV_EXCLUDED = (INT32_MIN, -1)  # the reference's idiv traps: there is no answer to match


@functools.lru_cache(None)
def arguments(name):
    """(a, b, c) int32 arrays for wmx_debug_spl(KINDS[name]); b, c are None where the primitive does not take them."""
    if name in ("norm_w16", "norm_w32", "norm_u32", "size_in_bits", "spl_sqrt", "sqrt_floor"):
        # all 65 536 16-bit values (norm_w16: its whole domain; the others: every small value of both signs), the 32-bit edge set, random
        # words -- which norm_w16 narrows like any other argument
        parts = [all16(), edge32(), rand32(101)]
        if name == "sqrt_floor":  # every argument at which the floor changes, and its neighbours (tests/test_sqrt_floor.py lists the same)
            k = np.arange(0, 46341, dtype=np.int64)
            parts += [k * k - 1, k * k, k * k + 1, np.array([INT32_MAX, INT32_MAX - 1])]
        a = np.concatenate(parts)
        return _frozen(a[(a >= INT32_MIN) & (a <= INT32_MAX)]), None, None
    if name in ("div_w32_w16", "div_u32_u16"):
        # the edge set against all 65 536 divisors, then random numerators against random divisors
        a, b = _grid(edge32(), all16())
        a, b = np.concatenate([a, rand32(102)]), np.concatenate([b, s16(rand32(103))])
        if name == "div_u32_u16":  # the same bit patterns, both operands read unsigned by the callee
            return _frozen(a), _frozen(b), None
        keep = ~((a == DIV_EXCLUDED[0]) & (b == DIV_EXCLUDED[1]))
        return _frozen(a[keep]), _frozen(b[keep]), None
    if name == "mul_rsft_round":
        # every 16-bit a against the 16-bit edge set, the shift running through 1 .. 31 (65 536 = 2 mod 31: each pair of neighbours in b
        # meets other shifts); then random words, narrowed by the callee
        a, b = _grid(all16(), edge16())
        c = 1 + np.arange(a.size, dtype=np.int64) % 31
        a, b = np.concatenate([a, rand32(104)]), np.concatenate([b, rand32(105)])
        c = np.concatenate([c, 1 + u32(rand32(106)) % 31])
        return _frozen(a), _frozen(b), _frozen(c)
    if name in ("agc_scalediff32", "spl_scalediff32"):
        e = edge32()
        a, b = _grid(e, e)
        a, c = _grid(a, e)
        b = np.repeat(b, e.size)
        return (_frozen(np.concatenate([a, rand32(107)])), _frozen(np.concatenate([b, rand32(108)])),
                _frozen(np.concatenate([c, rand32(109)])))
    if name == "agc_mul32":
        a, b = _grid(edge32(), edge32())
        a2, b2 = _grid(all16(), edge32()[::3])
        return (_frozen(np.concatenate([a, a2, b2, rand32(110)])), _frozen(np.concatenate([b, b2, a2, rand32(111)])), None)
    if name == "pk_abs16":
        # every 16-bit value in either half beside each 16-bit edge in the other, then random words
        lo, hi = _grid(all16(), edge16())
        a = np.concatenate([u16(lo) | (u16(hi) << 16), u16(hi) | (u16(lo) << 16), rand32(112)])
        return _frozen(s32(a)), None, None
    if name == "pk_max_u16":
        lo, hi = _grid(all16(), edge16())
        a = np.concatenate([u16(lo) | (u16(hi) << 16), u16(hi) | (u16(lo) << 16), rand32(113)])
        b = np.concatenate([u16(hi) | (u16(lo) << 16), u16(lo[::-1]) | (u16(hi) << 16), rand32(114)])
        return _frozen(s32(a)), _frozen(s32(b)), None
    raise KeyError(name)


# ---------------------------------------------------------------- numpy references, from the WebRTC text
def ref_norm_w32(a):
    """spl_inl.h WebRtcSpl_NormW32"""
    a = s32(a)
    x = u32(np.where(a < 0, ~a, a))
    z = np.where((x & 0xFFFF8000) == 0, 16, 0)
    z = z + np.where((u32(x << z) & 0xFF800000) == 0, 8, 0)
    z = z + np.where((u32(x << z) & 0xF8000000) == 0, 4, 0)
    z = z + np.where((u32(x << z) & 0xE0000000) == 0, 2, 0)
    z = z + np.where((u32(x << z) & 0xC0000000) == 0, 1, 0)
    return np.where(a == 0, 0, z)


def ref_norm_u32(a):
    """spl_inl.h WebRtcSpl_NormU32"""
    x = u32(a)
    z = np.where((x & 0xFFFF0000) == 0, 16, 0)
    z = z + np.where((u32(x << z) & 0xFF000000) == 0, 8, 0)
    z = z + np.where((u32(x << z) & 0xF0000000) == 0, 4, 0)
    z = z + np.where((u32(x << z) & 0xC0000000) == 0, 2, 0)
    z = z + np.where((u32(x << z) & 0x80000000) == 0, 1, 0)
    return np.where(x == 0, 0, z)


def ref_norm_w16(a):
    """spl_inl.h WebRtcSpl_NormW16; `a << zeros` is an int: no bits are lost before the mask"""
    a = s16(a)
    x = np.where(a < 0, ~a, a)
    z = np.where((x & 0xFF80) == 0, 8, 0)
    z = z + np.where(((x << z) & 0xF800) == 0, 4, 0)
    z = z + np.where(((x << z) & 0xE000) == 0, 2, 0)
    z = z + np.where(((x << z) & 0xC000) == 0, 1, 0)
    return np.where(a == 0, 0, z)


def ref_size_in_bits(a):
    """spl_inl.h WebRtcSpl_GetSizeInBits"""
    n = u32(a)
    bits = np.where(n & 0xFFFF0000, 16, 0)
    bits = bits + np.where((n >> bits) & 0x0000FF00, 8, 0)
    bits = bits + np.where((n >> bits) & 0x000000F0, 4, 0)
    bits = bits + np.where((n >> bits) & 0x0000000C, 2, 0)
    bits = bits + np.where((n >> bits) & 0x00000002, 1, 0)
    bits = bits + np.where((n >> bits) & 0x00000001, 1, 0)
    return bits


def ref_div_w32_w16(a, b):
    """division_operations.c WebRtcSpl_DivW32W16: C's division truncates towards zero; 0x7FFFFFFF for a zero divisor"""
    num, den = s32(a), s16(b)
    d = np.where(den == 0, 1, den)
    q = np.abs(num) // np.abs(d)
    q = np.where((num < 0) != (d < 0), -q, q)
    assert not np.any((num == DIV_EXCLUDED[0]) & (den == DIV_EXCLUDED[1]))
    return np.where(den == 0, INT32_MAX, q)


def ref_div_u32_u16(a, b):
    """division_operations.c WebRtcSpl_DivU32U16; 0xFFFFFFFF for a zero divisor.  Returned as the int32 with the same bits."""
    num, den = u32(a), u16(b)
    return s32(np.where(den == 0, 0xFFFFFFFF, num // np.where(den == 0, 1, den)))


def ref_sqrt_floor(a):
    """floor(sqrt(value)) for value > 0 and 0 otherwise, which is what spl_sqrt_floor.c's sixteen steps compute"""
    return np.array([math.isqrt(v) if v > 0 else 0 for v in s32(a).tolist()], dtype=np.int64)


def _ref_sqrt_local(a):
    """spl_sqrt.c WebRtcSpl_SqrtLocal"""
    b = np.where(a >= 0, a >> 1, -((-a) >> 1))  # in / 2 truncates towards zero
    b = s32(b - 0x40000000)
    x_half = s16(b >> 16)
    b = s32(b + 0x40000000)
    b = s32(b + 0x40000000)
    x2 = s32(s32(x_half * x_half) * 2)
    a = s32(-x2)
    b = s32(b + (a >> 1))
    a = a >> 16
    a = s32(s32(a * a) * 2)
    t16 = s16(a >> 16)
    b = s32(b + s32(-20480 * t16 * 2))
    a = s32(x_half * t16 * 2)
    t16 = s16(a >> 16)
    b = s32(b + s32(28672 * t16 * 2))
    t16 = s16(x2 >> 16)
    a = s32(x_half * t16 * 2)
    b = s32(b + (a >> 1))
    return s32(b + 32768)


def ref_spl_sqrt(value):
    """spl_sqrt.c WebRtcSpl_Sqrt"""
    value = s32(value)
    sh = ref_norm_w32(value)
    a = s32(value << sh)
    a = np.where(a < INT32_MAX - 32767, a + 32768, INT32_MAX)
    x_norm = s16(a >> 16)
    nshift = sh // 2
    a = s32(x_norm << 16)
    a = np.where(a >= 0, a, s32(-a))  # WEBRTC_SPL_ABS_W32: INT32_MIN stays
    a = _ref_sqrt_local(a)
    even = s32(s32(23170 * s16(a >> 16) * 2) + 32768)
    even = (even & 0x7FFF0000) >> 15
    a = np.where(2 * nshift == sh, even, a >> 16)
    a = (a & 0xFFFF) >> nshift
    return np.where(value == 0, 0, a)


def ref_mul_rsft_round(a, b, c):
    """signal_processing_library.h WEBRTC_SPL_MUL_16_16_RSFT_WITH_ROUND"""
    c = s32(c)
    return s32(s16(a) * s16(b) + (np.int64(1) << (c - 1))) >> c


def ref_agc_scalediff32(a, b, c):
    """digital_agc.h AGC_SCALEDIFF32: (C) + ((B)>>16)*(A) + (((0x0000FFFF & (B))*(A)) >> 16), all in int32"""
    a, b, c = s32(a), s32(b), s32(c)
    return s32(c + s32((b >> 16) * a) + (s32((b & 0xFFFF) * a) >> 16))


def ref_agc_mul32(a, b):
    """digital_agc.h AGC_MUL32: ((B)>>13)*(A) + (((0x00001FFF & (B))*(A)) >> 13), all in int32"""
    a, b = s32(a), s32(b)
    return s32(s32((b >> 13) * a) + (s32((b & 0x1FFF) * a) >> 13))


def ref_spl_scalediff32(a, b, c):
    """signal_processing_library.h WEBRTC_SPL_SCALEDIFF32: the low half's product and its shift are uint32"""
    a, b, c = s32(a), s32(b), s32(c)
    return s32(c + s32((b >> 16) * a) + (u32((b & 0xFFFF) * u32(a)) >> 16))


def ref_pk_abs16(a):
    """|x| of both int16 halves as uint16: 32768 for -32768"""
    a = u32(a)
    return s32(np.abs(s16(a)) | (np.abs(s16(a >> 16)) << 16))


def ref_pk_max_u16(a, b):
    a, b = u32(a), u32(b)
    return s32(np.maximum(a & 0xFFFF, b & 0xFFFF) | (np.maximum(a >> 16, b >> 16) << 16))


NUMPY_REFS = {"norm_w16": ref_norm_w16, "norm_w32": ref_norm_w32, "norm_u32": ref_norm_u32, "size_in_bits": ref_size_in_bits,
              "div_w32_w16": ref_div_w32_w16, "div_u32_u16": ref_div_u32_u16, "sqrt_floor": ref_sqrt_floor, "spl_sqrt": ref_spl_sqrt,
              "mul_rsft_round": ref_mul_rsft_round, "agc_scalediff32": ref_agc_scalediff32, "agc_mul32": ref_agc_mul32,
              "spl_scalediff32": ref_spl_scalediff32, "pk_abs16": ref_pk_abs16, "pk_max_u16": ref_pk_max_u16}


@functools.lru_cache(None)
def numpy_reference(name):
    args = [x for x in arguments(name) if x is not None]
    return _frozen(NUMPY_REFS[name](*args))


_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_i16p = np.ctypeslib.ndpointer(np.int16, flags="C_CONTIGUOUS")


def lib_sweep(lib, fn, kind, a, b=None):
    """orc_spl_sweep (oracle/orc_spl.c) or ref_spl_sweep (oracle/ref_shim.c) on whole arrays"""
    f = getattr(lib, fn)
    f.restype, f.argtypes = C.c_int, [C.c_int, _i32p, C.c_void_p, _i32p, C.c_size_t]
    y = np.zeros(a.size, np.int32)
    assert f(kind, a, None if b is None else b.ctypes.data, y, a.size) == 0
    return y


_oracle_cache = {}


def reference(name, oracle_port):
    """What the device is held to: the oracle's export where it has one, the numpy reference elsewhere."""
    if name not in ORC_SWEEP:
        return numpy_reference(name)
    if name not in _oracle_cache:
        a, b, _ = arguments(name)
        _oracle_cache[name] = _frozen(lib_sweep(oracle_port, "orc_spl_sweep", ORC_SWEEP[name], a, b))
    return _oracle_cache[name]


# ---------------------------------------------------------------- wave reductions
@functools.lru_cache(None)
def wave_rows():
    """[rows][64] int32: the extreme (largest, smallest, read signed or unsigned) in lane r of row r; the same for the second extreme,
    the first sitting elsewhere; rows of all-equal values; rows of INT32_MIN, INT32_MAX, 0 and 0xFFFFFFFF; 256 random rows."""
    rng = np.random.default_rng(120)
    rows = []
    lanes = np.arange(64)
    other = (lanes + 1 + 9 * (lanes % 5)) % 64  # a lane that is not r, moving through all rows of 16 and all positions in them
    assert not np.any(other == lanes)
    # (range of the other 63 lanes, the extreme, the second extreme)
    for lo, hi, first, second in ((-10**6, 10**6, 2 * 10**9, 15 * 10**8),       # largest signed (and unsigned among non-negatives)
                                  (-10**6, 10**6, -2 * 10**9, -15 * 10**8),     # smallest signed
                                  (10**3, 10**6, -16, -4096),                    # largest unsigned: 0xFFFFFFF0, 0xFFFFF000; negative signed
                                  (10**3, 10**6, 0, 1),                          # smallest unsigned and smallest non-negative
                                  (-10**6, -10**3, INT32_MIN, INT32_MIN + 1),    # smallest unsigned among the negatives
                                  (-10**6, -10**3, INT32_MAX, INT32_MAX - 1)):
        base = rng.integers(lo, hi, size=(64, 64), dtype=np.int64)
        one = base.copy()
        one[lanes, lanes] = first
        two = base.copy()
        two[lanes, lanes] = second
        two[lanes, other] = first
        rows += [one, two]
    rows.append(np.repeat(np.array([0, 1, -1, INT32_MIN, INT32_MAX, 12345], np.int64)[:, None], 64, axis=1))
    four = np.array([INT32_MIN, INT32_MAX, 0, -1], np.int64)
    rows.append(four[rng.integers(0, 4, size=(8, 64))])
    planted = rng.integers(INT32_MIN, INT32_MAX + 1, size=(8, 64), dtype=np.int64)
    for r in range(8):
        planted[r, rng.permutation(64)[:4]] = four
    rows.append(planted)
    rows.append(rng.integers(INT32_MIN, INT32_MAX + 1, size=(256, 64), dtype=np.int64))
    return _frozen(np.concatenate(rows))


@functools.lru_cache(None)
def wave_reference(name):
    """[rows][64]: the row's result in every lane"""
    x = wave_rows().astype(np.int64)
    if name == "wave_sum":
        r = s32(u32(x).sum(axis=1))  # the sum mod 2^32
    elif name == "wave_max":
        r = x.max(axis=1)
    elif name == "wave_min":
        r = x.min(axis=1)
    elif name == "wave_umax":
        r = s32(u32(x).max(axis=1))
    else:
        r = s32(u32(x).min(axis=1))
    return _frozen(np.repeat(r[:, None], 64, axis=1))


# ---------------------------------------------------------------- the SPL real FFTs
GOLDEN_AMPS = (0, 1, 7, 60, 500, 4000, 12000, 13573, 16384, 27146, 30000, 32767)  # tests/golden/make_nsx_golden.py
LOUD_VALUES = (13572, 13573, 13574, 27145, 27146, 27147, 32767, -32768, -13574, -27147)  # around complex_fft.c's two thresholds
FLOOR_AMPS = (0, 3, 300, 3000)
NOISE_AMPS = (0, 1, 50, 400, 1500, 3000, 6000, 12000, 20000, 32767)
HI, LO = 32767, -32768


def _clip16(x):
    return np.clip(x, LO, HI).astype(np.int16)


@functools.lru_cache(None)
def fft_forward_inputs(order):
    """[k][n] int16: zeros, an impulse at every position with 32767 and with -32768, constant full scale, alternating 32767 / -32768,
    square waves of period 2 .. n, Gaussian noise at the golden's twelve amplitudes x 16 seeds"""
    n = 1 << order
    i = np.arange(n)
    rows = [np.zeros((1, n), np.int64), np.eye(n, dtype=np.int64) * HI, np.eye(n, dtype=np.int64) * LO,
            np.full((1, n), HI), np.full((1, n), LO), np.where(i % 2 == 0, HI, LO)[None], np.where(i % 2 == 0, LO, HI)[None],
            np.stack([np.where(i % p < (p + 1) // 2, HI, LO) for p in range(2, n + 1)])]
    for ai, amp in enumerate(GOLDEN_AMPS):
        for seed in range(16):
            rng = np.random.default_rng((70, order, ai, seed))
            rows.append(np.clip(rng.standard_normal((1, n)) * amp / 2.5, LO, HI).astype(np.int64))
    return _frozen(np.concatenate(rows), np.int16)


def orc_fft(oracle_port, order, x):
    """orc_spl_real_fft on [k][n] -> [k][n + 2]"""
    n = 1 << order
    f = oracle_port.orc_spl_real_fft_batch
    f.restype, f.argtypes = None, [C.c_int, C.c_int, _i16p, _i16p]
    out = np.zeros((x.shape[0], n + 2), np.int16)
    f(order, x.shape[0], np.ascontiguousarray(x), out)
    return out


def orc_ifft(oracle_port, order, spec):
    """orc_spl_real_ifft on [k][n + 2] -> ([k][n], [k] scale counts)"""
    n = 1 << order
    f = oracle_port.orc_spl_real_ifft_batch
    f.restype, f.argtypes = None, [C.c_int, C.c_int, _i16p, _i16p, _i32p]
    out, sc = np.zeros((spec.shape[0], n), np.int16), np.zeros(spec.shape[0], np.int32)
    f(order, spec.shape[0], np.ascontiguousarray(spec), out, sc)
    return out, sc


def ref_fft(oracle_ref, order, x):
    n = 1 << order
    f = oracle_ref.ref_spl_real_fft_batch
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_int, _i16p, _i16p]
    out = np.zeros((x.shape[0], n + 2), np.int16)
    assert f(order, x.shape[0], np.ascontiguousarray(x), out) == 0
    return out


def ref_ifft(oracle_ref, order, spec):
    n = 1 << order
    f = oracle_ref.ref_spl_real_ifft_batch
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_int, _i16p, _i16p, _i32p]
    out, sc = np.zeros((spec.shape[0], n), np.int16), np.zeros(spec.shape[0], np.int32)
    assert f(order, spec.shape[0], np.ascontiguousarray(spec), out, sc) == 0
    return out, sc


_fft_cache = {}


def fft_inverse_families(order, oracle_port):
    """{"a": .., "b": .., "c": ..}, each [k][n + 2] int16 (n / 2 + 1 bins, real and imaginary part interleaved).
    a: the oracle's forward outputs of fft_forward_inputs, scaled by 1, 2, 4 and 8 and clipped.
    b: one loud component -- the real or the imaginary part of bin 0, 1, n / 4, n / 2 - 1 or n / 2, set to each of LOUD_VALUES -- over a
       floor of uniform noise within +-FLOOR_AMPS: the array's largest |value| sits exactly on, one below and one above the inverse
       transform's two thresholds.  The imaginary parts of bins 0 and n / 2 are set like any other: real_fft.c copies them as they are.
    c: noise spectra at NOISE_AMPS x 50 seeds."""
    key = ("inv", order)
    if key not in _fft_cache:
        n = 1 << order
        fwd = orc_fft(oracle_port, order, fft_forward_inputs(order)).astype(np.int64)
        fam = {"a": _clip16(np.concatenate([fwd * k for k in (1, 2, 4, 8)]))}
        rows = []
        for fi, floor in enumerate(FLOOR_AMPS):
            rng = np.random.default_rng((73, order, fi))
            for value in LOUD_VALUES:
                for b in (0, 1, n // 4, n // 2 - 1, n // 2):
                    for part in (0, 1):
                        row = rng.integers(-floor, floor + 1, size=n + 2, dtype=np.int64)
                        row[2 * b + part] = value
                        rows.append(row)
        fam["b"] = _clip16(np.stack(rows))
        rows = []
        for ai, amp in enumerate(NOISE_AMPS):
            for seed in range(50):
                rng = np.random.default_rng((75, order, ai, seed))
                rows.append(np.clip(rng.standard_normal(n + 2) * amp / 2.5, LO, HI))
        fam["c"] = _clip16(np.stack(rows))
        for v in fam.values():
            v.setflags(write=False)
        _fft_cache[key] = fam
    return _fft_cache[key]


def fft_inverse_inputs(order, oracle_port):
    fam = fft_inverse_families(order, oracle_port)
    return np.concatenate([fam["a"], fam["b"], fam["c"]])


def fft_oracle_answers(order, oracle_port):
    """(forward inputs, forward outputs, inverse inputs, inverse outputs, scale counts) of the oracle, computed once"""
    key = ("ans", order)
    if key not in _fft_cache:
        x = fft_forward_inputs(order)
        spec = fft_inverse_inputs(order, oracle_port)
        out, sc = orc_ifft(oracle_port, order, spec)
        ans = (x, orc_fft(oracle_port, order, x), spec, out, sc)
        for v in ans:
            v.setflags(write=False)
        _fft_cache[key] = ans
    return _fft_cache[key]


def assert_scale_counts_covered(order, oracle_port):
    """The condition on the inverse inputs, asserted on the ORACLE's results so that a later change of inputs cannot hollow the tests:
    the scale count takes every value 0 .. 6; family b alone 0 .. 4, family c 0 .. 6."""
    fam = fft_inverse_families(order, oracle_port)
    got = {k: set(orc_ifft(oracle_port, order, v)[1].tolist()) for k, v in fam.items()}
    assert set(range(5)) <= got["b"], (order, got)
    assert set(range(7)) <= got["c"], (order, got)
    assert set(range(7)) <= set(fft_oracle_answers(order, oracle_port)[4].tolist())
