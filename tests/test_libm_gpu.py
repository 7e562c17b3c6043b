"""GPU: the scalar math routines under the float NS and AEC (wmix_amd/csrc/libm_dev.h, sqrtf), run ON THE DEVICE through
wmx_debug_ns_libm_device (compiled in ns.hip, tables in LDS as ns_kernel holds them) and wmx_debug_aec_libm_device (compiled in
aec.hip), one launch per test, every result compared bit for bit:

  A  fast_log_ge1 / fast_exp / tanh_call on the very vectors of the host sweeps (tests/test_libm_tables.py), against the host
     evaluation of the same source and against glibc.  Device and host run the same IEEE operations; what differs is how they
     are spelled (fma_c's inline v_fma_f64, LDS tables, the compiler's fp64 conversions and division, float-subnormal results).
  B  log_d / exp_d / div_pow_d, which are ocml's fp64 log / exp / pow, on the domains their call sites produce, against glibc.
     That two libraries agree bit for bit is demanded only where it follows from their error bounds: a test without a GPU
     shows that no double result of glibc lies within 8 double ulps of a float rounding boundary.
  C  sqrtf from both translation units against the correctly rounded square root.
  D  the hooks' argument checks.
A also compares the DOUBLE each table-driven routine holds before its rounding, device against host, all 64 bits: the float results
cannot show an error of an ulp of double (one argument in 2^28 would), which is the size of error a wrong table entry makes."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_libm_tables import _exp_arguments, _log_arguments, _product, _run, _tanh_arguments

EINVAL = -10001
K_START_BAND = 5      # ns.hip kStartBand (ns_core.c:1045)
BINS = (65, 129)      # M = L / 2 + 1 of the two frame sizes, L = 128 (8 kHz) and 256 (16 / 32 kHz)
SEED = 21


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _ns_device(wmx, cuda, kind, x, a=None, b=None):
    import torch
    up = lambda v: None if v is None else torch.tensor(v).to(cuda)  # noqa: E731  (a copy: the shared vectors are read-only)
    dx, da, db = up(x), up(a), up(b)
    dy = torch.empty_like(dx)
    adr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = wmx.wmx_debug_ns_libm_device(kind, dx.data_ptr(), adr(da), adr(db), dy.data_ptr(), x.size, None)
    assert rc == 0, (rc, wmx.wmx_last_error())
    return dy.cpu().numpy()


def _aec_device(wmx, cuda, kind, x):
    import torch
    dx = torch.tensor(x).to(cuda)
    dy = torch.empty_like(dx)
    rc = wmx.wmx_debug_aec_libm_device(kind, dx.data_ptr(), dy.data_ptr(), x.size, None)
    assert rc == 0, (rc, wmx.wmx_last_error())
    return dy.cpu().numpy()


def _assert_same_floats(got, want, x, what):
    """NaN where the expected value is NaN, the same bits everywhere else; the first differing arguments in the message."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN-ness differs at x = %s" % (what, x[np.isnan(got) != nan][:8])
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
    assert bad.size == 0, "%s: %d of %d differ; x, got, want (bits) = %s" % (
        what, bad.size, x.size, [(float(x[i]), hex(got.view(np.uint32)[i]), hex(want.view(np.uint32)[i])) for i in bad[:8]])


# ---------------------------------------------------------------- A: the table-driven routines
@pytest.mark.gpu
@pytest.mark.parametrize("kind,arguments,oracle", [(0, _log_arguments, "orc_libm_log"), (1, _exp_arguments, "orc_libm_exp"),
                                                   (2, _tanh_arguments, "orc_libm_tanh")], ids=["log", "exp", "tanh"])
def test_table_driven_routine_on_the_device(wmx, cuda, oracle_port, kind, arguments, oracle):
    """The 12.0 M / 11.0 M / 9.0 M arguments of test_log_sweep / test_exp_sweep / test_tanh_sweep -- the first 4096 floats above 1,
    the float-subnormal exp results, the specials that go down slow_log / slow_exp to ocml -- through the device.  No tolerance."""
    x = arguments()
    got = _ns_device(wmx, cuda, kind, x)
    with np.errstate(all="ignore"):
        host, want = _product(wmx, kind, x), _run(getattr(oracle_port, oracle), x)
    _assert_same_floats(got, host, x, "device against the host evaluation of the same source")
    _assert_same_floats(got, want, x, "device against glibc")


def _host_doubles(wmx, kind, x):
    y = np.zeros(x.size, np.float64)
    assert wmx.wmx_debug_ns_libm_dbl(kind, x.ctypes.data, y.ctypes.data, x.size) == 0
    return y


_ARGUMENTS = [(0, _log_arguments), (1, _exp_arguments), (2, _tanh_arguments)]


@pytest.mark.parametrize("kind,arguments", _ARGUMENTS, ids=["log", "exp", "tanh"])
def test_the_double_cores_are_the_routines_before_their_rounding(wmx, kind, arguments):
    """wmx_debug_ns_libm_dbl hands out what the routine rounds: inside the guard (all arguments but the specials and, for tanh, the saturated |x| >= 20) the double,
    rounded to float (tanh: with the argument's sign), is the routine's float; outside it is NaN."""
    x = arguments()
    with np.errstate(all="ignore"):
        dbl, flt = _host_doubles(wmx, kind, x), _product(wmx, kind, x)
        inside = [(x >= 1) & (x < np.float32(3.0e38)), np.abs(x) < 700, np.abs(x) < 20][kind]
        assert np.array_equal(np.isnan(dbl), ~inside) and inside.mean() > 0.9
        rounded = dbl.astype(np.float32)
    if kind == 2:
        rounded = np.copysign(rounded, x)
    assert np.array_equal(rounded.view(np.uint32)[inside], flt.view(np.uint32)[inside])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,arguments", _ARGUMENTS, ids=["log", "exp", "tanh"])
def test_table_driven_routine_before_its_rounding_on_the_device(wmx, cuda, kind, arguments):
    """The same vectors, the DOUBLE each routine holds before it rounds, device against host, all 64 bits.  The floats above hide
    an error of an ulp of double in all but one argument of 2^28: with one logtab entry an ulp off in the kernel's LDS copy every
    float of the 12 M still agrees, and this test fails on every argument that reads the entry (tried).  Same source, same IEEE
    operations, same tables: the doubles are equal, or the device path is not what the host sweep proved.  What even this
    cannot see is an error that the Horner steps behind it shrink below the last bit: fma_c's device branch as a multiplication
    and an addition (two roundings) changes no double of the 32 M (tried) -- each step multiplies an earlier step's ulp by
    r < 2^-7, so after two or three of them the result moves in fewer arguments than were swept."""
    import torch
    x = arguments()
    dx = torch.tensor(x).to(cuda)
    dy = torch.empty(x.size, dtype=torch.float64, device=cuda)
    rc = wmx.wmx_debug_ns_libm_dbl_device(kind, dx.data_ptr(), dy.data_ptr(), x.size, None)
    assert rc == 0, (rc, wmx.wmx_last_error())
    got = dy.cpu().numpy()
    with np.errstate(all="ignore"):
        want = _host_doubles(wmx, kind, x)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and nan.mean() < 0.1
    bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)) & ~nan)
    assert bad.size == 0, "%d of %d doubles differ; x, device, host = %s" % (
        bad.size, x.size, [(float(x[i]), hex(got.view(np.uint64)[i]), hex(want.view(np.uint64)[i])) for i in bad[:8]])


# ---------------------------------------------------------------- B: the ocml-backed routines
N_B = 4_000_000


@functools.lru_cache(None)
def _log_d_arguments():
    """aec.hip: overDrive comes from log_d(hNlFbMin + 1e-10f), hNlFbMin the minimum of coherence-derived suppression gains, in (0, 1]
    (aec_core.c OverdriveAndSuppress).  Half uniform, a quarter within 1e-2 below 1 (a converged filter without echo), a quarter
    log-uniform down to e^-23 ~ 1e-10, where the added constant takes over; 1.0 itself; and what the call site never produces but
    the library decides by rule: 0, a subnormal, inf, NaN."""
    rng = np.random.default_rng(SEED)
    h = np.concatenate([1 - rng.random(N_B // 2), 1 - rng.random(N_B // 4) * 1e-2, np.exp(-rng.random(N_B // 4) * 23), [1.0]]).astype(np.float32)
    x = h + np.float32(1e-10)  # in float, as the kernel adds it
    return np.concatenate([x, np.array([0.0, 1e-40, np.inf, np.nan], np.float32)])


@functools.lru_cache(None)
def _exp_d_arguments():
    """ns.hip: pnum = exp_d(pink_num / (block_ind + 1)), the running mean of a regression intercept of log magnitudes that is clamped
    at 0 from below (ns_core.c:1111-1130); log(|X| + 1) of a 16-bit spectrum stays below 17, the intercept within [0, 24]."""
    rng = np.random.default_rng(SEED + 1)
    return np.concatenate([rng.random(N_B * 3 // 4) * 24, rng.random(N_B // 4) * 1e-3, [0.0]]).astype(np.float32)


@functools.lru_cache(None)
def _div_pow_arguments():
    """ns.hip: pn = div_pow_d(pnum, band, pexp).  pnum = exp_d(..) * (block_ind + 1) with block_ind + 1 in 1 .. 50 (kStartupShort);
    band = (float)max(bin, kStartBand) for bins up to M - 1, M = 65 or 129; pexp = pink_exp / (block_ind + 1), the mean of slopes
    clamped to [0, 1] and used only when positive: (0, 1], down to almost nothing after one small slope, and 1 exactly."""
    rng = np.random.default_rng(SEED + 2)
    n = N_B
    num = np.exp(rng.random(n) * 20) * rng.integers(1, 51, n)
    base = np.where(np.arange(n) % 2 == 0, rng.integers(K_START_BAND, BINS[0], n), rng.integers(K_START_BAND, BINS[1], n))
    e = 1 - rng.random(n)  # (0, 1]
    e[n - n // 8: n - n // 16] = 1.0
    e[n - n // 16:] = np.resize(np.array([1e-10, 1e-30, 1e-40]), n // 16)  # the last one is a float subnormal
    return tuple(np.ascontiguousarray(v, np.float32) for v in (num, base, e))


def _boundary_margin(d):
    """Smallest distance, in double ulps, of the finite non-zero doubles `d` from the nearest midpoint between two adjacent floats.
    For a double in the floats' normal range the float keeps the top 23 of its 52 mantissa bits; the rounding boundary is the
    pattern 1000...0 in the 29 bits below, in every binade (the midpoint under a power of two included)."""
    d = d[np.isfinite(d) & (d != 0)]
    a = np.abs(d)
    assert a.min() >= 2.0 ** -126 and a.max() < 2.0 ** 127, "outside the floats' normal range the formula below does not hold"
    low = (d.view(np.uint64) & np.uint64((1 << 29) - 1)).astype(np.int64)
    return int(np.abs(low - (1 << 28)).min())


@functools.lru_cache(None)
def _ocml_case(name):
    """(arguments, glibc's floats, glibc's doubles) of one routine; computed once, shared by the margin test and the device test"""
    from oracle import loader
    port = loader.port()
    args = {"log": (_log_d_arguments(),), "exp": (_exp_d_arguments(),), "div_pow": _div_pow_arguments()}[name]
    n = args[0].size
    flt, dbl = np.zeros(n, np.float32), np.zeros(n, np.float64)
    with np.errstate(all="ignore"):
        getattr(port, "orc_libm_" + name)(*[_ptr(a) for a in args], _ptr(flt), C.c_size_t(n))
        getattr(port, "orc_libm_%s_dbl" % name)(*[_ptr(a) for a in args], _ptr(dbl), C.c_size_t(n))
    for v in args + (flt, dbl):
        v.setflags(write=False)
    return args, flt, dbl


@pytest.mark.parametrize("name", ["log", "exp", "div_pow"])
def test_glibc_results_keep_clear_of_float_rounding_boundaries(name):
    """Why bit equality may be demanded of ANOTHER library on these vectors: glibc's log, exp and pow are good to < 1 ulp of
    double, ocml's to a few; two doubles that each lie within a few ulps of the true value round to different floats only when a
    float rounding boundary lies between them.  Here no result of glibc comes within 8 double ulps of one, so every double within
    8 ulps of it -- ocml's included, unless it is outside its own error bound -- rounds to the same float.  Decided by the
    reference alone; a vector that fails this gets another seed, whatever the device says.  Measured (seeds 21, 22, 23): the
    closest results
    are 21 (log), 21 (exp) and 96 (div_pow) double ulps from a boundary.  Also checks that the float the oracle returns is the rounded
    double (the two entry points restate one expression)."""
    args, flt, dbl = _ocml_case(name)
    with np.errstate(all="ignore"):
        assert np.array_equal(dbl.astype(np.float32).view(np.uint32)[~np.isnan(dbl)], flt.view(np.uint32)[~np.isnan(dbl)])
    margin = _boundary_margin(dbl)
    print("%s: %d arguments, closest double result %d ulps from a float rounding boundary" % (name, args[0].size, margin))
    assert margin >= 8


@pytest.mark.gpu
def test_log_d_on_the_device(wmx, cuda):
    """ocml's fp64 log behind aec.hip's log_d, compiled in aec.hip: glibc's floats, bit for bit (-inf for 0, NaN for NaN)"""
    (x,), flt, _ = _ocml_case("log")
    _assert_same_floats(_aec_device(wmx, cuda, 0, x), flt, x, "log_d against glibc")


@pytest.mark.gpu
def test_exp_d_on_the_device(wmx, cuda):
    """ocml's fp64 exp behind ns.hip's exp_d: glibc's floats, bit for bit"""
    (x,), flt, _ = _ocml_case("exp")
    _assert_same_floats(_ns_device(wmx, cuda, 3, x), flt, x, "exp_d against glibc")


@pytest.mark.gpu
def test_div_pow_d_on_the_device(wmx, cuda):
    """num / pow(base, e) with ocml's fp64 pow and the compiler's fp64 division: glibc's floats, bit for bit"""
    (num, base, e), flt, _ = _ocml_case("div_pow")
    assert num.nbytes + base.nbytes + e.nbytes <= 48_000_000
    _assert_same_floats(_ns_device(wmx, cuda, 4, num, base, e), flt, num, "div_pow_d against glibc")


# ---------------------------------------------------------------- C: sqrtf
@functools.lru_cache(None)
def _sqrt_case():
    """10 M arguments and their correctly rounded roots (IEEE 754 requires it of the square root; numpy's float32 sqrt is the
    host's instruction).  Random normal floats over every exponent; what the kernels feed in -- re * re + im * im of the spectrum of
    a 16-bit frame (ns.hip magnitude, aec.hip |E|), the gain energy2 / (energy1 + 1) in [0, 4] (ns.hip), noise-floor powers
    (aec.hip comfort noise); every perfect square a float holds (a 12-bit mantissa squared, times 4^j) with its neighbours one ulp
    either side, where a root that is an ulp off shows; subnormals, which the device's v_sqrt_f32 does not take as they are; and
    the arguments decided by rule."""
    rng = np.random.default_rng(SEED + 3)
    f32 = np.float32
    re, im = ((rng.random(2_000_000) * 2 - 1) * 32768 * 128).astype(f32), ((rng.random(2_000_000) * 2 - 1) * 32768 * 128).astype(f32)
    sq = (np.arange(2048, 4096, dtype=np.float64)[:, None] ** 2 * 4.0 ** np.arange(-70, 52)[None, :]).ravel().astype(f32)
    parts = [
        re * re + im * im, (rng.random(1_500_000) * 4).astype(f32), np.exp(rng.random(1_000_000) * 30 - 5).astype(f32),
        sq, np.nextafter(sq, f32(0)), np.nextafter(sq, f32(np.inf)),
        rng.integers(1, 0x00800000, 500_000, dtype=np.uint32).view(f32),
        np.array([0.0, -0.0, np.inf, -1.0, np.nan, 1e-45, 1.17549435e-38, 3.4028235e38, 1.0, 2.0, 4.0], f32),
    ]
    n = 10_000_000 - sum(p.size for p in parts)
    x = np.concatenate([rng.integers(0x00800000, 0x7F800000, n, dtype=np.uint32).view(f32)] + parts)
    assert x.size == 10_000_000 and x.dtype == f32
    with np.errstate(all="ignore"):
        want = np.sqrt(x)
    assert want.dtype == f32 and np.signbit(want[x.size - 10]) and want[x.size - 10] == 0  # sqrt(-0.0) = -0.0
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def test_the_expected_roots_are_correctly_rounded():
    """the reference of part C checked by itself, in double: sqrt of a float in double, rounded to float, is the correctly rounded
    float root (53 >= 2 * 24 + 2 bits), and numpy's float32 sqrt gives the same bits"""
    x, want = _sqrt_case()
    with np.errstate(all="ignore"):
        dbl = np.sqrt(x.astype(np.float64)).astype(np.float32)
    ok = ~np.isnan(dbl)
    assert np.array_equal(np.isnan(want), ~ok) and np.array_equal(want.view(np.uint32)[ok], dbl.view(np.uint32)[ok])


@pytest.mark.gpu
@pytest.mark.parametrize("unit", ["ns", "aec"])
def test_sqrtf_on_the_device(wmx, cuda, unit):
    """sqrtf as ns.hip (kind 5) and aec.hip (kind 1) compile it: the correctly rounded root, the sign of -0.0 kept, NaN for -1"""
    x, want = _sqrt_case()
    got = _ns_device(wmx, cuda, 5, x) if unit == "ns" else _aec_device(wmx, cuda, 1, x)
    _assert_same_floats(got, want, x, "sqrtf in %s.hip" % unit)


# ---------------------------------------------------------------- D: argument checks
@pytest.mark.gpu
def test_hooks_reject_bad_arguments(wmx, cuda):
    import torch
    t = torch.full((4,), 2.0, dtype=torch.float32, device=cuda)
    y = torch.full((4,), -7.0, dtype=torch.float32, device=cuda)
    p, q = t.data_ptr(), y.data_ptr()
    ns, aec = wmx.wmx_debug_ns_libm_device, wmx.wmx_debug_aec_libm_device
    assert ns(0, None, None, None, q, 4, None) == EINVAL and ns(0, p, None, None, None, 4, None) == EINVAL
    assert ns(4, p, None, p, q, 4, None) == EINVAL and ns(4, p, p, None, q, 4, None) == EINVAL
    assert ns(-1, p, p, p, q, 4, None) == EINVAL and ns(6, p, p, p, q, 4, None) == EINVAL
    assert aec(0, None, q, 4, None) == EINVAL and aec(0, p, None, 4, None) == EINVAL
    assert aec(-1, p, q, 4, None) == EINVAL and aec(2, p, q, 4, None) == EINVAL
    for kind in range(6):
        assert ns(kind, p, p, p, q, 0, None) == 0
    assert aec(0, p, q, 0, None) == 0 and aec(1, p, q, 0, None) == 0
    d = torch.full((4,), -7.0, dtype=torch.float64, device=cuda)
    dbl = wmx.wmx_debug_ns_libm_dbl_device
    assert dbl(0, None, d.data_ptr(), 4, None) == EINVAL and dbl(0, p, None, 4, None) == EINVAL
    assert dbl(-1, p, d.data_ptr(), 4, None) == EINVAL and dbl(3, p, d.data_ptr(), 4, None) == EINVAL
    assert dbl(0, p, d.data_ptr(), 0, None) == 0
    torch.cuda.synchronize()
    assert y.cpu().tolist() == [-7.0] * 4 and d.cpu().tolist() == [-7.0] * 4  # n == 0 and the refused calls wrote nothing
    assert ns(5, p, None, None, q, 4, None) == 0 and y.cpu().tolist() == [float(np.sqrt(np.float32(2.0)))] * 4
