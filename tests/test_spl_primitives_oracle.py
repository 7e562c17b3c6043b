"""CPU: the references that tests/test_spl_primitives_gpu.py holds the device to (tests/spl_inputs.py), checked against each other on
the whole argument sets: the numpy restatements of the WebRTC text against the oracle's exports and against plain Python integers,
and -- where oracle/_ref is built -- both against the real WebRtcSpl_SqrtFloor / Sqrt / DivW32W16 / DivU32U16 and the real
WebRtcSpl_RealForwardFFT / RealInverseFFT (through the whole-array drivers of oracle/ref_shim.c)."""
import numpy as np
import pytest

import spl_inputs as S


@pytest.mark.parametrize("name", sorted(S.ORC_SWEEP))
def test_numpy_reference_equals_the_oracle(oracle_port, name):
    assert np.array_equal(S.reference(name, oracle_port), S.numpy_reference(name))


def test_clz_references_equal_python_integers():
    """norm_w16 on its whole domain, the others on the edge set and 2^16 random words: int.bit_length knows no masks and shifts"""
    def norm(v, width):
        return 0 if v == 0 else width - 1 - (v if v >= 0 else ~v).bit_length()
    a16 = S.all16()
    assert S.ref_norm_w16(a16).tolist() == [norm(v, 16) for v in a16.tolist()]
    a = np.concatenate([S.edge32(), S.rand32(101)[:1 << 16]])
    assert S.ref_norm_w32(a).tolist() == [norm(v, 32) for v in a.tolist()]
    assert S.ref_norm_u32(a).tolist() == [0 if v == 0 else 32 - (v & 0xFFFFFFFF).bit_length() for v in a.tolist()]
    assert S.ref_size_in_bits(a).tolist() == [(v & 0xFFFFFFFF).bit_length() for v in a.tolist()]


def test_the_only_excluded_pair_is_int32_min_over_minus_one():
    """div_w32_w16 leaves out (INT32_MIN, -1), on which the reference's division traps; nothing else is dropped from any set"""
    grid = S.edge32().size * 65536
    a, b, _ = S.arguments("div_w32_w16")
    ua, ub, _ = S.arguments("div_u32_u16")
    assert ua.size == grid + (1 << 20) and a.size == ua.size - 1
    gone = np.flatnonzero((ua == S.DIV_EXCLUDED[0]) & (ub == S.DIV_EXCLUDED[1]))
    assert gone.size == 1 and gone[0] < grid
    assert np.array_equal(np.delete(ua, gone), a) and np.array_equal(np.delete(ub, gone), b)
    # the edge set is whole, and every other set is what its builder concatenated
    e = set(S.edge32().tolist())
    assert {0, 1, -1, S.INT32_MIN, S.INT32_MAX} <= e
    assert all(s * (2**k + d) in e for k in range(1, 32) for d in (-1, 0, 1) for s in (1, -1) if S.INT32_MIN <= s * (2**k + d) <= S.INT32_MAX)
    one = 65536 + S.edge32().size + (1 << 20)
    for name in ("norm_w16", "norm_w32", "norm_u32", "size_in_bits", "spl_sqrt"):
        assert S.arguments(name)[0].size == one
    assert S.arguments("sqrt_floor")[0].size == one + 3 * 46341 + 2
    # zero and negative divisors, all of them, against every edge numerator
    assert np.array_equal(np.unique(b[:grid - 1]), np.arange(-32768, 32768))


@pytest.mark.parametrize("name", sorted(S.REF_SWEEP))
def test_reference_equals_the_real_spl_routine(oracle_port, oracle_ref, name):
    if not hasattr(oracle_ref, "ref_spl_sweep"):
        pytest.skip("oracle/_ref/libwmixref.so was built before oracle/ref_shim.c had ref_spl_sweep")
    a, b, _ = S.arguments(name)
    got = S.lib_sweep(oracle_ref, "ref_spl_sweep", S.REF_SWEEP[name], a, b)
    assert np.array_equal(got, S.reference(name, oracle_port))
    assert np.array_equal(got, S.numpy_reference(name))


@pytest.mark.parametrize("order", [7, 8])
def test_inverse_fft_inputs_reach_every_scale_count(oracle_port, order):
    S.assert_scale_counts_covered(order, oracle_port)
    x, fwd, spec, out, sc = S.fft_oracle_answers(order, oracle_port)
    n = 1 << order
    assert x.shape == (1 + 2 * n + 2 + 2 + (n - 1) + 12 * 16, n) and spec.shape == (4 * x.shape[0] + 400 + 500, n + 2)
    # family b puts the array's largest |value| on the thresholds themselves: the loud component is the maximum of its row
    b = S.fft_inverse_families(order, oracle_port)["b"].astype(np.int64)
    assert sorted(set(np.abs(b).max(axis=1).tolist())) == sorted(set(abs(v) for v in S.LOUD_VALUES))


@pytest.mark.parametrize("order", [7, 8])
def test_oracle_fft_equals_the_real_spl_fft(oracle_port, oracle_ref, order):
    if not hasattr(oracle_ref, "ref_spl_real_ifft_batch"):
        pytest.skip("oracle/_ref/libwmixref.so was built before oracle/ref_shim.c had ref_spl_real_ifft_batch")
    x, fwd, spec, out, sc = S.fft_oracle_answers(order, oracle_port)
    assert np.array_equal(S.ref_fft(oracle_ref, order, x), fwd)
    got, got_sc = S.ref_ifft(oracle_ref, order, spec)
    assert np.array_equal(got_sc, sc) and np.array_equal(got, out)
