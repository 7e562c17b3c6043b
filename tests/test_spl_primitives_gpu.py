"""GPU: the fixed-point primitives every bit-exact integer kernel stands on (spl_dev.h, spl_fx.h), stand-alone on the device
(wmx_debug_spl), and the SPL real FFT executors (wmx_debug_fft kinds 8 .. 13), bit for bit against the references of
tests/spl_inputs.py: the oracle, math.isqrt, and numpy integers written from the WebRTC text.  No tolerance anywhere.  The references
are held to each other and to the real reference routines on the CPU (tests/test_spl_primitives_oracle.py); oracle/_ref is not read
here."""
import numpy as np
import pytest
import torch

import spl_inputs as S

pytestmark = pytest.mark.gpu


def dev(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a)).to(cuda)


def ptr(t):
    return None if t is None else t.data_ptr()


def run_spl(wmx, cuda, kind, a, b=None, c=None):
    da, db, dc = dev(cuda, a), dev(cuda, b), dev(cuda, c)
    y = torch.full((a.size,), 0x5A5A5A5A, dtype=torch.int32, device=cuda)
    assert wmx.wmx_debug_spl(kind, ptr(da), ptr(db), ptr(dc), y.data_ptr(), a.size, None) == 0
    return y.cpu().numpy().reshape(a.shape)


def first_difference(got, want, *operands):
    """None, or the first differing element with its operands (an assertion message a reader can act on)"""
    bad = np.flatnonzero(got.ravel() != want.ravel())
    if bad.size == 0:
        return None
    i = int(bad[0])
    return "%d of %d differ; first at %d: operands %s, got %d, want %d" % (
        bad.size, got.size, i, [int(o.ravel()[i]) for o in operands if o is not None], int(got.ravel()[i]), int(want.ravel()[i]))


@pytest.mark.parametrize("name", list(S.KINDS))
def test_primitive_on_the_device(wmx, cuda, oracle_port, name):
    a, b, c = S.arguments(name)
    want = S.reference(name, oracle_port)
    got = run_spl(wmx, cuda, S.KINDS[name], a, b, c)
    assert first_difference(got, want, a, b, c) is None


@pytest.mark.parametrize("name", list(S.WAVE_KINDS))
def test_wave_reduction_on_the_device(wmx, cuda, name):
    x = S.wave_rows()
    got = run_spl(wmx, cuda, S.WAVE_KINDS[name], x)
    assert first_difference(got, S.wave_reference(name), x) is None  # every lane of every row: the result is wave-uniform
    # a short batch, where a row's place in the grid is not its place in the whole set
    got = run_spl(wmx, cuda, S.WAVE_KINDS[name], x[600:637])
    assert first_difference(got, S.wave_reference(name)[600:637], x[600:637]) is None


def test_hook_refuses_what_it_does_not_know(wmx, cuda):
    a = dev(cuda, np.zeros(128, np.int32))
    y = torch.zeros(128, dtype=torch.int32, device=cuda)
    for kind in (-1, 14, 15, 21):
        assert wmx.wmx_debug_spl(kind, a.data_ptr(), a.data_ptr(), a.data_ptr(), y.data_ptr(), 128, None) != 0
    assert wmx.wmx_debug_spl(4, a.data_ptr(), None, None, y.data_ptr(), 128, None) != 0  # a two-operand kind without b
    assert wmx.wmx_debug_spl(8, a.data_ptr(), a.data_ptr(), None, y.data_ptr(), 128, None) != 0
    assert wmx.wmx_debug_spl(16, a.data_ptr(), None, None, y.data_ptr(), 100, None) != 0  # not whole rows
    assert wmx.wmx_debug_spl(1, a.data_ptr(), None, None, y.data_ptr(), 0, None) == 0


def run_fft(wmx, cuda, kind, x):
    d = torch.from_numpy(np.array(x)).to(cuda)
    aux = torch.full((x.shape[0],), -1, dtype=torch.int32, device=cuda)
    assert wmx.wmx_debug_fft(kind, x.shape[0], d.data_ptr(), aux.data_ptr(), None) == 0
    return d.cpu().numpy(), aux.cpu().numpy()


def padded(x, n):
    out = np.zeros((x.shape[0], n + 2), np.int16)
    out[:, :n] = x
    return out


# (order, forward kind, inverse kind): the register executors the product runs, and the generic LDS executor kept as their cross-check
EXECUTORS = [(7, 8, 9), (8, 10, 11), (8, 12, 13)]


@pytest.mark.parametrize("order,fwd_kind,inv_kind", EXECUTORS)
def test_spl_fft_executor_equals_the_oracle(wmx, cuda, oracle_port, order, fwd_kind, inv_kind):
    n = 1 << order
    S.assert_scale_counts_covered(order, oracle_port)
    x, fwd, spec, out, sc = S.fft_oracle_answers(order, oracle_port)
    got, _ = run_fft(wmx, cuda, fwd_kind, padded(x, n))
    assert first_difference(got, fwd) is None
    got, got_sc = run_fft(wmx, cuda, inv_kind, spec)
    assert first_difference(got_sc, sc) is None, "scale counts"
    assert first_difference(got[:, :n], out) is None  # all n samples of every transform
    # 37 transforms from the middle of each family, as a batch of their own
    fam = S.fft_inverse_families(order, oracle_port)
    at = np.concatenate([np.arange(37) + o for o in (1000, fam["a"].shape[0] + 150, fam["a"].shape[0] + fam["b"].shape[0] + 300)])
    got, got_sc = run_fft(wmx, cuda, inv_kind, spec[at])
    assert np.array_equal(got_sc, sc[at]) and np.array_equal(got[:, :n], out[at])


def test_generic_executor_equals_the_register_executor(wmx, cuda, oracle_port):
    """kinds 12 / 13 against kinds 10 / 11 directly, beside both being held to the oracle above"""
    x, fwd, spec, out, sc = S.fft_oracle_answers(8, oracle_port)
    assert np.array_equal(run_fft(wmx, cuda, 12, padded(x, 256))[0], run_fft(wmx, cuda, 10, padded(x, 256))[0])
    a, b = run_fft(wmx, cuda, 13, spec), run_fft(wmx, cuda, 11, spec)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0][:, :256], b[0][:, :256])
