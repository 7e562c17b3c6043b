"""The float NS kernel decides `frame energy == 0` (the early return of Analyze and Process) without summing: the sum of the windowed samples' squares,
non-negative finite terms added up from +0, is zero exactly when every term is, so the kernel asks whether any term is non-zero.  That
holds only if no non-zero term is lost on its way into the sum: window[i] * x with an int16 x != 0 is at least window[i] in magnitude, and
its square at least window[i]^2 (rounding is monotonic), so it is enough that the smallest non-zero window[i]^2 is a NORMAL float --
then every non-zero term is >= FLT_MIN whatever the kernel's denormal mode.  Checked here for both analysis windows (L = 128 for 8 kHz,
256 for 16 / 32 kHz) as the library's constants block holds them; no GPU needed."""
import ctypes as C

import numpy as np
import pytest


def library_window(wmx, L):
    w = np.empty(L, np.float32)
    assert wmx.wmx_debug_ns_window(L, w.ctypes.data) == 0
    return w


@pytest.mark.parametrize("L", [128, 256])
def test_smallest_nonzero_window_square_is_a_normal_float(wmx, L):
    w = library_window(wmx, L)
    assert np.isfinite(w).all() and (w >= 0).all() and w.max() == 1.0
    sq = w * w  # float32 product, rounded once, like the kernel's w * w with x = 1
    assert sq.dtype == np.float32
    nz = sq[w != 0]
    assert nz.size >= L - 1  # at most the ramp's first point is zero
    tiny = np.finfo(np.float32).tiny  # FLT_MIN, the smallest normal float
    print("L = %d: smallest non-zero window value %.9g, its square %.9g, FLT_MIN %.9g" % (L, w[w != 0].min(), nz.min(), tiny))
    assert nz.min() >= tiny
    assert (sq[w == 0] == 0).all()


@pytest.mark.parametrize("L", [128, 256])
def test_window_is_the_oracles_and_starts_with_zero(wmx, oracle_port, L):
    """The zero-frame case of tests/test_ns_idle_lanes_gpu.py puts a lone sample at index 0 of the analysis buffer: window[0] must be 0."""
    w = library_window(wmx, L)
    ref = np.empty(256, np.float32)
    oracle_port.orc_ns_window.argtypes = [C.c_int, C.c_void_p]
    oracle_port.orc_ns_window.restype = None
    oracle_port.orc_ns_window(L, ref.ctypes.data)
    assert np.array_equal(w.view(np.uint32), ref[:L].view(np.uint32))
    assert w[0] == 0.0 and w[1] != 0.0


def test_window_hook_rejects_other_sizes(wmx):
    w = np.empty(512, np.float32)
    assert wmx.wmx_debug_ns_window(64, w.ctypes.data) != 0
    assert wmx.wmx_debug_ns_window(256, None) != 0
