"""GPU parity: wmix_amd/csrc/g711.hip through the C ABI vs the oracle and the
golden tables.  Bit-exact (integer path)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_g711_oracle import orc_decode, orc_encode

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(GOLDEN, "g711_golden.npz"))


def _t(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


@pytest.mark.parametrize("law", ["a", "u"])
def test_exhaustive_tables_device_api(cuda, law):
    from wmix_amd import g711
    pcm = _t(np.arange(-32768, 32768, dtype=np.int16), cuda)
    assert np.array_equal(g711.encode(law, pcm).cpu().numpy(), G["enc_" + law])
    codes = _t(np.arange(256, dtype=np.uint8), cuda)
    assert np.array_equal(g711.decode(law, codes).cpu().numpy(), G["dec_" + law])


@pytest.mark.parametrize("law", ["a", "u"])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 80, 81, 4095, 80 * 6078])
def test_ragged_sizes_and_unaligned_pointers_vs_oracle(cuda, oracle_port, law, n):
    import torch
    from wmix_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(n)
    pcm = rng.integers(-32768, 32768, size=n + 3, dtype=np.int16)
    for off in (0, 1, 3):  # element offsets -> 2/6-byte misalignment exercises the scalar path
        d_pcm = _t(pcm, cuda)
        d_code = torch.zeros(n + 8, dtype=torch.uint8, device=cuda)
        _lib.check(L.wmx_g711_encode(g711_law(law), d_pcm.data_ptr() + 2 * off, d_code.data_ptr() + off, n,
                                     torch.cuda.current_stream().cuda_stream))
        want, _ = orc_encode(oracle_port, law, pcm[off:off + n])
        got = d_code.cpu().numpy()
        assert np.array_equal(got[off:off + n], want)
        assert not got[:off].any() and not got[off + n:].any()  # no write outside [off, off+n)
        d_out = torch.zeros(n + 8, dtype=torch.int16, device=cuda)
        _lib.check(L.wmx_g711_decode(g711_law(law), d_code.data_ptr() + off, d_out.data_ptr() + 2 * off, n,
                                     torch.cuda.current_stream().cuda_stream))
        want_d, _ = orc_decode(oracle_port, law, want)
        got_d = d_out.cpu().numpy()
        assert np.array_equal(got_d[off:off + n], want_d)
        assert not got_d[:off].any() and not got_d[off + n:].any()


def g711_law(law):
    return 0 if law == "a" else 1


@pytest.mark.parametrize("law", ["a", "u"])
def test_reference_host_signatures(wmx, oracle_port, law):
    """PCM2G711x / G711x2PCM / g711x_encode / g711x_decode over HOST buffers (src/g711codec.h:24-34); PCM2G711x / G711x2PCM also at
    the last size the adapter stages in mapped memory (16 384 samples) and the first it copies (16 385)."""
    for n in (16384, 16385):
        x = np.random.default_rng(n).integers(-32768, 32768, size=n, dtype=np.int16)
        enc, dec = np.zeros(n + 8, np.uint8), np.zeros(n + 8, np.int16)
        assert getattr(wmx, "PCM2G711" + law)(C.c_void_p(x.ctypes.data), C.c_void_p(enc.ctypes.data), 2 * n, 0) == n
        assert np.array_equal(enc[:n], orc_encode(oracle_port, law, x)[0]) and not enc[n:].any()
        assert getattr(wmx, "G711%s2PCM" % law)(C.c_void_p(enc.ctypes.data), C.c_void_p(dec.ctypes.data), n, 0) == 2 * n
        assert np.array_equal(dec[:n], orc_decode(oracle_port, law, enc[:n])[0]) and not dec[n:].any()
    pcm = G["wav_excerpt"]
    out = np.zeros(pcm.size, np.uint8)
    r = getattr(wmx, "PCM2G711" + law)(C.c_void_p(pcm.ctypes.data), C.c_void_p(out.ctypes.data), pcm.size * 2, 0)
    assert r == pcm.size and np.array_equal(out, G["wav_excerpt_enc_" + law])
    back = np.zeros(pcm.size, np.int16)
    r = getattr(wmx, "G711%s2PCM" % law)(C.c_void_p(out.ctypes.data), C.c_void_p(back.ctypes.data), out.size, 0)
    assert r == 2 * pcm.size and np.array_equal(back, G["wav_excerpt_dec_" + law])
    out2 = np.zeros(80, np.uint8)
    assert getattr(wmx, "g711%s_encode" % law)(C.c_void_p(out2.ctypes.data), C.c_void_p(pcm.ctypes.data), 80) == 80
    assert np.array_equal(out2, out[:80])
    back2 = np.zeros(80, np.int16)
    assert getattr(wmx, "g711%s_decode" % law)(C.c_void_p(back2.ctypes.data), C.c_void_p(out2.ctypes.data), 80) == 160
    assert np.array_equal(back2, back[:80])
    f = getattr(wmx, "linear2%slaw" % law)
    assert [f(int(v)) for v in (-1, -8, -32768, 0, 32767)] == [int(G["enc_" + law][v + 32768]) for v in (-1, -8, -32768, 0, 32767)]


@pytest.mark.parametrize("law", ["a", "u"])
def test_full_size_round_trip_properties(cuda, law):
    """Size-independent properties at bench scale (2^26 samples): enc(dec(c)) == c for every
    code stream produced by enc, and dec(enc(x)) is idempotent."""
    import torch
    from wmix_amd import g711
    gen = torch.Generator(device="cpu").manual_seed(11)
    pcm = torch.randint(-32768, 32768, (1 << 26,), dtype=torch.int16, generator=gen).to(cuda)
    c1 = g711.encode(law, pcm)
    p1 = g711.decode(law, c1)
    c2 = g711.encode(law, p1)
    p2 = g711.decode(law, c2)
    assert torch.equal(p1, p2)
    # A-law code 0x55^... : the reference's negative path maps -1..-8 oddly, so codes need not
    # round-trip exactly, but the decoded PCM must (idempotence), and sign must be preserved.
    assert bool(((p1 >= 0) == (pcm >= 0))[pcm.abs() > 16].all())
    # checksum-of-table property: histogram of codes only depends on the exhaustive table
    idx = (pcm.to(torch.int32) + 32768).cpu().numpy()
    assert np.array_equal(c1.cpu().numpy(), G["enc_" + law][idx])
