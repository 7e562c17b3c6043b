"""What wmx_mix_play_duck / wmx_mix_export_duck refuse (include/wmix_amd.h): a reduce outside the reference's 0 .. 15, a mixer without
a store, a mixer whose rings are not 1 x 8000 (it can have no store) -- and that a refusal changes nothing.  The signatures themselves
are those tests/test_abi_signatures.py reads from the header."""
import numpy as np
import pytest

from conf_inputs import EINVAL

pytestmark = pytest.mark.gpu

ESTATE = -10003


def test_refusals_of_play_duck_and_export_duck(cuda, wmx):
    from wmix_amd.mix import MixBatch
    clip = np.arange(1, 401, dtype=np.int16)
    mb = MixBatch(6, 1, 8000)
    div = np.full(6, 9, np.uint8)
    # no store: nothing to play from, nothing ducks
    assert wmx.wmx_mix_play_duck(mb._h, None, 0, 0, 1, 0, 3, None) == ESTATE
    assert wmx.wmx_mix_export_duck(mb._h, div.ctypes.data, None) == 0 and div.tolist() == [1] * 6
    assert wmx.wmx_mix_prompts(mb._h, 2, 400) == 0 and wmx.wmx_mix_add_clip(mb._h, clip.ctypes.data, 400, None) == 0
    idx = np.array([1, 4], np.int32)
    assert wmx.wmx_mix_play_duck(mb._h, idx.ctypes.data, 2, 0, 0, 2, 15, None) == 0  # the largest reduce there is
    pos, state = np.zeros(6, np.uint32), np.zeros(6, np.int32)

    def now():
        assert wmx.wmx_mix_export_duck(mb._h, div.ctypes.data, None) == 0
        assert wmx.wmx_mix_export_prompts(mb._h, state.ctypes.data, pos.ctypes.data, None, None, None) == 0
        return div.tolist(), state.tolist(), pos.tolist()

    was = now()
    assert was[0] == [1, 16, 1, 1, 16, 1] and was[1] == [-1, 0, -1, -1, 0, -1]
    for what, args in (("reduce 16", (idx.ctypes.data, 2, 0, 1, 0, 16)), ("reduce -1", (idx.ctypes.data, 2, 0, 1, 0, -1)),
                       ("reduce 256", (idx.ctypes.data, 2, 0, 1, 0, 256)), ("a bad clip", (idx.ctypes.data, 2, 1, 1, 0, 3)),
                       ("a gap too long", (idx.ctypes.data, 2, 0, 1, 65536, 3)), ("a negative repeat", (idx.ctypes.data, 2, 0, -1, 0, 3)),
                       ("a bad ring", (np.array([1, 6], np.int32).ctypes.data, 2, 0, 1, 0, 3))):
        assert wmx.wmx_mix_play_duck(mb._h, *args, None) == EINVAL, what
        assert now() == was, what
    assert wmx.wmx_mix_export_duck(mb._h, None, None) == EINVAL and wmx.wmx_mix_export_duck(None, div.ctypes.data, None) == EINVAL
    assert wmx.wmx_mix_play_duck(None, None, 0, 0, 1, 0, 3, None) == EINVAL
    # wmx_mix_play is wmx_mix_play_duck with reduce 0: it releases the duck of the ring it replaces
    assert wmx.wmx_mix_play(mb._h, idx.ctypes.data, 1, 0, 1, 0, None) == 0 and now()[0] == [1, 1, 1, 1, 16, 1]
    # a tick's step: 400 samples are three calls, then a gap of two ticks that is not ducked, then the next pass
    seen = []
    for _ in range(6):
        assert wmx.wmx_mix_load_prompts(mb._h, None) == 0
        seen.append(now()[0][4])
    assert seen == [16, 16, 1, 1, 16, 16]
    mb.close()
    # a mixer that is not 1 x 8000 has no store, hence no play
    for chn, freq in ((2, 8000), (1, 16000)):
        other = MixBatch(2, chn, freq)
        assert wmx.wmx_mix_prompts(other._h, 1, 100) == EINVAL
        assert wmx.wmx_mix_play_duck(other._h, None, 0, 0, 1, 0, 3, None) == ESTATE
        assert wmx.wmx_mix_export_duck(other._h, div.ctypes.data, None) == 0 and div[:2].tolist() == [1, 1]
        other.close()
