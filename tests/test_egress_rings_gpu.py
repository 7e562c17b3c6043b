"""Play and send in one kernel: wmx_rtp_egress_rings (wmix_amd/csrc/rtp.hip) against the pair it replaces, wmx_mix_drain(320 bytes)
followed by wmx_rtp_egress(1, 8000 -> 1, 8000), on twin mixers and twin sender sets loaded alike.  Datagrams, every ring, head, tick,
seq and timestamp, byte for byte."""
import numpy as np
import pytest

from conf_inputs import EINVAL

pytestmark = pytest.mark.gpu

G, RING = 5, 16000
# head 0; a head whose byte offset is 2 mod 8 (the narrow reads); 160 bytes before the ring's end (the package straddles it, between two
# lanes' pieces); and 162 bytes before it (2 mod 8 again: the end falls inside one lane's four samples)
STARTS = [0, 4010, RING - 160, RING - 162]


@pytest.mark.parametrize("out_stride", [172, 173], ids=["rows_aligned", "rows_unaligned"])
@pytest.mark.parametrize("law", ["a", "u"])
def test_egress_rings_is_drain_then_egress(cuda, law, out_stride):
    import torch
    from wmix_amd.mix import MixBatch
    from wmix_amd.rtp import RtpSenders
    assert STARTS[1] % 8 == 2 and STARTS[3] % 8 == 6 and all(s % 2 == 0 for s in STARTS)
    rng = np.random.default_rng(8)
    pair, fused = (MixBatch(G, 1, 8000), RtpSenders(G, law)), (MixBatch(G, 1, 8000), RtpSenders(G, law))
    tick = 0
    for start in STARTS:
        audio = rng.integers(-32768, 32768, size=(G, 1, 6 * 160 + 1), dtype=np.int16)  # six packages from the head on: four are played
        audio[0, 0, :8] = [-32768, 32767, 0, -1, 1, -8, 8, 255]
        src = torch.from_numpy(audio).to(cuda)
        for mb, _ in (pair, fused):
            mb.set_play_correct(0)
            mb.set(start, tick, 1)
            mb.load(src, 6 * 320, 8000, 1)
        for t in range(4):
            pcm = pair[0].drain(320)
            want = pair[1].egress(pcm, 1, 8000, 1, 8000).cpu().numpy()
            rows = torch.full((G, out_stride), 0xEE, dtype=torch.uint8, device=cuda)
            got = fused[1].egress_rings(fused[0], rows[:, :172]).cpu().numpy()
            assert got.shape == (G, 172) and np.array_equal(got, want), (start, t, np.argwhere(got != want)[:6])
            assert (rows[:, 172:].cpu().numpy() == 0xEE).all()
            for g in range(G):
                a, b = pair[0].export(g), fused[0].export(g)
                assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], ("ring / head / tick", start, t, g)
                assert pair[1].state(g) == fused[1].state(g), ("seq / timestamp", start, t, g)
        ring, head, tick = fused[0].export(0)
        assert head == (start + 4 * 320) % RING and ring.any()  # two packages are still queued
        assert (got[:, 12:] != got[0, 12]).any()  # audio was sent, not one code
    assert fused[1].state(G - 1) == (4 * len(STARTS), 160 * 4 * len(STARTS))
    for mb, snd in (pair, fused):
        mb.close()
        snd.close()


def test_egress_rings_refusals_advance_nothing(cuda, wmx):
    import torch
    from wmix_amd.mix import MixBatch
    from wmix_amd.rtp import RtpSenders
    stream = torch.cuda.current_stream().cuda_stream
    rows = torch.zeros((G, 172), dtype=torch.uint8, device=cuda)
    good, wide, snd, four = MixBatch(G, 1, 8000), MixBatch(G, 2, 16000), RtpSenders(G), RtpSenders(G - 1)
    src = torch.from_numpy(np.full((G, 1, 161), 1234, np.int16)).to(cuda)
    good.set_play_correct(0)
    good.load(src, 320, 8000, 1)
    assert snd.egress_rings(good).shape == (G, 172)
    before = [good.export(g) for g in range(G)], [snd.state(g) for g in range(G)], wide.export(0)[1:], four.state(0)

    def call(h, m, p=rows.data_ptr(), stride=172):
        return wmx.wmx_rtp_egress_rings(h, m, p, stride, None, stream)

    assert call(snd._h, wide._h) == EINVAL and b"1 x 8000" in wmx.wmx_last_error()  # another ring format
    assert call(four._h, good._h) == EINVAL and b"senders" in wmx.wmx_last_error()  # mismatched counts
    assert call(None, good._h) == EINVAL and call(snd._h, None) == EINVAL and call(snd._h, good._h, p=None) == EINVAL
    assert call(snd._h, good._h, stride=171) == EINVAL
    after = [good.export(g) for g in range(G)], [snd.state(g) for g in range(G)], wide.export(0)[1:], four.state(0)
    assert before[1:] == after[1:] and all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(before[0], after[0]))
    assert before[0][0][1:] == (320, 320) and before[1][0] == (1, 160)
    for h in (good, wide, snd, four):
        h.close()


def test_a_new_call_in_a_used_slot_resets_rings_and_senders(cuda, wmx):
    """wmx_mix_reset_rings zeroes the listed rings and leaves head and tick; wmx_rtp_reset_streams starts the listed senders from 0; a bad
    index resets nothing"""
    import torch
    from wmix_amd.mix import MixBatch
    from wmix_amd.rtp import RtpSenders
    stream = torch.cuda.current_stream().cuda_stream
    mb, snd = MixBatch(G, 1, 8000), RtpSenders(G)
    mb.load(torch.from_numpy(np.full((G, 1, 161), 77, np.int16)).to(cuda), 320, 8000, 1)
    for _ in range(3):
        snd.egress_rings(mb)
    bad = np.array([1, G], np.int32)
    assert wmx.wmx_mix_reset_rings(mb._h, bad.ctypes.data, 2, stream) == EINVAL and wmx.wmx_rtp_reset_streams(snd._h, bad.ctypes.data, 2, stream) == EINVAL
    assert all(mb.export(g)[0].any() for g in range(G)) and all(snd.state(g) == (3, 480) for g in range(G))
    mb.reset_rings([1, 3])
    snd.reset_streams([3, 4])
    assert [bool(mb.export(g)[0].any()) for g in range(G)] == [True, False, True, False, True]
    assert [snd.state(g) for g in range(G)] == [(3, 480)] * 3 + [(0, 0)] * 2 and mb.export(0)[1:] == (960, 960)
    mb.reset_rings()
    snd.reset_streams()
    assert not any(mb.export(g)[0].any() for g in range(G)) and all(snd.state(g) == (0, 0) for g in range(G)) and mb.export(1)[1:] == (960, 960)
    mb.close()
    snd.close()
