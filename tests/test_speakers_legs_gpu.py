"""GPU parity of talker selection over leg packets: wmx_mix_select_speakers_legs (wmix_amd/csrc/mix.hip, speakers.h) through the Python
mirror against the numpy model of tests/speakers_legs_model.py.  Integer results, np.array_equal.

The layout has conferences of 2, 3, 5 and 32 members in non-ascending ring order and two rings in no conference: 44 rings, the fewest
that hold them (the four sizes alone are 42)."""
import numpy as np
import pytest

from conf_inputs import EINVAL
from speakers_legs_model import SpeakersLegsModel

pytestmark = pytest.mark.gpu

G, K, T, N_EL = 44, 3, 12, 160
SBYTES = 2 * N_EL
IDLE = [9, 30]


def layout():
    pool = [r for r in range(G) if r not in IDLE]
    c5, c2, c32, c3 = pool[0:5][::-1], pool[5:7][::-1], pool[7:39], pool[39:42]
    return [c5, c32[1::2] + c32[0::2][::-1], c2, c3[1:] + c3[:1]]


def script(seed):
    """rows [T, G, K, N_EL] and lens [T, G, K]: most legs call in slot 0; some call only in slot 1 or only in slot 2 on some ticks, some in
    two slots, some not at all; a slot that is no call holds 0, 1, a shorter or a longer length -- and a loud row all the same"""
    rng = np.random.default_rng(seed)
    scale = rng.choice([3, 40, 400, 4000, 20000], size=G)
    rows = (rng.integers(-1000, 1000, size=(T, G, K, N_EL)) * scale[None, :, None, None] // 1000).astype(np.int16)
    rows[:, :, :, 0] |= 1  # no row is silent: a slot that is no call would show if it were read
    lens = np.zeros((T, G, K), np.uint32)
    kind = rng.integers(0, 6, size=(T, G))
    lens[:, :, 0][kind <= 2] = SBYTES
    lens[:, :, 1][(kind == 2) | (kind == 3)] = SBYTES
    lens[:, :, 2][(kind == 2) | (kind == 4)] = SBYTES
    junk = np.array([0, 1, SBYTES - 2, SBYTES + 2], np.uint32)[rng.integers(0, 4, size=lens.shape)]
    return rows, np.where(lens == SBYTES, lens, junk).astype(np.uint32)


def model_run(rows, lens, lay, mx, floor, shift, mute, slots=None):
    m, res = SpeakersLegsModel(G), []
    for t in range(T):
        sp, mo = m.step_legs(lay, rows[t], lens[t], SBYTES, mx, floor, shift, mute, slots)
        res.append((sp.copy(), mo.copy(), m.env.copy()))
    return res


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("max_speakers", [1, 2, 32])
@pytest.mark.parametrize("stride", [161, 164], ids=["unaligned", "aligned"])
def test_selection_over_leg_packets_against_the_model(cuda, stride, max_speakers, shift):
    import torch
    from wmix_amd.mix import MixBatch
    rows, lens = script(17)
    lay = layout()
    assert sorted(len(c) for c in lay) == [2, 3, 5, 32] and sorted(r for c in lay for r in c) == [r for r in range(G) if r not in IDLE]
    assert any(c != sorted(c) for c in lay)
    mute = np.zeros(G, np.uint8)
    mute[[lay[1][0], lay[3][1]]] = 1
    levels = np.abs(rows.astype(np.int64)).sum(3).max(2)
    floor = int(np.median(levels[0]))  # the quiet legs miss it
    want = model_run(rows, lens, lay, max_speakers, floor, shift, mute)
    # on the CPU: the script has legs whose only call is in slot 1 or 2, and the level of slot 0 alone -- what a row per leg sees --
    # selects somebody else on at least one tick, so the old rule cannot pass here
    only_later = (lens[:, :, 0] != SBYTES) & ((lens[:, :, 1] == SBYTES) ^ (lens[:, :, 2] == SBYTES))
    members = np.isin(np.arange(G), [r for c in lay for r in c])
    assert (only_later & members[None, :]).any()
    old = model_run(rows, lens, lay, max_speakers, floor, shift, mute, slots=[0])
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(want, old))
    assert any(w[0].any() for w in want) and any((w[2][[r for c in lay for r in c]] < floor).any() for w in want)

    padded = np.full((T, G, K, stride), 32767, np.int16)  # loud between the rows
    padded[..., :N_EL] = rows
    d_rows, d_lens = torch.from_numpy(padded).to(cuda), torch.from_numpy(lens.view(np.int32)).to(cuda)
    d_mute = torch.from_numpy(mute).to(cuda)
    mb = MixBatch(G, 1, 8000)
    mb.set_conferences(lay)
    out = torch.full((G,), 7, dtype=torch.uint8, device=cuda)
    for t in range(T):
        src = d_rows[t][:, :, :N_EL]  # strides (K * stride, stride, 1)
        got = mb.select_speakers_legs(src, SBYTES, d_lens[t], max_speakers, floor, shift, mute=d_mute, out=out).cpu().numpy()
        sp, env = mb.export_speakers()
        assert np.array_equal(got, want[t][1]), ("mute_out, tick", t, np.flatnonzero(got != want[t][1]))
        assert np.array_equal(sp, want[t][0]) and np.array_equal(env, want[t][2]), ("speaking / env, tick", t)
    assert got[IDLE].tolist() == [1, 1] and not env[IDLE].any()
    mb.close()


def test_one_slot_that_is_always_a_call_is_the_conf_form(cuda):
    import torch
    from wmix_amd.mix import MixBatch
    rows, _ = script(5)
    lay = layout()
    a, b = MixBatch(G, 1, 8000), MixBatch(G, 1, 8000)
    lens = torch.full((G, 1), SBYTES, dtype=torch.int32, device=cuda)
    for m in (a, b):
        m.set_conferences(lay)
    for t in range(6):
        src = torch.from_numpy(np.ascontiguousarray(rows[t, :, :1])).to(cuda)
        ma = a.select_speakers_conf(src[:, 0], SBYTES, 2, 5000, 3).cpu().numpy()
        mo = b.select_speakers_legs(src, SBYTES, lens, 2, 5000, 3).cpu().numpy()
        assert np.array_equal(ma, mo), t
        assert all(np.array_equal(x, y) for x, y in zip(a.export_speakers(), b.export_speakers())), t
    a.close()
    b.close()


def test_refusals_leave_the_envelopes_alone(cuda, wmx):
    import torch
    from wmix_amd.mix import MixBatch
    rows, lens = script(3)
    d_rows, d_lens = torch.from_numpy(rows[0]).to(cuda), torch.from_numpy(lens[0].view(np.int32)).to(cuda)
    out = torch.zeros(G, dtype=torch.uint8, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    mb = MixBatch(G, 1, 8000)

    def call(src=d_rows.data_ptr(), sbytes=SBYTES, sstride=K * N_EL, pstride=N_EL, k=K, ln=d_lens.data_ptr(), mx=2, shift=3, o=out.data_ptr()):
        return wmx.wmx_mix_select_speakers_legs(mb._h, src, sbytes, sstride, pstride, k, ln, None, mx, 100, shift, o, stream)

    assert call() == EINVAL and b"layout" in wmx.wmx_last_error()
    mb.set_conferences(layout())
    assert call() == 0
    before = mb.export_speakers()
    assert before[1].any()
    for kw in (dict(k=0), dict(k=5), dict(ln=None), dict(src=None), dict(o=None), dict(mx=0), dict(mx=33), dict(shift=-1), dict(shift=32),
               dict(sbytes=2 * 131072), dict(pstride=N_EL - 1), dict(sstride=K * N_EL - 1), dict(pstride=-N_EL)):
        assert call(**kw) == EINVAL, kw
    after = mb.export_speakers()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    louder = torch.from_numpy(rows[0] * 2).to(cuda)
    assert call(src=louder.data_ptr()) == 0 and not np.array_equal(mb.export_speakers()[1], before[1])  # and it still works
    mb.close()
