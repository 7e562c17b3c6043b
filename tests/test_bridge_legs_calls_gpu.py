"""wmx_mix_load_minus_legs_calls (wmix_amd/csrc/mix.hip, leg_cursor.h: leg_cursor_span_calls) through the Python mirror: the bridge load
with a cursor per leg, fed a call list per leg.  The oracle is LegsOracle of tests/leg_oracle_model.py -- one reference ring per leg,
one cursor per source leg, one orc_load_data call per valid slot in slot order -- fed the REPAIRED rows: the call list of
tests/leg_seq_model.py laid out as four slots, a silence call being a row of zeros with lens = sbytes (what WCT_SILENCE loads).
Integers, np.array_equal."""
import numpy as np
import pytest

from conf_inputs import EINVAL, NULL_HEAD
from leg_oracle_model import LegsOracle
from leg_seq_model import LegsSeqModel, pack, repaired_rows
from test_bridge_legs_gpu import big_layout, main_layout, script
from test_rtp_sequence_gpu import arrivals

pytestmark = pytest.mark.gpu

K = 3


def run_both(cuda, lib, layout, n, T, seed, check_at, mute=None, unreadable=(), hog=None, drop_rule=False):
    """T ticks on the oracle and on the device: drain one package, sequence the tick's arrivals with the model, load.  `unreadable`:
    legs whose d_len is spoilt behind the sequencer for every slot now and then -- a data call that names such a slot is silence.
    `hog`: a leg that delivers sequence numbers three apart every tick, so that its lists are S S S D."""
    import torch
    from wmix_amd.mix import MixBatch
    rng = np.random.default_rng(seed)
    raw, lens = arrivals(seed, n, T, K)
    if hog is not None:
        lens[:, hog, :] = 0
        lens[:, hog, 1] = 320
        s = (4 * np.arange(T) + 3) % 65536
        raw[:, hog, 1] = ((s & 0xFF) << 8) | (s >> 8)
    src = rng.integers(-20000, 20000, size=(T, n, K, 161), dtype=np.int16)
    orc, model = LegsOracle(lib, n, (1, 8000), 1, None, drop_rule), LegsSeqModel(n)
    if hog is not None:
        model.legs[hog].synced = 1  # next = 0: the first tick is a gap of three already
    mb = MixBatch(n, 1, 8000)
    mb.set(0, 0, 1)
    mb.set_conferences(layout)
    dmute = torch.from_numpy(mute).to(cuda) if mute is not None else None
    seen = {"silence": 0, "reordered": 0, "four": 0, "unreadable": 0}
    for t in range(T):
        want = orc.drain()
        got = mb.drain(orc.pkg).cpu().numpy()
        assert np.array_equal(got, want), ("drained rows, tick", t, np.argwhere((got != want).any(1))[:6].ravel())
        words, new_lens, lists = model.tick(raw[t], lens[t], 3)
        pcm = src[t].copy()
        for g in unreadable:
            if t % 3 == 1:
                new_lens[g, :] = [0, 319, 640]
                pcm[g] = 0  # the oracle's rows of these calls: zeros
                seen["unreadable"] += sum(kind == "D" for kind, _ in lists[g])
        rows, rlens = repaired_rows(pcm, lists)
        for calls in lists:
            data = [k for kind, k in calls if kind == "D"]
            seen["silence"] += any(kind == "S" for kind, _ in calls)
            seen["reordered"] += data != sorted(data)
            seen["four"] += len(calls) == 4
        orc.load(layout, rows, rlens, 320, 8000, 1, 160, mute)
        mb.load_minus_legs_calls(torch.from_numpy(src[t]).to(cuda), 320, 8000, 1, torch.from_numpy(new_lens.view(np.int32)).to(cuda),
                                 torch.from_numpy(words.view(np.int32)).to(cuda), mute=dmute)
        if t + 1 in check_at:
            h, tk, dropped = mb.export_leg_cursors()
            wh, wt = orc.cursors()
            assert np.array_equal(h, wh) and np.array_equal(tk, wt), ("cursors after tick", t, np.argwhere((h != wh) | (tk != wt)).ravel())
            assert np.array_equal(dropped, orc.dropped), ("dropped after tick", t)
            for k in range(n):
                assert np.array_equal(mb.export(k)[0], orc.rings.ring(k)), ("ring", k, "after tick", t)
    res = mb.export_leg_cursors()
    mb.close()
    return res, orc, seen


def test_call_lists_against_one_reference_mixer_per_leg(cuda, oracle_port):
    """conferences of 2, 3, 5, 9 and 17: 60 ticks of legs that lose, duplicate, swap, delay and restart, so the lists hold silence, data
    calls out of slot order and up to four calls; a muted leg; a leg whose rows are not readable every third tick"""
    layout, idle = main_layout()
    c17, c9 = layout[0], layout[6]
    mute = np.zeros(40, np.uint8)
    mute[c17[9]] = 1
    (h, tk, dropped), orc, seen = run_both(cuda, oracle_port, layout, 40, 60, 11, {1, 30, 60}, mute=mute, unreadable=[c9[2], c17[3]])
    assert not dropped.any()
    assert seen["silence"] > 50 and seen["reordered"] > 20 and seen["four"] >= 3 and seen["unreadable"] > 10, seen
    assert all(orc.cursor[r] == (NULL_HEAD, 0) for r in idle) and orc.cursor[c17[9]] != (NULL_HEAD, 0)


def test_call_lists_in_a_conference_of_32(cuda, oracle_port):
    layout, idle = big_layout()
    (h, tk, dropped), orc, seen = run_both(cuda, oracle_port, layout, 40, 40, 12, {1, 40})
    assert not dropped.any() and seen["silence"] > 30 and seen["reordered"] > 10, seen


def test_a_gap_filled_list_runs_into_the_lap_rule(cuda, oracle_port):
    """One leg's lists are S S S D every tick: four calls a tick on a lead of 200 ms.  Once the end cursor would lie more than one ring
    ahead of the mixer's tick the list's tail is left out and counted, silence calls included."""
    layout = [[4, 0, 2], [], [5, 1]]
    (h, tk, dropped), orc, seen = run_both(cuda, oracle_port, layout, 7, 30, 13, {1, 16, 30}, hog=0, drop_rule=True)
    assert np.array_equal(dropped, orc.dropped) and dropped[0] > 30 and not dropped[1:].any()
    assert tk[0] - orc.rings.r[0].tick <= 16000 < tk[0] - orc.rings.r[0].tick + 320


def identity_lists(lens, sbytes):
    """every valid slot in slot order, no silence"""
    return np.array([pack([("D", k) for k in range(lens.shape[1]) if row[k] == sbytes]) for row in lens], np.uint32)


def test_identity_lists_are_load_minus_legs_byte_for_byte(cuda):
    import torch
    from wmix_amd.mix import MixBatch
    T, n = 50, 40
    layout, idle = main_layout()
    c17, c3, c5, c9 = layout[0], layout[3], layout[5], layout[6]
    lens = script(T, n, {"lossy": c3[1], "silent": c5[2], "burst": c9[1], "gap": c17[5]}, 320, 5)
    rng = np.random.default_rng(3)
    src = torch.from_numpy(rng.integers(-20000, 20000, size=(T, n, 3, 161), dtype=np.int16)).to(cuda)
    mute = np.zeros(n, np.uint8)
    mute[c17[9]] = 1
    dmute = torch.from_numpy(mute).to(cuda)
    twin, mb = MixBatch(n, 1, 8000), MixBatch(n, 1, 8000)
    for m in (twin, mb):
        m.set(16000 - 3200 - 480, 0, 2)
        m.set_conferences(layout)
    for t in range(T):
        dl = torch.from_numpy(lens[t].view(np.int32)).to(cuda)
        twin.load_minus_legs(src[t], 320, 8000, 1, dl, mute=dmute)
        mb.load_minus_legs_calls(src[t], 320, 8000, 1, dl, torch.from_numpy(identity_lists(lens[t], 320).view(np.int32)).to(cuda), mute=dmute)
        assert np.array_equal(twin.drain(320).cpu().numpy(), mb.drain(320).cpu().numpy()), t
        if t in (0, 24, 49):
            assert all(np.array_equal(a, b) for a, b in zip(twin.export_leg_cursors(), mb.export_leg_cursors())), t
            for k in range(n):
                assert np.array_equal(twin.export(k)[0], mb.export(k)[0]), (t, k)
    assert twin.export(c17[0])[0].any()
    twin.close()
    mb.close()


def test_refusals_leave_rings_layout_and_cursors_alone(cuda, wmx):
    import torch
    from wmix_amd.mix import MixBatch
    n, per = 12, 160
    mb = MixBatch(n, 1, 8000)
    rng = np.random.default_rng(4)
    mb.load(torch.from_numpy(rng.integers(-20000, 20000, size=(n, 1, per + 1), dtype=np.int16)).to(cuda), 320, 8000, 1)
    src = torch.from_numpy(rng.integers(-20000, 20000, size=n * 4 * 9000, dtype=np.int16)).to(cuda)  # room for every call below, refused or not
    lens = torch.full((n, 4), 320, dtype=torch.int32, device=cuda)
    calls = torch.full((n,), int(pack([("D", 1), ("S", None), ("D", 0)])), dtype=torch.int32, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream

    def load(src_ptr, sbytes, max_packets, len_ptr, calls_ptr, freq=8000, stride=9000):
        return wmx.wmx_mix_load_minus_legs_calls(mb._h, src_ptr, sbytes, freq, 1, 16, 4 * stride, stride, max_packets, len_ptr, calls_ptr, None, 1,
                                                 stream)

    def state():
        torch.cuda.synchronize()
        return [mb.export(k)[0] for k in range(n)], mb.export_leg_cursors(), mb.conferences()

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and a[2] == b[2]

    first = state()
    assert load(src.data_ptr(), 320, 3, lens.data_ptr(), calls.data_ptr()) == EINVAL and b"layout" in wmx.wmx_last_error()
    assert same(state(), first)
    mb.set_conferences([[3, 1], [7, 5, 9]])
    assert load(src.data_ptr(), 320, 3, lens.data_ptr(), calls.data_ptr()) == 0
    before = state()
    assert not same(before, first) and sorted(np.flatnonzero(before[1][0] != NULL_HEAD)) == [1, 3, 5, 7, 9]
    ticks = before[1][1][[1, 3, 5, 7, 9]]
    assert len(set(ticks.tolist())) == 1 and ticks[0] >= 3 * 320 and ticks[0] % 320 == 0  # three calls each, the silent one too
    for max_packets in (0, 5, -1):
        assert load(src.data_ptr(), 320, max_packets, lens.data_ptr(), calls.data_ptr()) == EINVAL and b"max_packets" in wmx.wmx_last_error()
    assert load(None, 320, 3, lens.data_ptr(), calls.data_ptr()) == EINVAL and load(src.data_ptr(), 320, 3, None, calls.data_ptr()) == EINVAL
    assert load(src.data_ptr(), 320, 3, lens.data_ptr(), None) == EINVAL
    # 3 x 2100 samples fit the ring of 8000 and wmx_mix_load_minus_legs takes them; a list may hold 4 calls, which do not
    assert load(src.data_ptr(), 4200, 3, lens.data_ptr(), calls.data_ptr()) == EINVAL and b"do not fit" in wmx.wmx_last_error()
    assert load(src.data_ptr(), 17000, 1, lens.data_ptr(), calls.data_ptr()) == EINVAL
    assert load(src.data_ptr(), 320, 3, lens.data_ptr(), calls.data_ptr(), freq=100) == EINVAL
    assert same(state(), before)
    assert load(src.data_ptr(), 320, 3, lens.data_ptr(), calls.data_ptr()) == 0
    after = state()
    assert [k for k in range(n) if not np.array_equal(after[0][k], before[0][k])] == [1, 3, 5, 7, 9]
    mb.close()
