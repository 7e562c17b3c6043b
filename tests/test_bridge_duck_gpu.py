"""GPU parity of the duck: wmx_mix_play_duck / wmx_mix_export_duck and the ducking form of wmx_mix_load_minus_legs and
wmx_mix_load_minus_legs_calls (wmix_amd/csrc/mix.hip: duck_fold_kernel in front of the sweeps; the rule in leg_prompt.h, REDUCE).  The
oracle is LegsOracle of tests/leg_oracle_model.py -- one reference ring per leg, the ordered orc_load_data calls of the other members --
with ring g's reduce_mode set per tick from tests/leg_duck_model.py, as the reference's play task holds wmix->reduceMode while it makes
calls, and the prompt's own call made last with reduce = D.  Every sample of every ring and export_duck, every tick.  One conference of
each of 2, 3, 4, 5, 8, 9, 17 and 32 members -- every size class and both sides of each boundary -- and a leg in none.  Integers,
np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from leg_duck_model import LegsDuckModel
from leg_oracle_model import LegsOracle
from leg_seq_model import pack, repaired_rows

pytestmark = pytest.mark.gpu

K, T, SIZES = 3, 12, (2, 3, 4, 5, 8, 9, 17, 32)
N = sum(SIZES) + 1
CLIPS = (400, 161, 1, 800)  # samples: 3 calls, 2 calls (160 + 1), one sample, 5 calls


def the_layout():
    """-> (the conferences, member lists in no order; the lone leg): over 81 rings dealt out by a fixed shuffle"""
    order = np.random.default_rng(7).permutation(N).tolist()
    lone, layout, at = order[-1], [], 0
    for size in SIZES:
        layout.append(order[at:at + size])
        at += size
    return layout, lone


def the_plays(layout, lone):
    """-> ({tick: [(legs, clip, repeat, gap, reduce)]}, {tick: legs stopped}, the muted ducked leg).  Within 12 ticks: clip 0 (3 ticks)
    with gap 2 has a gap and a second pass, clip 1 (2 ticks) with gap 1 three of each"""
    c2, c3, c4, c5, c8, c9, c17, c32 = layout
    plays = {0: [([c2[0]], 0, 0, 2, 1), ([c2[1]], 1, 0, 1, 3),            # both legs of the pair
                 ([c3[0]], 0, 0, 2, 1), ([c3[2]], 1, 3, 1, 2),            # two of the three: divisors 2 and 3
                 ([c32[0]], 0, 0, 2, 15), ([c32[15]], 1, 0, 1, 1), ([c32[31]], 3, 2, 1, 4),  # members 0, 15, 31: 16, 2 and 5
                 ([c9[4]], 0, 0, 2, 2),                                   # the muted leg
                 ([lone], 0, 0, 2, 1),                                    # the lone leg: nothing to duck
                 ([c5[1]], 1, 0, 0, 0), ([c17[3]], 3, 1, 0, 0)],          # plain plays beside them
             1: [([c8[7]], 2, 0, 1, 15), ([c17[16]], 0, 2, 2, 6), ([c4[1], c5[4]], 3, 1, 0, 7)],
             6: [([c2[0]], 1, 0, 1, 4), ([c4[1]], 0, 1, 0, 0), ([c17[3]], 1, 0, 0, 9)]}  # a play over a play, another reduce
    return plays, {7: [c32[15], c3[0]]}, c9[4]


def the_sources(seed):
    """near full scale, odd negative samples among them; every row carries its look-ahead frame"""
    rng = np.random.default_rng(seed)
    src = rng.integers(-32768, 32768, size=(T, N, K, 161), dtype=np.int16)
    odd = rng.random(src.shape) < 0.25
    return np.where(odd, -(np.abs(src.astype(np.int32)) | 1).clip(1, 32767), src).astype(np.int16)


def the_arrivals(seed, with_lists):
    """-> (lens [T, N, K], call lists [T][N] or None): 0 .. 3 packets per leg and tick; with lists, the data calls in any order and
    silence calls among them, four calls at most"""
    rng = np.random.default_rng(seed)
    lens, lists = np.zeros((T, N, K), np.uint32), [[None] * N for _ in range(T)]
    for t in range(T):
        for g in range(N):
            slots = rng.permutation(K)[:rng.choice([0, 1, 1, 1, 2, 3])].tolist()
            lens[t, g, slots] = 320
            calls = [("D", k) for k in slots]
            if with_lists and rng.random() < 0.3 and len(calls) < 4:
                calls.insert(int(rng.integers(0, len(calls) + 1)), ("S", None))
            lists[t][g] = calls if with_lists else [("D", k) for k in sorted(slots)]
    junk = rng.integers(0, 3, size=lens.shape)
    lens = np.where(lens == 320, lens, np.array([0, 319, 640], np.uint32)[junk]).astype(np.uint32)
    return lens, lists


class DuckOracle(LegsOracle):
    """LegsOracle with a prompt per leg: a tick is the duck taken per ring, the legs' load, the prompts' calls, the duck released"""

    def __init__(self, lib, n, head_off, tick, play_correct):
        super().__init__(lib, n, (1, 8000), 1, play_correct)
        self.pm, self.ducked_ticks, self.prompt_calls = LegsDuckModel(n), 0, 0
        for r in self.rings.r:
            r.head_off, r.tick = head_off, tick

    def tick(self, layout, rows, lens, mute, duck=True):
        divisors = [self.pm.ducks(g) if duck else 1 for g in range(self.n)]
        for g, r in enumerate(self.rings.r):
            r.reduce_mode = divisors[g]  # the play task holds the mode while it makes calls (src/wmixTask.c:1416-1423, 1555-1557)
            self.ducked_ticks += divisors[g] > 1
        self.load(layout, rows, lens, 320, 8000, 1, 160, mute)  # every call reduce 1: rdce = (1 == D) ? 1 : D
        for g, r in enumerate(self.rings.r):
            call = self.pm.step(g, (r.head_off, r.tick, r.play_correct, self.size))
            if call is not None:
                row, (head, tick), after = call
                end = self.rings.load(g, row, 2 * (len(row) - 1), 8000, 1, head, tick, divisors[g])  # its own call: reduce == reduceMode
                assert end == after, ("leg", g, end, after)
                self.prompt_calls += 1
            r.reduce_mode = 1


def run_both(cuda, wmx, lib, with_lists, head_off, play_correct, seed, duck=True):
    """T ticks on the oracle and on the device -> (every ring after every tick [T, N, 8000], the oracle); duck = False: the same plays
    with reduce 0 on both"""
    import torch
    from wmix_amd.mix import MixBatch
    layout, lone = the_layout()
    plays, stops, muted = the_plays(layout, lone)
    src, (lens, lists) = the_sources(seed), the_arrivals(seed + 1, with_lists)
    mute = np.zeros(N, np.uint8)
    mute[muted] = 1
    orc = DuckOracle(lib, N, head_off, 640000, play_correct)
    mb = MixBatch(N, 1, 8000)
    mb.set(head_off, 640000, 1)
    if play_correct is not None:
        mb.set_play_correct(play_correct)
    mb.set_conferences(layout)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(3)
    clips = [rng.integers(-20000, 20000, size=s).astype(np.int16) for s in CLIPS]
    assert wmx.wmx_mix_prompts(mb._h, len(clips), sum(CLIPS)) == 0
    orc.pm.prompts(len(clips), sum(CLIPS))
    for pcm in clips:
        got = C.c_int(-1)
        assert wmx.wmx_mix_add_clip(mb._h, pcm.ctypes.data, pcm.size, C.byref(got)) == 0 and got.value == orc.pm.add_clip(pcm)
    dmute, rings, divisor = torch.from_numpy(mute).to(cuda), np.zeros((T, N, 8000), np.int16), np.zeros(N, np.uint8)
    for t in range(T):
        for legs, clip, repeat, gap, reduce in plays.get(t, ()):
            idx = np.array(legs, np.int32)
            reduce = reduce if duck else 0
            assert wmx.wmx_mix_play_duck(mb._h, idx.ctypes.data, idx.size, clip, repeat, gap, reduce, stream) == 0
            orc.pm.play(legs, clip, repeat, gap, reduce)
        if t in stops:
            idx = np.array(stops[t], np.int32)
            assert wmx.wmx_mix_stop(mb._h, idx.ctypes.data, idx.size, stream) == 0
            orc.pm.stop(stops[t])
        want = orc.drain()
        got = mb.drain(orc.pkg).cpu().numpy()
        assert np.array_equal(got, want), ("drained rows, tick", t, np.argwhere((got != want).any(1))[:6].ravel())
        assert wmx.wmx_mix_export_duck(mb._h, divisor.ctypes.data, stream) == 0
        assert np.array_equal(divisor, orc.pm.export_duck()), ("export_duck, tick", t, divisor, orc.pm.export_duck())
        rows, rlens = repaired_rows(src[t], lists[t])
        orc.tick(layout, rows, rlens, mute, duck)
        dsrc, dlens = torch.from_numpy(src[t]).to(cuda), torch.from_numpy(lens[t].view(np.int32)).to(cuda)
        if with_lists:
            words = np.array([pack(calls) for calls in lists[t]], np.uint32)
            mb.load_minus_legs_calls(dsrc, 320, 8000, 1, dlens, torch.from_numpy(words.view(np.int32)).to(cuda), mute=dmute)
        else:
            mb.load_minus_legs(dsrc, 320, 8000, 1, dlens, mute=dmute)
        assert wmx.wmx_mix_load_prompts(mb._h, stream) == 0
        for k in range(N):
            rings[t, k] = mb.export(k)[0]
            assert np.array_equal(rings[t, k], orc.rings.ring(k)), ("ring", k, "after tick", t, np.flatnonzero(rings[t, k] != orc.rings.ring(k))[:6])
    h, tk, dropped = mb.export_leg_cursors()
    wh, wt = orc.cursors()
    assert np.array_equal(h, wh) and np.array_equal(tk, wt) and not dropped.any()
    mb.close()
    return rings, orc


#                     with_lists  head_off             play_correct
FORMS = [pytest.param(False, 16000 - 960, 320, id="legs"),             # behind the first drain the head is two ticks from the ring's end
                                                                       # and a fresh cursor one: a leg's second packet wraps
         pytest.param(True, 16000 - 3200 - 480, None, id="legs_calls")]  # the platform's 200 ms: the windows wrap from the second tick on


@pytest.mark.parametrize("with_lists,head_off,play_correct", FORMS)
def test_ducked_rings_against_one_reference_mixer_per_leg(cuda, wmx, oracle_port, with_lists, head_off, play_correct):
    layout, lone = the_layout()
    plays, stops, muted = the_plays(layout, lone)
    ducking = sorted({g for ps in plays.values() for legs, _, _, _, reduce in ps if reduce for g in legs})
    never = [g for g in range(N) if g not in ducking]
    rings, orc = run_both(cuda, wmx, oracle_port, with_lists, head_off, play_correct, 41)
    # on the oracle alone: the story did what it is for
    assert orc.ducked_ticks > 40 and orc.prompt_calls > 60 and muted in ducking and lone in ducking
    assert orc.pm.legs[layout[0][0]].reduce == 4 and orc.pm.legs[layout[7][15]].clip == -1
    # the rings of the members that are not ducked are those of a run in which nobody ducks; every ducked member's but the lone leg's differ
    plain, _ = run_both(cuda, wmx, oracle_port, with_lists, head_off, play_correct, 41, duck=False)
    assert np.array_equal(rings[:, never], plain[:, never])
    for g in ducking:
        assert np.array_equal(rings[:, g], plain[:, g]) == (g == lone), g
    # the rings start empty, so one that holds samples at both of its ends within two ticks was written across its end
    wrapped = [g for g in ducking for t in (0, 1) if g != lone and rings[t, g, :80].any() and rings[t, g, -80:].any()]
    assert wrapped, "no ducked ring's window lay across the ring's end"


def test_a_ducking_play_on_a_mixer_that_is_not_in_mode_1_is_an_ordinary_play(cuda, wmx):
    """the play task takes the mode only if reduceMode == 1: on a mixer whose reduce_mode is 2 nothing is ducked, export_duck says 1 and
    the rings are those of the same play with reduce 0"""
    import torch
    from wmix_amd.mix import MixBatch
    rng = np.random.default_rng(9)
    src = torch.from_numpy(rng.integers(-30000, 30000, size=(3, 1, 161), dtype=np.int16)).to(cuda)
    lens = torch.full((3, 1), 320, dtype=torch.int32, device=cuda)
    clip, out, stream = rng.integers(-9000, 9000, 500).astype(np.int16), [], torch.cuda.current_stream().cuda_stream
    for reduce in (0, 3):
        mb = MixBatch(3, 1, 8000)
        mb.set(0, 0, 2)
        mb.set_conferences([[2, 0, 1]])
        assert wmx.wmx_mix_prompts(mb._h, 1, 500) == 0 and wmx.wmx_mix_add_clip(mb._h, clip.ctypes.data, 500, None) == 0
        assert wmx.wmx_mix_play_duck(mb._h, None, 0, 0, 1, 0, reduce, stream) == 0
        divisor = np.zeros(3, np.uint8)
        for t in range(3):
            assert wmx.wmx_mix_export_duck(mb._h, divisor.ctypes.data, stream) == 0 and divisor.tolist() == [1, 1, 1]
            mb.load_minus_legs(src, 320, 8000, 1, lens)
            assert wmx.wmx_mix_load_prompts(mb._h, stream) == 0
        out.append(np.stack([mb.export(k)[0] for k in range(3)]))
        mb.close()
    assert np.array_equal(out[0], out[1]) and out[0].any()
