"""The stories of the prompt tests, on the replay (tests/conf_prompt_replay.py) and on the handle alike: (rows, recv, setup, before) as
in tests/conf_stories.py, calling only setters wmix_amd/conf.py and the replay share.  G = 10 legs, the family's layout, 60 ticks: the
ring's end (50 ticks) is crossed while prompts play.  numpy only; nothing of wmix_amd."""
import numpy as np

from conf_inputs import G, LAYOUT, SEED, alaw_decode, arrivals, clean_script, impair, rows_of

T = 60
ALONE4 = [[0, 1], [2, 3], [4], [5, 6, 7, 8]]  # leg 4 in a conference of one
MOVE_AT, STOP_AT, OVER_AT, RESET_AT = 20, 31, 17, 23
MUSIC, LONG, ODD, ONE, TAIL = 0, 1, 2, 3, 4  # the clips of clips(), by index


def clips():
    """hold music of two whole ticks; 1 000 samples (six ticks and a quarter); 477; one sample; 161: a whole tick and a tail of one"""
    rng = np.random.default_rng(77)
    return [rng.integers(-9000, 9000, size=n).astype(np.int16) for n in (320, 1000, 477)] + [np.array([12345], np.int16),
                                                                                             rng.integers(-20000, 20000, size=161).astype(np.int16)]


def store(c, max_clips=8, max_samples=4000):
    c.prompts(max_clips, max_samples)
    assert [c.add_clip(x) for x in clips()] == [MUSIC, LONG, ODD, ONE, TAIL]


def main_story():
    """everything at once: different clips and phases on legs of one conference (5, 6, 7); one clip on legs 0 and 1, three ticks
    apart; a 1-sample and a 161-sample clip, three passes, no gap, every pass jumping in front of the play head again (2, 3); gap 7 (7); an endless clip stopped at tick 31 (8); a play over
    a playing leg at tick 17 (5); reset_legs of a playing leg at tick 23 (0); leg 9, in no conference, and leg 4, moved into a
    conference of one at tick 20, on hold music"""
    pk, recv = arrivals(SEED, T, G)

    def setup(c):
        c.set_conferences(LAYOUT)
        store(c)
        c.play([0], LONG, 0, 2)
        c.play([5], LONG, 1, 0)
        c.play([6], ODD, 2, 1)
        c.play([9], MUSIC, 0, 0)

    def moved(c):
        c.set_conferences(ALONE4)
        c.play([4], MUSIC, 0, 0)

    before = {1: lambda c: c.play([8], MUSIC, 0, 0),
              2: lambda c: (c.play([2], ONE, 3, 0), c.play([3], TAIL, 3, 0)),
              3: lambda c: c.play([1], LONG, 0, 2),
              5: lambda c: c.play([7], ODD, 2, 7),
              10: lambda c: c.play([5], LONG, 0, 0),
              OVER_AT: lambda c: c.play([5], ODD, 4, 0),
              MOVE_AT: moved,
              RESET_AT: lambda c: c.reset_legs([0]),
              STOP_AT: lambda c: c.stop([8])}
    return pk, recv, setup, before


# ---- the order: ring g receives the other legs' calls first and the prompt's call last
LOUD = 0xAA  # the A-law code of the largest sample, +32 256
ORDER_T = 14


def order_story():
    """legs 2 and 3 of the conference [2, 3, 4] send a constant near +30 000, one packet a tick; leg 4 plays a clip near -30 000.  In
    ring 4 the legs' calls first saturate (+32 767) and the prompt then leaves +2 767; the prompt first leaves +2 256 for the first leg,
    and the second saturates it: +32 767.  The other legs send nothing."""
    assert int(alaw_decode([LOUD])[0]) > 30000
    script = [[[(t, 8, np.full(160, LOUD, np.uint8))] if g in (2, 3) else [] for g in range(G)] for t in range(ORDER_T)]
    pk, recv = rows_of(script, ticks=ORDER_T)

    def setup(c):
        c.set_conferences(LAYOUT)
        c.prompts(1, 160 * 8)
        c.play([4], c.add_clip(np.full(160 * 8, -30000, np.int16)), 1, 0)

    return pk, recv, setup, None


# ---- beside the stages: sequencing with its drops, concealment, the gate, talker selection
def stages_script():
    return rows_of(impair(clean_script(51, ticks=T), 52, ticks=T)[0], ticks=T)


def stages_story(floor, prompts=True):
    def setup(c):
        c.set_conferences(LAYOUT)
        c.sequence(True, 3)
        c.conceal(True)
        c.gate(True)
        c.speakers(2, floor, 3)
        if prompts:
            store(c)
            c.play([0, 3, 6], LONG, 0, 1)
            c.play([2, 9], TAIL, 0, 0)

    before = {12: lambda c: c.play([5, 7], ODD, 3, 2), 30: lambda c: c.reset_legs([6])} if prompts else {30: lambda c: c.reset_legs([6])}
    return setup, before


# ---- with echo control on: the prompt is part of what the leg is sent, hence in its far row
def echo_story():
    pk, recv = arrivals(SEED, T, G)

    def setup(c):
        c.set_conferences(LAYOUT)
        c.echo(True, 20)
        store(c)
        c.play([1, 4, 9], LONG, 0, 1)
        c.play([6], TAIL, 5, 0)

    return pk, recv, setup, {25: lambda c: c.reset_legs([4]), 40: lambda c: c.stop([1])}


def only_the_clip(enc, out, leg, clip, first_tick, from_tick=None, until=None):
    """True when what `leg` is sent from from_tick on (default: first_tick) and before `until` (default: the end) is the clip alone,
    tiled, its first sample the first of tick first_tick: enc(int16 [160]) -> 160 codes"""
    x = np.tile(clip, (out.shape[0] * 160) // clip.size + 2)
    ticks = range(first_tick if from_tick is None else from_tick, out.shape[0] if until is None else until)
    return all(np.array_equal(out[t, leg, 12:], enc(x[(t - first_tick) * 160:(t - first_tick + 1) * 160])) for t in ticks)
