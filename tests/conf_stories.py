"""The stories the conference tests run, on the composed replay (tests/conf_replay_model.py) and on the handle alike.  A story is
(rows, recv, setup, before) -- setup(target) in front of the first tick, before[t](target) in front of tick t -- and calls only the
setters wmix_amd/conf.py and ConfReplay share.  tests/test_conf_replay_model.py holds them against what they are for on the model
alone; the test_conf_*_gpu.py modules run them on the handle."""
import numpy as np

from conf_inputs import (BY_PT_LEG, G, IN_CONF, K, LAYOUT, SEED, STRICT_A_LEG, T, ULAW_LEGS, arrivals, clean_script, gap_behind, impair,
                         retyped, rows_of, with_key)
from conf_replay_model import ConfReplay, replay_story
from leg_codec_model import BY_PT, LAW_A, LAW_U, PCMA, PCMU

WITHOUT3, JOINED = [[0, 1], [2, 4], [5, 6, 7, 8]], [[0, 1, 3], [2, 4], [5, 6, 7, 8]]
START = [(ULAW_LEGS, PCMU, LAW_U), ([BY_PT_LEG], BY_PT, LAW_A), ([STRICT_A_LEG], PCMA, LAW_A)]  # the rest: the default
VALUE = 20  # the compression gain of the level stories


def start(target):
    """the codecs the legs of the codec tests negotiated; the rest: the default"""
    for legs, in_codec, out_law in START:
        target.set_codecs(legs, in_codec, out_law)


def floor_of(lib, pk, recv, setup=None, percentile=40):
    """the level below which `percentile` in a hundred of the script's decoded packets lie"""
    m = ConfReplay(lib, recv.shape[1], recv.shape[2])
    if setup:
        setup(m)
    levels = []
    for t in range(recv.shape[0]):
        pcm, lens = m.rp.decode(pk[t], recv[t], m.K)
        levels += [int(np.abs(pcm[g, k].astype(np.int64)).sum()) for g, k in np.argwhere(lens == 320)]
    return int(np.percentile(levels, percentile))


def mask_of(legs, n=G):
    if legs is None:
        return None
    mask = np.zeros(n, np.uint8)
    mask[legs] = 1
    return mask


# ---- everything on
MUTES_A = {6: [6, 2], 21: [5, 0], 33: None}
CODEC_AT, RESET8_AT = 25, 30


def all_stages_script():
    script, _ = impair(retyped(clean_script(2), {2: CODEC_AT}), 3)
    gap_behind(script, 3, 15)
    gap_behind(script, 8, RESET8_AT)
    return rows_of(script)


def all_stages(floor, without=None):
    """-> (setup, before) of the story with everything on: mu-law legs, a BY_PT leg and a strict PCMA leg; sequence, conceal, speakers;
    the host's mute changes three times; leg 3 leaves at tick 15 (and is reset) and joins legs 0 and 1 at tick 20; leg 2 goes to
    mu-law at tick 25; leg 8 is a new call from tick 30 on.  without: one of "speakers", "conceal", "codecs", "mute" left out."""
    def setup(c):
        c.set_conferences(LAYOUT)
        if without != "codecs":
            start(c)
        c.sequence(True, 3)
        if without != "conceal":
            c.conceal(True)
        if without != "speakers":
            c.speakers(2, floor, 3)

    def leave(c):
        c.set_conferences(WITHOUT3)
        c.reset_legs([3])

    before = {15: leave, 20: lambda c: c.set_conferences(JOINED), RESET8_AT: lambda c: c.reset_legs([8])}
    if without != "codecs":
        before[CODEC_AT] = lambda c: c.set_codecs([2], PCMU, LAW_U)
    if without != "mute":
        before.update({t: (lambda c, legs=legs: c.mute(mask_of(legs))) for t, legs in MUTES_A.items()})
    return setup, before


def all_stages_floor(lib, pk, recv):
    return floor_of(lib, pk, recv, start)


# ---- switches changed on a running handle
def switching_script():
    return rows_of(impair(retyped(clean_script(11)), 12)[0])


def switching(floor):
    """the written-out story: sequence off -> sequence on -> conceal on -> speakers on -> conceal off -> conceal on -> sequence off
    (concealment stays "on" and is not launched) -> sequence on -> speakers off; beside it every other setter twice, with a change"""
    def setup(c):
        c.set_conferences(LAYOUT)

    def at(*calls):
        return lambda c: [getattr(c, name)(*args) for name, args in calls]

    before = {
        3: at(("set_codecs", (ULAW_LEGS, PCMU, LAW_U))),
        5: at(("sequence", (True, 3))),
        7: at(("mute", (mask_of([7]),))),
        10: at(("conceal", (True,))),
        12: at(("set_codecs", ([BY_PT_LEG], BY_PT, LAW_A)), ("set_codecs", ([STRICT_A_LEG], PCMA, LAW_A))),
        15: at(("speakers", (2, floor, 3))),
        17: at(("set_conferences", (WITHOUT3,)), ("reset_legs", ([3],))),
        20: at(("conceal", (False,))),
        22: at(("set_conferences", (JOINED,)), ("mute", (mask_of([0, 6]),))),
        25: at(("conceal", (True,))),
        27: at(("reset_legs", ([5],)), ("speakers", (1, floor // 2, 2))),
        29: at(("sequence", (False, 3))),
        31: at(("mute", (None,))),
        33: at(("sequence", (True, 2))),
        37: at(("speakers", (0, 0, 3))),
    }
    return setup, before


SETTERS = ("mute", "speakers", "sequence", "conceal", "set_codecs", "reset_legs", "set_conferences")


def random_schedule(seed, floor, ticks=T, n=G):
    """per tick at most one setter call drawn from SETTERS -> (setup, before, the calls as (tick, name, args))"""
    rng = np.random.default_rng(seed)
    calls = []
    for t in range(1, ticks):
        name = (SETTERS + ("nothing",) * 3)[int(rng.integers(0, len(SETTERS) + 3))]
        if name == "mute":
            args = (None if rng.integers(0, 4) == 0 else (rng.integers(0, 4, size=n) == 0).astype(np.uint8),)
        elif name == "speakers":
            args = [(0, 0, 3), (2, floor, 3), (1, floor // 2, 2), (3, 0, 4)][int(rng.integers(0, 4))]
        elif name == "sequence":
            args = (bool(rng.integers(0, 3)), int(rng.integers(0, 4)))
        elif name == "conceal":
            args = (bool(rng.integers(0, 3)),)
        elif name == "set_codecs":
            args = ([int(rng.integers(0, n))], int(rng.integers(0, 4)), int(rng.integers(0, 2)))
        elif name == "reset_legs":
            args = ([int(rng.integers(0, n))],)
        elif name == "set_conferences":
            args = ([LAYOUT, JOINED][int(rng.integers(0, 2))],)
        else:
            continue
        calls.append((t, name, args))

    def setup(c):
        c.set_conferences(LAYOUT)
        c.sequence(True, 3)
        c.conceal(True)

    return setup, {t: (lambda c, name=name, args=args: getattr(c, name)(*args)) for t, name, args in calls}, calls


RANDOM_SEEDS = (101, 102, 103)

# ---- other slot counts
TICKS_C = 16


def lose(script, seed, legs, runs):
    """losses only: `runs` times a leg of `legs` loses 1 .. 3 packets in a row (the numbers are consumed, nothing arrives)"""
    rng = np.random.default_rng(seed)
    ticks = len(script)
    for _ in range(runs):
        g, t, n = int(rng.choice(legs)), int(rng.integers(2, ticks - 4)), int(rng.integers(1, 4))
        for u in range(t, t + n):
            script[u][g] = []
    return script


def slots_script(slots):
    """K = 1: a steady script with runs of 1 .. 3 lost packets, so the lists are S D, S S D and S S S D on the only slot.  K = 2: the
    impaired script at two slots.  K = 4: the same at four, and leg 5 loses three packets and delivers the next four in one tick --
    S S S D fills the list and three packets overflow; behind them the next tick finds a gap of three again."""
    if slots == 1:
        script = lose(clean_script(21, steady=True, ticks=TICKS_C), 22, IN_CONF, 12)
        for t, n in ((4, 3), (9, 2)):  # and for certain: three in a row, two in a row
            for u in range(t, t + n):
                script[u][6] = []
    else:
        script, _ = impair(clean_script(23 + slots, ticks=TICKS_C), 24, ticks=TICKS_C, slots=slots, restarts=((1, 6),))
    if slots == 4:
        steady = clean_script(29, steady=True, ticks=TICKS_C)
        for t in range(TICKS_C):
            script[t][5] = steady[t][5]
        script[11][5] = [steady[t][5][0] for t in (11, 12, 13, 14)]
        for t in (8, 9, 10, 12, 13, 14):
            script[t][5] = []
    return rows_of(script, ticks=TICKS_C, slots=slots)


def slots_story(floor):
    def setup(c):
        c.set_conferences(LAYOUT)
        c.set_codecs(ULAW_LEGS, PCMU, LAW_U)
        c.sequence(True, 3)
        c.conceal(True)
        c.speakers(2, floor, 3)

    return setup, {5: lambda c: c.mute(mask_of([6]))}


# ---- every size class and a ragged last block
N_D, TICKS_D = 35, 12
C17 = [34, 32, 30, 28, 26, 24, 22, 20, 18, 33, 31, 29, 27, 25, 23, 21, 19]
LAYOUT_D = [[1, 0], C17, [2], [7, 5, 3, 6, 4], [16, 15, 14, 13, 12, 11, 10, 9, 8]]  # sizes 2, 17, 1, 5, 9; leg 17 is in no conference
MUTED_D = [21, 12]


def sizes_script():
    """steady, quiet, with losses; now and then a leg is loud for a tick, so that the number of eligible talkers moves"""
    rng = np.random.default_rng(31)
    script = clean_script(32, steady=True, quiet=True, legs=N_D, ticks=TICKS_D)
    for t in range(TICKS_D):
        for g in range(N_D):
            if rng.integers(0, 10) == 0:
                s, pt, _ = script[t][g][0]
                script[t][g] = [(s, pt, rng.integers(0, 256, size=160).astype(np.uint8))]
    script = lose(script, 33, [g for c in LAYOUT_D if len(c) >= 2 for g in c], 24)
    return rows_of(script, legs=N_D, ticks=TICKS_D)


FLOOR_D = 700000  # a quiet packet is below 10 000, a loud one 600 000 .. 1 270 000: a talker stays above it for a tick or two


def sizes_story():
    def setup(c):
        c.set_conferences(LAYOUT_D)
        c.sequence(True, 3)
        c.conceal(True)
        c.speakers(3, FLOOR_D, 3)
        c.mute(mask_of(MUTED_D, N_D))

    return setup, None


# ---- the stages per leg: denoise, level and gate
def turn_on(c, stage, on=True):
    c.level(on, VALUE) if stage == "level" else getattr(c, stage)(on)


def plain_setup(c):
    c.set_conferences(LAYOUT)


def alone(stage):
    """the plain script with one stage per leg on from the first tick: "denoise", "level" or "gate" """
    def setup(c):
        c.set_conferences(LAYOUT)
        turn_on(c, stage)

    return arrivals(SEED, T, G) + (setup, None)


def everything(lib, impaired=True, level=None, floor_from=None, gate=False):
    """the all-stages story with a key pressed in it, dtmf(True, True, 101) and denoise(True); level None: no more (the story of the
    denoise tests), True / False: level(level, VALUE) behind them; gate: gate(True) behind those, with the floor of the story without it.
    The floor: four in ten of the rows the selection is shown -- cleaned
    rows, levelled rows -- lie below it in the replay of the story itself, or of the story with level = floor_from."""
    script = retyped(with_key(clean_script(2)), {2: CODEC_AT})
    if impaired:
        script, _ = impair(script, 3)
    gap_behind(script, 3, 15)
    gap_behind(script, 8, RESET8_AT)
    pk, recv = rows_of(script)

    def story(floor, level, gate=False):
        # codecs, sequence, conceal, speakers(2, floor); mutes, a leg that leaves, joins elsewhere, changes its codec; two resets
        setup0, before = all_stages(floor)

        def setup(c):
            setup0(c)
            c.dtmf(True, True, 101)
            c.denoise(True)
            if level is not None:
                c.level(level, VALUE)
            if gate:
                c.gate(True)

        return setup, before

    shown = replay_story(lib, G, K, pk, recv, *story(0, level if floor_from is None else floor_from))[2].levels
    return (pk, recv) + story(int(np.percentile(shown, 40)), level, gate)


ON_AT, RESET_ON_AT, RESET_ON_LEG, OFF_AT, RESET_OFF_AT, RESET_OFF_LEG, ON_AGAIN_AT = 8, 16, 1, 22, 26, 6, 30


def switched(stage):
    """the stage on at tick 8 (level: legs 1 and 6 get a gain of their own at 12); leg 1 a new call at 16 while it is on; off at 22; leg 6
    reset at 26 while the stage is off; on again at 30"""
    before = {ON_AT: lambda c: turn_on(c, stage), RESET_ON_AT: lambda c: c.reset_legs([RESET_ON_LEG]), OFF_AT: lambda c: turn_on(c, stage, False),
              RESET_OFF_AT: lambda c: c.reset_legs([RESET_OFF_LEG]), ON_AGAIN_AT: lambda c: turn_on(c, stage)}
    if stage == "level":
        before[12] = lambda c: c.set_leg_gain([1, 6], 9)
    return arrivals(SEED, T, G) + (plain_setup, before)


def regained():
    """level on; another value for every leg at tick 14, one leg's own gain at 24"""
    def setup(c):
        c.set_conferences(LAYOUT)
        c.level(True, VALUE)

    before = {14: lambda c: c.level(True, 9), 24: lambda c: c.set_leg_gain([2], 30)}
    return arrivals(SEED, T, G) + (setup, before)
