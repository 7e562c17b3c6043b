"""The conference handle with ducking prompts (wmx_conf_play_duck / wmx_conf_export_duck, include/wmix_amd.h): the replay of
tests/conf_prompt_replay.py with the reference's reduceMode.  DuckReplay is PromptReplay whose tick first takes the duck per leg -- the
reference ring g's reduce_mode is D for the tick in which leg g's prompt makes a call and was played with reduce = D - 1 > 0
(tests/leg_duck_model.py), as wmix_task_play_wav holds wmix->reduceMode while it makes calls (src/wmixTask.c:1416-1423, 1525-1527,
1555-1557, 1592-1594) -- then makes the legs' load (every orc_load_data call reduce 1, so rdce = D on a ducked ring), then the prompts'
calls with reduce = D (rdce 1: undivided), and releases the duck.  Every sample is the oracle's.  Two replays that are WRONG on purpose
are the controls of tests/test_conf_duck_gpu.py: keep_in_gap holds the duck through the pause between two passes, divide_prompt makes
the prompt's call with reduce 1, so that it is divided like everybody else.  Nothing of wmix_amd is imported or read."""
import numpy as np

from conf_inputs import G, LAYOUT, SEED, T, arrivals, clean_script, impair, rows_of
from conf_prompt_replay import PromptReplay, with_prompts
from conf_prompt_stories import LONG, MUSIC, ODD, TAIL, store
from conf_replay_model import ConfReplay
from conf_stories import VALUE
from leg_duck_model import LegsDuckModel
from leg_prompt_model import NULL_HEAD


class DuckReplay(PromptReplay):
    def __init__(self, lib, n, keep_in_gap=False, divide_prompt=False):
        super().__init__(lib, n)
        self.pm, self.keep_in_gap, self.divide_prompt = LegsDuckModel(n), keep_in_gap, divide_prompt
        self.div, self.duck_seen, self.ducked_calls = [1] * n, [], 0

    def take(self):
        """the divisor per leg for this tick, on the prompts' state as the tick finds it"""
        self.div = [self.pm.ducks(g) for g in range(self.n)]
        if self.keep_in_gap:  # the control: the task keeps the mode while it sleeps
            self.div = [leg.reduce + 1 if leg.clip >= 0 else 1 for leg in self.pm.legs]
        for g, r in enumerate(self.orc.rings.r):
            r.reduce_mode = self.div[g]

    def play_prompts(self):
        for g, r in enumerate(self.orc.rings.r):
            call = self.pm.step(g, (r.head_off, r.tick, r.play_correct, self.orc.size))
            if call is None:
                continue
            row, (head, tick), after = call
            if head == NULL_HEAD and r.tick > 0:  # a fresh cursor as the reference's task holds it (tests/conf_prompt_replay.py)
                head, tick = r.head_off, 0
            rarg = 1 if self.divide_prompt else self.div[g]  # reduce == reduceMode: the prompt's own call is not divided
            end = self.orc.rings.load(g, row, 2 * (len(row) - 1), 8000, 1, head, tick, rarg)
            assert end == after, ("leg", g, "the oracle's call ends at", end, "the rule's text at", after)
            self.prompt_calls += 1
            self.ducked_calls += self.div[g] > 1

    def tick(self, pcm, lens, layout, mute=None):
        self.take()
        self.orc.load(layout, pcm, lens, 320, 8000, 1, 160, mute)
        self.play_prompts()
        for r in self.orc.rings.r:
            r.reduce_mode = 1
        play, out = self.orc.drain(), np.zeros((self.n, 172), np.uint8)
        for g in range(self.n):
            row = np.ascontiguousarray(play[g])
            assert self.eg(self.senders[g], 1, 8000, row.ctypes.data, 320, 1, 8000, out[g].ctypes.data) == 172
        self.prompt_seen.append(self.pm.export())
        self.duck_seen.append(self.pm.export_duck())  # what the NEXT tick's load will apply
        return out


def with_duck(base=ConfReplay, keep_in_gap=False, divide_prompt=False):
    """-> a class like `base` whose rp is a DuckReplay, with the prompt setters of wmix_amd/conf.py, play(..., reduce) among them"""
    class WithDuck(with_prompts(base)):
        def __init__(self, lib, n_legs, max_packets=3):
            super().__init__(lib, n_legs, max_packets)
            self.rp = DuckReplay(lib, n_legs, keep_in_gap, divide_prompt)

        def play(self, legs, clip, repeat=1, gap_ticks=0, reduce=0):
            self.rp.pm.play(legs, clip, repeat, gap_ticks, reduce)

        def export_duck(self):
            return self.rp.pm.export_duck()

    return WithDuck


def replay_duck_story(lib, n_legs, max_packets, pk, recv, setup=None, before=None, base=ConfReplay, **wrong):
    """replay_prompt_story of tests/conf_prompt_replay.py on with_duck(base) -> (datagrams, export_legs() after every tick, the model;
    model.rp.duck_seen holds export_duck() after every tick)"""
    m = with_duck(base, **wrong)(lib, n_legs, max_packets)
    if setup:
        setup(m)
    out, legs = np.zeros((recv.shape[0], n_legs, 172), np.uint8), []
    for t in range(recv.shape[0]):
        if before and t in before:
            before[t](m)
        out[t] = m.tick(pk[t], recv[t])
        legs.append(m.export_legs())
    return out, legs, m


# ---- the stories: (rows, recv, setup, before), calling only setters wmix_amd/conf.py and the replay share.  G = 10 legs, 40 ticks
JOINED9 = [[0, 1], [2, 3, 4, 9], [5, 6, 7, 8]]
OVER_AT, STOP_AT, JOIN_AT, RESET_AT, LATE_AT = 8, 12, 15, 20, 25


def duck_plays(c):
    """leg 0: seven calls a pass, gap 2, the others halved; leg 5: three calls, gap 3, divided by 4; leg 2: a whole tick and a tail, gap
    1, divided by 16; leg 9, in no conference: hold music with reduce 2 and nothing to duck; leg 6: a plain play beside them"""
    store(c)
    c.play([0], LONG, 0, 2, reduce=1)
    c.play([5], ODD, 0, 3, reduce=3)
    c.play([2], TAIL, 0, 1, reduce=15)
    c.play([9], MUSIC, 0, 0, reduce=2)
    c.play([6], LONG, 1, 0)


def duck_before():
    """a play over a ducking leg with another reduce (8); a stop (12); leg 9 joins legs 2, 3 and 4 while it ducks (15); reset_legs of a
    ducking leg (20); two legs of one pair start late, with a gap (25)"""
    return {OVER_AT: lambda c: c.play([5], ODD, 4, 1, reduce=1),
            STOP_AT: lambda c: c.stop([0]),
            JOIN_AT: lambda c: c.set_conferences(JOINED9),
            RESET_AT: lambda c: c.reset_legs([2]),
            LATE_AT: lambda c: c.play([1, 3], LONG, 2, 2, reduce=7)}


def plain_duck_story():
    pk, recv = arrivals(SEED, T, G)

    def setup(c):
        c.set_conferences(LAYOUT)
        duck_plays(c)

    return pk, recv, setup, duck_before()


def stages_duck_story():
    """the same plays beside sequencing, concealment, denoise, echo control, level and the gate, on legs that lose, repeat and swap
    packets; with echo control on, what a ducked leg is sent -- the ducked mix under its prompt -- is its far row"""
    pk, recv = rows_of(impair(clean_script(51), 52)[0])

    def setup(c):
        c.set_conferences(LAYOUT)
        c.sequence(True, 3)
        c.conceal(True)
        c.denoise(True)
        c.echo(True, 20)
        c.level(True, VALUE)
        c.gate(True)
        duck_plays(c)

    return pk, recv, setup, duck_before()
