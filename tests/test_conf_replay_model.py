"""tests/conf_replay_model.py anchored without a GPU.  First the composed replay reproduces, byte for byte, each single-purpose replay
the suite already has, on that replay's own script with the matching switches.  Then the stories tests/test_conf_all_stages_gpu.py
runs on the handle are held, on the model alone, against what they are for: a failing assertion there means the script is wrong, not
the library.  The stories live here: a story is (rows, recv, setup, before) -- setup(target) in front of the first tick, before[t](target)
in front of tick t -- and calls only the setters wmix_amd/conf.py and ConfReplay share."""
import numpy as np
import pytest

from conf_replay_model import ConfReplay, replay_story
from leg_codec_model import BY_PT, LAW_A, LAW_U, PCMA, PCMU, REFERENCE
from leg_seq_model import COUNTERS
from test_conf_codecs_gpu import BY_PT_LEG, STRICT_A_LEG, ULAW_LEGS, replay_sequenced, start
from test_conf_codecs_gpu import story  # noqa: F401  (the fixture)
from test_conf_conceal_gpu import replay_conceal
from test_conf_gpu import G, K, LAYOUT, SEED, T, replay_with
from test_conf_sequence_gpu import IN_CONF, clean_script, impair, replay_seq, rows_of
from test_host_tick_bridge_rtp_gpu import arrivals

WITHOUT3, JOINED = [[0, 1], [2, 4], [5, 6, 7, 8]], [[0, 1, 3], [2, 4], [5, 6, 7, 8]]


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


def same(got, want):
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]


def same_selection(legs, sel):
    for t, (speaking, env) in enumerate(sel):
        assert np.array_equal(legs[t]["speaking"], speaking) and np.array_equal(legs[t]["env"], env), ("speaking / env, tick", t)


def same_counters(m, model):
    want = model.export()
    for name, got in m.export_sequence().items():
        assert np.array_equal(got, want[name]), (name, got, want[name])


# ------------------------------------------------------------------ the anchors
@pytest.fixture(scope="module")
def plain_script():
    return arrivals(SEED, T, G)


@pytest.fixture(scope="module")
def impaired():
    return rows_of(impair(clean_script(2), 3)[0])


def test_plain_is_replay_with(oracle_port, plain_script):
    pk, recv = plain_script
    got, _, m = replay_story(oracle_port, G, K, pk, recv, lambda c: c.set_conferences(LAYOUT))
    same(got, replay_with(oracle_port, pk, recv, lambda t: LAYOUT)[0])
    assert not m.export_conceal().any() and not any(v.any() for v in m.export_sequence().values()) and m.export_codecs()["refused"].any()


def test_selection_is_replay_with_select(oracle_port, plain_script):
    pk, recv = plain_script[0][:30], plain_script[1][:30]
    select = (2, floor_of(oracle_port, pk, recv), 3)
    want, sel = replay_with(oracle_port, pk, recv, lambda t: LAYOUT, select=select)

    def setup(c):
        c.set_conferences(LAYOUT)
        c.speakers(*select)

    got, legs, _ = replay_story(oracle_port, G, K, pk, recv, setup)
    same(got, want)
    same_selection(legs, sel)


def test_the_hosts_mute_is_replay_with_mute_at(oracle_port, plain_script):
    pk, recv = plain_script
    masks = {10: np.eye(G, dtype=np.uint8)[6], 22: np.eye(G, dtype=np.uint8)[3], 31: None}

    def mute_at(t):
        since = [s for s in masks if s <= t]
        return masks[max(since)] if since else None

    want, _ = replay_with(oracle_port, pk, recv, lambda t: LAYOUT, mute_at=mute_at)
    got, _, _ = replay_story(oracle_port, G, K, pk, recv, lambda c: c.set_conferences(LAYOUT),
                             {t: (lambda c, m=m: c.mute(m)) for t, m in masks.items()})
    same(got, want)


def test_a_new_call_in_a_used_slot_is_replay_with_fresh_at(oracle_port, plain_script):
    pk, recv = plain_script
    layout_at = lambda t: LAYOUT if t < 15 else (WITHOUT3 if t < 20 else JOINED)  # noqa: E731
    want, _ = replay_with(oracle_port, pk, recv, layout_at, fresh_at={15: [3]})

    def leave(c):
        c.set_conferences(WITHOUT3)
        c.reset_legs([3])

    got, _, _ = replay_story(oracle_port, G, K, pk, recv, lambda c: c.set_conferences(LAYOUT), {15: leave, 20: lambda c: c.set_conferences(JOINED)})
    same(got, want)


@pytest.mark.parametrize("selecting", [False, True])
def test_sequencing_is_replay_seq(oracle_port, impaired, selecting):
    pk, recv = impaired
    select = (2, floor_of(oracle_port, pk, recv), 3) if selecting else None
    want, model, sel = replay_seq(oracle_port, pk, recv, select=select)

    def setup(c):
        c.set_conferences(LAYOUT)
        c.sequence(True, 3)
        if select:
            c.speakers(*select)

    got, legs, m = replay_story(oracle_port, G, K, pk, recv, setup)
    same(got, want)
    same_counters(m, model)
    same_selection(legs, sel)
    assert not m.export_conceal().any()


def concealing(c):
    c.set_conferences(LAYOUT)
    c.sequence(True, 3)
    c.conceal(True)


def test_concealment_is_replay_conceal(oracle_port, impaired):
    pk, recv = impaired
    want, seq, plc, _ = replay_conceal(oracle_port, pk, recv)
    got, _, m = replay_story(oracle_port, G, K, pk, recv, concealing)
    same(got, want)
    same_counters(m, seq)
    assert np.array_equal(m.export_conceal(), plc.export()["concealed"]) and m.export_conceal()[IN_CONF].sum() >= 3


def test_concealment_behind_a_reset_is_replay_conceal_with_fresh_at(oracle_port):
    script = clean_script(7, steady=True)  # the script of test_a_reset_leg_conceals_from_a_fresh_history
    for t in range(15, T):
        script[t][3] = [((s + 30000) % 65536, pt, codes) for s, pt, codes in script[t][3]]
    script[9][3], script[16][3] = [], []
    pk, recv = rows_of(script)
    want, seq, plc, _ = replay_conceal(oracle_port, pk, recv, fresh_at={15: [3]})
    got, _, m = replay_story(oracle_port, G, K, pk, recv, concealing, {15: lambda c: c.reset_legs([3])})
    same(got, want)
    same_counters(m, seq)
    assert np.array_equal(m.export_conceal(), plc.export()["concealed"]) and m.export_conceal()[3] == 1


def test_codecs_are_the_story_of_the_codec_tests(oracle_port, story):  # noqa: F811
    from test_conf_codecs_gpu import CHANGE_AT, LATER_ULAW_LEG, RESET_AT, RESET_LEG
    pk, recv, want, rp, _ = story

    def setup(c):
        c.set_conferences(LAYOUT)
        start(c)

    got, _, m = replay_story(oracle_port, G, K, pk, recv, setup,
                             {CHANGE_AT: lambda c: c.set_codecs([LATER_ULAW_LEG], PCMU, LAW_U), RESET_AT: lambda c: c.reset_legs([RESET_LEG])})
    same(got, want)
    st = m.export_codecs()
    assert np.array_equal(st["refused"], rp.refused) and st["in_codec"].tolist() == rp.in_codec and st["out_law"].tolist() == rp.out_law


def test_codecs_sequenced_and_selected_are_the_codec_tests_replay(oracle_port, story):  # noqa: F811
    pk, recv = story[:2]

    def setup(c):
        c.set_conferences(LAYOUT)
        start(c)

    select = (2, floor_of(oracle_port, pk, recv, setup), 3)
    want, model, sel, rp = replay_sequenced(oracle_port, pk, recv, select, True)

    def switched(c):
        setup(c)
        c.sequence(True, 3)
        c.speakers(*select)

    got, legs, m = replay_story(oracle_port, G, K, pk, recv, switched)
    same(got, want)
    same_counters(m, model)
    same_selection(legs, sel)
    assert np.array_equal(m.export_codecs()["refused"], rp.refused)


# ------------------------------------------------------------------ what a story reaches, counted on the model
class Reach:
    """watch() of replay_story.  Over the legs that are in a conference of two or more, per tick: the silence calls of the tick's lists
    (gaps) by what becomes of them, and for how many ticks each switch was on and off."""

    def __init__(self):
        self.n = dict.fromkeys(("masked", "host_muted", "speaking", "ulaw", "zeros", "after_back_on", "longest_run"), 0)
        self.ticks = {name: [0, 0] for name in ("sequence", "conceal", "speakers")}  # [off, on]
        self.gaps_at, self.conceal_was_off, self.concealed_moved_while_off = {}, False, False
        self.concealed = None

    def __call__(self, t, m, pk_t, recv_t):
        for name, on in (("sequence", m.seq_on), ("conceal", m.conceal_on), ("speakers", m.max_speakers > 0)):
            self.ticks[name][int(on)] += 1
        concealed = m.export_conceal()
        if not (m.seq_on and m.conceal_on):
            self.conceal_was_off = self.conceal_was_off or self.ticks["conceal"][1] > 0
            if self.concealed is not None and not np.array_equal(concealed, self.concealed):
                self.concealed_moved_while_off = True
        self.concealed = concealed
        if not m.seq_on:
            return
        for g in sorted(g for c in m.layout if len(c) >= 2 for g in c):
            kinds = "".join(kind for kind, _ in m.lists[g])
            gaps = kinds.count("S")
            if not gaps:
                continue
            self.gaps_at.setdefault(t, []).append(g)
            if not m.conceal_on:
                self.n["zeros"] += gaps
                continue
            self.n["longest_run"] = max(self.n["longest_run"], max(len(run) for run in kinds.split("D")))
            self.n["after_back_on"] += gaps if self.conceal_was_off else 0
            host = m.host_mute is not None and bool(m.host_mute[g])
            self.n["host_muted"] += gaps if host else 0
            self.n["masked"] += gaps if m.max_speakers > 0 and m.load_mute[g] and not host else 0
            self.n["speaking"] += gaps if m.max_speakers > 0 and not m.load_mute[g] else 0
            self.n["ulaw"] += gaps if m.rp.in_codec[g] == PCMU else 0


def retyped(packets, ulaw_from=None):
    """the payload types of a script rewritten per leg, by the rule of rewritten_script() in tests/test_conf_codecs_gpu.py: 0 on the
    mu-law legs (and on the legs of ulaw_from = {leg: tick} from that tick), alternating 8 / 0 per packet on the BY_PT leg, 8 with
    every fifth packet 0 on the strict A-law leg; the default legs keep their 8s and 0s"""
    nth, out = {}, []
    for t, tick in enumerate(packets):
        out.append([])
        for g, now in enumerate(tick):
            new = []
            for s, pt, codes in now:
                n = nth.get(g, 0)
                if g in ULAW_LEGS or (ulaw_from and g in ulaw_from and t >= ulaw_from[g]):
                    pt = 0
                elif g == BY_PT_LEG:
                    pt = 8 if n % 2 == 0 else 0
                elif g == STRICT_A_LEG:
                    pt = 0 if n % 5 == 4 else 8
                nth[g] = n + 1
                new.append((s, pt, codes))
            out[-1].append(new)
    return out


def gap_behind(script, g, t):
    """leg g delivers one packet in tick t and in tick t + 1 what it delivered anyway, which starts two numbers on: a gap of one in the
    tick behind a reset_legs at t (where it delivered nothing in tick t + 1: the packet in front of its next one)"""
    if not script[t + 1][g]:
        s, pt, codes = next(now[g][0] for now in script[t + 2:] if now[g])
        script[t + 1][g] = [((s - 1) % 65536, pt, codes[::-1].copy())]
    s, pt, codes = script[t + 1][g][0]
    script[t][g] = [((s - 2) % 65536, pt, codes[::-1].copy())]


# ---- 3a: everything on
MUTES_A = {6: [6, 2], 21: [5, 0], 33: None}
CODEC_AT, RESET8_AT = 25, 30


def all_stages_script():
    script, _ = impair(retyped(clean_script(2), {2: CODEC_AT}), 3)
    gap_behind(script, 3, 15)
    gap_behind(script, 8, RESET8_AT)
    return rows_of(script)


def mask_of(legs, n=G):
    if legs is None:
        return None
    mask = np.zeros(n, np.uint8)
    mask[legs] = 1
    return mask


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


def test_the_all_stages_story_reaches_what_it_is_for(oracle_port):
    pk, recv = all_stages_script()
    floor = all_stages_floor(oracle_port, pk, recv)
    setup, before = all_stages(floor)
    reach, lists_at = Reach(), {}

    def watch(t, m, pk_t, recv_t):
        reach(t, m, pk_t, recv_t)
        lists_at[t] = [list(calls) for calls in m.lists]

    want, _, m = replay_story(oracle_port, G, K, pk, recv, setup, before, watch)
    n = reach.n
    assert n["masked"] >= 5 and n["host_muted"] >= 3 and n["speaking"] >= 5 and n["ulaw"] >= 3 and n["longest_run"] >= 2, n
    assert ("S", None) in lists_at[16][3] and ("S", None) in lists_at[RESET8_AT + 1][8]  # a gap in the tick behind the leg's reset
    st = m.export_sequence()
    assert all(st[name].any() for name in COUNTERS if name != "overflow") and not st["overflow"].any(), {c: st[c] for c in COUNTERS}
    assert not m.export_legs()["dropped"].any() and st["synced"].all()
    assert np.array_equal(m.export_conceal(), st["lost"])  # both on throughout, both zeroed by a reset
    # a gap that exists only because a packet was refused: the strict leg conceals more than it does when it takes both payload types
    def lenient(c):
        setup(c)
        c.set_codecs([STRICT_A_LEG], BY_PT, LAW_A)

    _, _, other = replay_story(oracle_port, G, K, pk, recv, lenient, before)
    refused = m.export_codecs()["refused"]
    assert refused[STRICT_A_LEG] >= 1 and other.export_codecs()["refused"][STRICT_A_LEG] == 0
    assert m.export_conceal()[STRICT_A_LEG] >= other.export_conceal()[STRICT_A_LEG] + 1
    codecs = m.export_codecs()
    assert codecs["in_codec"].tolist() == [REFERENCE, PCMU, PCMU, PCMU, BY_PT, REFERENCE, PCMU, PCMA, REFERENCE, REFERENCE]
    # each stage matters to the bytes
    for without in ("speakers", "conceal", "codecs", "mute"):
        other, _, _ = replay_story(oracle_port, G, K, pk, recv, *all_stages(floor, without))
        assert not np.array_equal(other, want), without


# ---- 3b: switches changed on a running handle
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


class Recorder:
    """stands where the handle stands and writes down what a story calls"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args))


def test_the_switching_story_reaches_what_it_is_for(oracle_port):
    pk, recv = switching_script()
    floor = floor_of(oracle_port, pk, recv)
    setup, before = switching(floor)
    rec = Recorder()
    setup(rec)
    for t in sorted(before):
        before[t](rec)
    for name in SETTERS:  # every setter at least twice, with a change of value
        args = [repr(a) for n, a in rec.calls if n == name]
        assert len(args) >= 2 and (name == "reset_legs" or any(a != b for a, b in zip(args, args[1:]))), name
    reach = Reach()
    want, _, m = replay_story(oracle_port, G, K, pk, recv, setup, before, reach)
    assert all(min(reach.ticks[name]) >= 5 for name in ("sequence", "conceal", "speakers")), reach.ticks
    assert reach.n["zeros"] >= 1 and not reach.concealed_moved_while_off and reach.n["after_back_on"] >= 1, reach.n
    assert any(20 <= t < 25 for t in reach.gaps_at) and any(25 <= t < 29 for t in reach.gaps_at), sorted(reach.gaps_at)
    st = m.export_sequence()
    assert st["resync"].sum() >= 1 and m.export_conceal().sum() >= 3 and not m.export_legs()["dropped"].any()
    # sequencing came back on over a stale `next`: the counters show it, against the run whose sequencer never paused
    never_off = {t: call for t, call in before.items() if t not in (29, 33)}
    _, _, other = replay_story(oracle_port, G, K, pk, recv, setup, never_off)
    assert any(not np.array_equal(st[name], other.export_sequence()[name]) for name in COUNTERS)


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_a_random_schedule_is_runnable_and_switches(oracle_port, seed):
    pk, recv = switching_script()
    setup, before, calls = random_schedule(seed, floor_of(oracle_port, pk, recv))
    assert len(set(name for _, name, _ in calls)) >= 6 and len(calls) >= 15, calls
    reach = Reach()
    _, _, m = replay_story(oracle_port, G, K, pk, recv, setup, before, reach)
    assert not m.export_legs()["dropped"].any() and m.export_conceal().sum() >= 1
    assert all(min(reach.ticks[name]) >= 1 for name in reach.ticks), reach.ticks


# ---- 3c: other slot counts
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


@pytest.mark.parametrize("slots", [1, 2, 4])
def test_the_slot_count_stories_reach_what_they_are_for(oracle_port, slots):
    pk, recv = slots_script(slots)
    assert pk.shape == (TICKS_C, G, slots, 172) and (recv[:, :, slots - 1] > 0).any()
    lists_at, concealed_at = {}, {}

    def watch(t, m, pk_t, recv_t):
        lists_at[t], concealed_at[t] = [list(calls) for calls in m.lists], m.export_conceal()

    _, _, m = replay_story(oracle_port, G, slots, pk, recv, *slots_story(floor_of(oracle_port, pk, recv)), watch)
    st = m.export_sequence()
    assert m.export_conceal()[IN_CONF].sum() >= 5 and not m.export_legs()["dropped"].any()
    if slots == 1:
        assert any(calls == [("S", None)] * 3 + [("D", 0)] for lists in lists_at.values() for calls in lists)
        assert any(calls == [("S", None)] * 2 + [("D", 0)] for lists in lists_at.values() for calls in lists)
    if slots == 4:
        assert st["overflow"][5] == 3 and lists_at[11][5][:3] == [("S", None)] * 3 and lists_at[11][5][3][0] == "D" and len(lists_at[11][5]) == 4
        assert concealed_at[11][5] - concealed_at[10][5] == 3  # concealment sees the truncated list: three rows, not six
        assert lists_at[15][5][:3] == [("S", None)] * 3 and concealed_at[15][5] == 6
        assert any(len(calls) == 4 and all(kind == "D" for kind, _ in calls) for lists in lists_at.values() for calls in lists) or st["dup"].any()
    if slots == 1:
        assert not st["overflow"].any()


# ---- 3d: every size class and a ragged last block
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


def test_the_sizes_story_reaches_what_it_is_for(oracle_port):
    pk, recv = sizes_script()
    assert sorted(len(c) for c in LAYOUT_D) == [1, 2, 5, 9, 17] and sorted([g for c in LAYOUT_D for g in c] + [17]) == list(range(N_D)) and N_D % 4
    got, legs, m = replay_story(oracle_port, N_D, K, pk, recv, *sizes_story())
    talkers = [int(st["speaking"][C17].sum()) for st in legs]
    assert 3 in talkers and min(talkers) < 3 and max(talkers) == 3, talkers
    assert m.export_conceal()[C17].sum() >= 3 and m.export_conceal()[MUTED_D].sum() >= 1 and not m.export_legs()["dropped"].any()
    assert all(m.export_conceal()[c].sum() >= 1 for c in LAYOUT_D if len(c) >= 2), m.export_conceal()
    assert (got[:, [2, 17], 12:] == 0xD5).all()  # alone and in no conference: silence
