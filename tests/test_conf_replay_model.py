"""tests/conf_replay_model.py anchored without a GPU.  First the composed replay reproduces, byte for byte, each single-purpose replay
of tests/conf_single_replays.py, on that replay's own script with the matching switches.  Then the stories of tests/conf_stories.py
that tests/test_conf_all_stages_gpu.py runs on the handle are held, on the model alone, against what they are for: a failing assertion
there means the script is wrong, not the library."""
import numpy as np
import pytest

from conf_inputs import (CHANGE_AT, G, IN_CONF, K, LATER_ULAW_LEG, LAYOUT, RESET_AT, RESET_LEG, SEED, STRICT_A_LEG, T, arrivals, clean_script, impair,
                         rows_of)
from conf_replay_model import replay_story
from conf_single_replays import codec_story, replay_conceal, replay_seq, replay_sequenced, replay_with
from conf_stories import (C17, JOINED, LAYOUT_D, MUTED_D, N_D, RANDOM_SEEDS, RESET8_AT, SETTERS, TICKS_C, WITHOUT3, all_stages, all_stages_floor,
                          all_stages_script, floor_of, random_schedule, sizes_script, sizes_story, slots_script, slots_story, start, switching,
                          switching_script)
from leg_codec_model import BY_PT, LAW_A, LAW_U, PCMA, PCMU, REFERENCE
from leg_seq_model import COUNTERS


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


@pytest.fixture(scope="module")
def story(oracle_port):
    return codec_story(oracle_port)


def test_codecs_are_the_story_of_the_codec_tests(oracle_port, story):
    pk, recv, want, rp, _ = story

    def setup(c):
        c.set_conferences(LAYOUT)
        start(c)

    got, _, m = replay_story(oracle_port, G, K, pk, recv, setup,
                             {CHANGE_AT: lambda c: c.set_codecs([LATER_ULAW_LEG], PCMU, LAW_U), RESET_AT: lambda c: c.reset_legs([RESET_LEG])})
    same(got, want)
    st = m.export_codecs()
    assert np.array_equal(st["refused"], rp.refused) and st["in_codec"].tolist() == rp.in_codec and st["out_law"].tolist() == rp.out_law


def test_codecs_sequenced_and_selected_are_the_codec_tests_replay(oracle_port, story):
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
def test_the_sizes_story_reaches_what_it_is_for(oracle_port):
    pk, recv = sizes_script()
    assert sorted(len(c) for c in LAYOUT_D) == [1, 2, 5, 9, 17] and sorted([g for c in LAYOUT_D for g in c] + [17]) == list(range(N_D)) and N_D % 4
    got, legs, m = replay_story(oracle_port, N_D, K, pk, recv, *sizes_story())
    talkers = [int(st["speaking"][C17].sum()) for st in legs]
    assert 3 in talkers and min(talkers) < 3 and max(talkers) == 3, talkers
    assert m.export_conceal()[C17].sum() >= 3 and m.export_conceal()[MUTED_D].sum() >= 1 and not m.export_legs()["dropped"].any()
    assert all(m.export_conceal()[c].sum() >= 1 for c in LAYOUT_D if len(c) >= 2), m.export_conceal()
    assert (got[:, [2, 17], 12:] == 0xD5).all()  # alone and in no conference: silence
