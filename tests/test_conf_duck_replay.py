"""The duck stories (tests/conf_duck_replay.py) on the replay alone: the reference's orc_load_data on one ring per leg with the
reference's reduceMode per ring and tick.  No GPU, nothing of wmix_amd: what the stories are for is held here, so that
tests/test_conf_duck_gpu.py compares the handle with a replay that is known to reach it -- a story without any reduce is the prompt
replay of tests/test_conf_prompt_replay.py, byte for byte, and the two replays that are wrong on purpose send other datagrams."""
import numpy as np

from conf_duck_replay import JOIN_AT, OVER_AT, RESET_AT, STOP_AT, plain_duck_story, replay_duck_story
from conf_inputs import G, K, T
from conf_prompt_replay import replay_prompt_story
from conf_prompt_stories import main_story

REPLAYED = {}


def plain(lib, **wrong):
    key = tuple(sorted(wrong))
    if key not in REPLAYED:
        REPLAYED[key] = replay_duck_story(lib, G, K, *plain_duck_story(), **wrong)
    return REPLAYED[key]


def test_a_story_in_which_every_play_has_reduce_0_is_the_prompt_replay(oracle_port):
    story = main_story()
    want, legs, m = replay_prompt_story(oracle_port, G, K, *story)
    got, legs2, d = replay_duck_story(oracle_port, G, K, *story)
    assert np.array_equal(got, want) and d.rp.prompt_calls == m.rp.prompt_calls > 150 and d.rp.ducked_calls == 0
    assert all((seen == 1).all() for seen in d.rp.duck_seen)
    for a, b in zip(d.rp.prompt_seen, m.rp.prompt_seen):
        assert all(np.array_equal(a[name], b[name]) for name in b)


def test_the_duck_story_reaches_what_it_is_for(oracle_port):
    out, legs, m = plain(oracle_port)
    seen = np.stack(m.rp.duck_seen)  # [T, G]: seen[t] is the divisor tick t + 1's load applies, as the state behind tick t says it
    assert seen.shape == (T, G) and m.rp.ducked_calls > 80
    # leg 0: seven calls at 2, a gap of two ticks at 1, and 2 again behind it; released by the stop
    assert seen[:STOP_AT, 0].tolist() == [2, 2, 2, 2, 2, 2, 1, 1, 2, 2, 2, 2] and not (seen[STOP_AT:, 0] != 1).any()
    # leg 5: three calls at 4 and a gap of three; the play over it divides by 2 from its first tick on, gap 1
    assert seen[:OVER_AT, 5].tolist() == [4, 4, 1, 1, 1, 4, 4, 4] and seen[OVER_AT:OVER_AT + 4, 5].tolist() == [2, 2, 1, 2]
    # leg 2: divided by 16 until its reset; leg 9 ducks from the first tick, in no conference and in one alike; leg 6 never
    assert set(seen[:RESET_AT, 2].tolist()) == {1, 16} and not (seen[RESET_AT:, 2] != 1).any()
    assert (seen[:, 9] == 3).all() and (seen[:, 6] == 1).all() and JOIN_AT < T - 12
    # without any reduce the same story sends other datagrams to the ducked legs that are in a conference, the same to everybody else
    pk, recv, setup, before = plain_duck_story()

    class NoReduce:
        def __init__(self, c):
            self.c = c

        def __getattr__(self, name):
            return getattr(self.c, name)

        def play(self, legs, clip, repeat=1, gap_ticks=0, reduce=0):
            self.c.play(legs, clip, repeat, gap_ticks)

    undu, _, _ = replay_duck_story(oracle_port, G, K, pk, recv, lambda c: setup(NoReduce(c)), {t: (lambda c, f=f: f(NoReduce(c))) for t, f in before.items()})
    differ = [g for g in range(G) if not np.array_equal(out[:, g], undu[:, g])]
    assert differ == [0, 1, 2, 3, 5, 9]
    # leg 9 hears its clip alone until legs 2, 3 and 4 reach it: what it is sent changes only from play_correct behind the join on
    assert np.array_equal(out[:JOIN_AT + 10, 9], undu[:JOIN_AT + 10, 9])


def test_the_controls_send_other_datagrams(oracle_port):
    """a replay that keeps ducking through the gap, and one that divides the prompt too, differ from the replay -- so a handle that
    equals the replay does neither"""
    out, _, _ = plain(oracle_port)
    kept, _, _ = plain(oracle_port, keep_in_gap=True)
    divided, _, _ = plain(oracle_port, divide_prompt=True)
    # a gap is heard only by a leg that has one while the others talk -- legs 0 and 5 among them -- and never by leg 9, whose music has no
    # gap, nor by a leg that never ducks
    gap_heard = {g for g in range(G) if not np.array_equal(out[:, g], kept[:, g])}
    assert {0, 5} <= gap_heard <= {0, 1, 2, 3, 5}, gap_heard
    assert [g for g in range(G) if not np.array_equal(out[:, g], divided[:, g])] == [0, 1, 2, 3, 5, 9]
