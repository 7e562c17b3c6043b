"""The prompt stories (tests/conf_prompt_stories.py) on the replay alone (tests/conf_prompt_replay.py): the reference's orc_load_data on
one ring per leg, the legs' calls and the prompts' calls in the stated order.  No GPU, nothing of wmix_amd: what the stories are for is
held here, so that tests/test_conf_prompts_gpu.py compares the handle with a replay that is known to reach it -- above all the guard of
the order test: its inputs saturate, so the two orders give different datagrams."""
import numpy as np

from conf_inputs import G, K, SEED, T as T_PLAIN, alaw_decode, arrivals
from conf_prompt_replay import replay_prompt_story
from conf_prompt_stories import (LONG, MOVE_AT, MUSIC, ODD, ONE, ORDER_T, OVER_AT, RESET_AT, STOP_AT, T, TAIL, clips, main_story, only_the_clip,
                                 order_story)
from conf_replay_model import replay_story
from conf_stories import plain_setup

REPLAYED = {}


def main(lib):
    if "main" not in REPLAYED:
        pk, recv, setup, before = main_story()
        REPLAYED["main"] = replay_prompt_story(lib, G, K, pk, recv, setup, before)
    return REPLAYED["main"]


def encoder(lib):
    from oracle import loader
    return lambda x: loader._g711(lib, "orc_PCM2G711a", np.ascontiguousarray(x, np.int16), np.uint8, 320)[0]


def test_the_order_story_saturates_so_the_order_shows(oracle_port):
    pk, recv, setup, before = order_story()
    last, _, m = replay_prompt_story(oracle_port, G, K, pk, recv, setup, before)
    first, _, _ = replay_prompt_story(oracle_port, G, K, pk, recv, setup, before, prompt_first=True)
    assert not np.array_equal(last[:, 4], first[:, 4]) and np.array_equal(np.delete(last, 4, 1), np.delete(first, 4, 1))
    # play_correct is ten ticks: what tick 0 loaded is sent in tick 10
    heard_last, heard_first = alaw_decode(last[10, 4, 12:]), alaw_decode(first[10, 4, 12:])
    enc = encoder(oracle_port)
    assert np.array_equal(last[10, 4, 12:], enc(np.full(160, 32767 - 30000, np.int16))), heard_last[:4]
    assert np.array_equal(first[10, 4, 12:], enc(np.full(160, 32767, np.int16))), heard_first[:4]
    assert m.export_prompts()["done"][4] == 1 and m.rp.prompt_calls == 8


def test_the_main_story_reaches_what_it_is_for(oracle_port):
    out, legs, m = main(oracle_port)
    seen, cl = m.rp.prompt_seen, clips()
    assert len(seen) == T > 50
    col = lambda name, g: [int(s[name][g]) for s in seen]  # noqa: E731
    # the 1-sample clip and the 161-sample clip: three passes, a call per tick (a whole tick and a tail for the latter), then idle
    assert col("clip", 2)[2:6] == [ONE, ONE, -1, -1] and col("done", 2)[-1] == 1
    assert col("pos", 3)[2:9] == [160, 0, 160, 0, 160, 0, 0] and col("clip", 3)[7:9] == [-1, -1] and col("left", 3)[2:8] == [3, 2, 2, 1, 1, 0]
    # gap 7 on leg 7: 477 samples are three calls, then seven ticks without one
    assert col("pos", 7)[5:17] == [160, 320, 0, 0, 0, 0, 0, 0, 0, 0, 160, 320] and col("done", 7)[-1] == 1
    # the endless clip on leg 8 until it is stopped; the play over leg 5; the reset of leg 0 (done back to 0, idle)
    assert col("clip", 8)[1:STOP_AT] == [MUSIC] * (STOP_AT - 1) and col("clip", 8)[STOP_AT] == -1 and col("done", 8)[-1] == 0
    assert col("clip", 5)[OVER_AT - 1:OVER_AT + 1] == [LONG, ODD] and col("pos", 5)[OVER_AT] == 160 and col("done", 5)[-1] == 2
    assert col("clip", 0)[RESET_AT - 1:RESET_AT + 1] == [LONG, -1] and col("done", 0)[-1] == 0
    # one clip on two legs three ticks apart: leg 1 is where leg 0 was three ticks earlier
    assert col("pos", 1)[3:RESET_AT] == col("pos", 0)[:RESET_AT - 3]
    # hold music: leg 9 is in no conference, leg 4 alone in one from tick 20: from ten ticks (play_correct) behind its play -- for leg 4,
    # behind the last the others loaded ahead -- each hears its clip and nothing else, the passes of two whole ticks joining without a
    # seam although every pass jumps.  Until tick 50: the passes that begin in ticks 42 .. 48 find head + play_correct behind the ring's
    # end and start at the ring's START (src/wmix.c:1666-1673), on top of one another -- the reference's own repeated play does that.
    enc = encoder(oracle_port)
    assert only_the_clip(enc, out, 9, cl[MUSIC], 10, until=50) and not only_the_clip(enc, out, 9, cl[MUSIC], 10, 50, 51)
    clear = int(max(legs[MOVE_AT - 1]["tick"][[2, 3]])) // 320  # the tick in which the last that legs 2 and 3 loaded ahead has played out
    assert MOVE_AT + 10 < clear < 50 - 10 and only_the_clip(enc, out, 4, cl[MUSIC], MOVE_AT + 10, clear, 50)
    assert not only_the_clip(enc, out, 4, cl[MUSIC], MOVE_AT + 10, clear - 1, 50)  # (their last packet, mixed with it)
    # and the legs' own cursors are those of the story without prompts: a prompt is no leg
    plain, plain_legs, _ = replay_story(oracle_port, G, K, *main_story()[:2], plain_setup, {MOVE_AT: lambda c: c.set_conferences([[0, 1], [2, 3], [4], [5, 6, 7, 8]]),
                                                                                           RESET_AT: lambda c: c.reset_legs([0])})
    for t in range(T):
        for name in ("head", "tick", "dropped", "env", "speaking"):
            assert np.array_equal(legs[t][name], plain_legs[t][name]), (name, t)
    assert not np.array_equal(plain, out)


def test_a_model_with_a_store_and_no_play_is_the_plain_model(oracle_port):
    pk, recv = arrivals(SEED, T_PLAIN, G)
    want, _, _ = replay_story(oracle_port, G, K, pk, recv, plain_setup)

    def setup(c):
        plain_setup(c)
        c.prompts(4, 1000)
        c.add_clip(clips()[TAIL])

    got, _, m = replay_prompt_story(oracle_port, G, K, pk, recv, setup)
    assert np.array_equal(got, want) and m.rp.prompt_calls == 0
