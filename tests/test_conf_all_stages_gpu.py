"""wmx_conf (wmix_amd/csrc/conf.hip) with every stage on at once, and with its switches changed on a running handle, against the composed
replay of tests/conf_replay_model.py.  The stories are those of tests/conf_stories.py, which tests/test_conf_replay_model.py holds
against what they are for on the model alone; here the handle runs them, through handle_equals_replay() of tests/conf_harness.py.
Every test compares every datagram of every tick; after every tick speaking and env; at the end head, tick and dropped, every field of
export_sequence, export_conceal and the three fields of export_codecs.  Bytes and integers, np.array_equal."""
import numpy as np
import pytest

from conf_harness import MODES, expected, handle_equals_replay, host_conf
from conf_inputs import G, K, LAYOUT, SEED, T, ULAW, arrivals, fnv1a, ulaw_every_script
from conf_replay_model import replay_story
from conf_stories import (N_D, RANDOM_SEEDS, all_stages, all_stages_floor, all_stages_script, floor_of, random_schedule, sizes_script,
                          sizes_story, slots_script, slots_story, switching, switching_script)
from leg_codec_model import LAW_U, PCMU
from leg_seq_model import COUNTERS

pytestmark = pytest.mark.gpu


# ---- a. everything on
@pytest.mark.parametrize("slots,mode", MODES)
def test_every_stage_on_at_once(cuda, oracle_port, slots, mode):
    def story():
        pk, recv = all_stages_script()
        return (pk, recv) + all_stages(all_stages_floor(oracle_port, pk, recv))

    handle_equals_replay(expected("everything", oracle_port, G, K, story), slots, mode)


# ---- b. switches changed on a running handle
@pytest.fixture(scope="module")
def switched_script(oracle_port):
    pk, recv = switching_script()
    return pk, recv, floor_of(oracle_port, pk, recv)


@pytest.mark.parametrize("slots,mode", MODES[1:])
def test_the_switches_change_on_a_running_handle(cuda, oracle_port, switched_script, slots, mode):
    """sequence off -> on -> conceal on -> speakers on -> conceal off -> on -> sequence off -> on -> speakers off.  The state of a
    stage that is off does not move: a gap behind conceal off -> on is concealed from the history as it stood when the stage last ran,
    and behind sequence off -> on the stale `next` meets the far packet and the counters show it."""
    pk, recv, floor = switched_script
    handle_equals_replay(expected("switching", oracle_port, G, K, lambda: (pk, recv) + switching(floor)), slots, mode)


@pytest.mark.parametrize("seed,mode", list(zip(RANDOM_SEEDS, ("ahead", "resident", "wait"))))
def test_a_random_schedule_of_setters(cuda, oracle_port, switched_script, seed, mode):
    pk, recv, floor = switched_script
    e = expected(("random", seed), oracle_port, G, K, lambda: (pk, recv) + random_schedule(seed, floor)[:2])
    handle_equals_replay(e, 1 if mode == "wait" else 3, mode)


# ---- c. other slot counts
@pytest.mark.parametrize("max_packets,mode", [(1, "ahead"), (2, "resident"), (4, "ahead"), (4, "resident")])
def test_other_slot_counts(cuda, oracle_port, max_packets, mode):
    def story():
        pk, recv = slots_script(max_packets)
        return (pk, recv) + slots_story(floor_of(oracle_port, pk, recv))

    handle_equals_replay(expected(("slots", max_packets), oracle_port, G, max_packets, story), 3, mode)


# ---- d. every size class and a ragged last block
@pytest.mark.parametrize("mode", ["ahead", "resident"])
def test_every_size_class_and_a_ragged_last_block(cuda, oracle_port, mode):
    handle_equals_replay(expected("sizes", oracle_port, N_D, K, lambda: sizes_script() + sizes_story()), 3, mode)


# ---- e. the C example, judged independently
FLOOR_E = 950000  # between the levels of this script's packets (600 000 .. 1 270 000)


def example_equals_replay(tmp_path, lib, flags, pk, recv, setup):
    info, got = host_conf(tmp_path, *flags)
    want, _, m = replay_story(lib, G, K, pk, recv, setup)
    assert info["rc"] == 0 and info["dropped"] == 0 and not m.export_legs()["dropped"].any()
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    assert info["datagrams_fnv1a"] == fnv1a(want)
    return info, m


def test_host_conf_with_every_flag_sends_what_the_composed_replay_sends(tmp_path, oracle_port):
    def setup(c):
        c.set_conferences(LAYOUT)
        c.speakers(2, FLOOR_E, 3)
        c.sequence(True, 3)
        c.conceal(True)
        c.set_codecs(ULAW, PCMU, LAW_U)

    flags = ("--sequence", "3", "--conceal", "--speakers", "2,%d,3" % FLOOR_E, "--ulaw-every", "3")
    info, m = example_equals_replay(tmp_path, oracle_port, flags, *ulaw_every_script(), setup)
    sq = m.export_sequence()
    assert [info[c] for c in COUNTERS] == [int(sq[c].sum()) for c in COUNTERS]
    assert info["concealed"] == int(m.export_conceal().sum()) > 0 and info["refused"] == int(m.export_codecs()["refused"].sum()) > 0
    assert info["speakers"] == 2 and info["sequence"] == 3 and info["conceal"] == 1 and info["ulaw_legs"] == len(ULAW)


def test_host_conf_sequence_conceal_sends_what_the_composed_replay_sends(tmp_path, oracle_port):
    def setup(c):
        c.set_conferences(LAYOUT)
        c.sequence(True, 3)
        c.conceal(True)

    info, m = example_equals_replay(tmp_path, oracle_port, ("--sequence", "3", "--conceal"), *arrivals(SEED, T, G), setup)
    sq = m.export_sequence()
    assert [info[c] for c in COUNTERS] == [int(sq[c].sum()) for c in COUNTERS]
    assert info["concealed"] == int(m.export_conceal().sum()) == info["lost"] > 0


def test_host_conf_speakers_sends_what_the_composed_replay_sends(tmp_path, oracle_port):
    def setup(c):
        c.set_conferences(LAYOUT)
        c.speakers(2, FLOOR_E, 3)

    info, m = example_equals_replay(tmp_path, oracle_port, ("--speakers", "2,%d,3" % FLOOR_E), *arrivals(SEED, T, G), setup)
    assert info["speakers"] == 2 and m.export_legs()["env"][:9].all()
