"""wmx_conf (wmix_amd/csrc/conf.hip) with every stage on at once, and with its switches changed on a running handle, against the composed
replay of tests/conf_replay_model.py.  The stories are those of tests/test_conf_replay_model.py, which holds them against what they are
for on the model alone; here the handle runs them.  Every test compares every datagram of every tick; after every tick speaking and
env; at the end head, tick and dropped, every field of export_sequence, export_conceal and the three fields of export_codecs.  Bytes
and integers, np.array_equal."""
import numpy as np
import pytest

from conf_replay_model import replay_story
from leg_codec_model import LAW_U, PCMU
from leg_seq_model import COUNTERS
from test_conf_gpu import G, K, LAYOUT, SEED, T, bridge, run
from test_conf_replay_model import (N_D, RANDOM_SEEDS, all_stages, all_stages_floor, all_stages_script, floor_of, random_schedule,
                                    sizes_script, sizes_story, slots_script, slots_story, switching, switching_script)
from test_host_conf_codecs_gpu import ULAW, script as ulaw_every_script
from test_host_conf_gpu import host_conf
from test_host_tick_bridge_rtp_gpu import arrivals, fnv1a

pytestmark = pytest.mark.gpu

MODES = [(1, "wait"), (3, "ahead"), (3, "resident")]
REPLAYED = {}  # a story's replay, made once and shared by the modes that run it


def expected(key, lib, n, slots, story):
    """story() -> (pk, recv, setup, before)"""
    if key not in REPLAYED:
        pk, recv, setup, before = story()
        want, legs, m = replay_story(lib, n, slots, pk, recv, setup, before)
        REPLAYED[key] = {"pk": pk, "recv": recv, "setup": setup, "before": before, "want": want, "legs": legs, "model": m}
    return REPLAYED[key]


def handle_equals_replay(e, slots, mode):
    """the handle over the story of e, compared with the replay in all four ways"""
    pk, recv, m = e["pk"], e["recv"], e["model"]
    cb, seen = bridge(recv.shape[1], slots, None, recv.shape[2]), []
    e["setup"](cb)
    got = run(cb, pk, recv, mode, before=e["before"], after=lambda t, c: seen.append(c.export_legs()))
    end, sq, concealed, codecs = cb.export_legs(), cb.export_sequence(), cb.export_conceal(), cb.export_codecs()
    cb.close()
    for t in range(recv.shape[0]):
        for name in ("speaking", "env"):
            assert np.array_equal(seen[t][name], e["legs"][t][name]), (name, "tick", t, seen[t][name], e["legs"][t][name])
    assert np.array_equal(got, e["want"]), np.argwhere((got != e["want"]).any(2))[:6]
    for name in ("head", "tick", "dropped"):
        assert np.array_equal(end[name], e["legs"][-1][name]), (name, end[name], e["legs"][-1][name])
    want = m.export_sequence()
    assert sorted(want) == sorted(COUNTERS + ("next", "synced"))
    for name in want:
        assert np.array_equal(sq[name], want[name]), (name, sq[name], want[name])
    assert np.array_equal(concealed, m.export_conceal()), (concealed, m.export_conceal())
    want = m.export_codecs()
    for name in ("in_codec", "out_law", "refused"):
        assert np.array_equal(codecs[name], want[name]), (name, codecs[name], want[name])


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
FLOOR_E = 950000  # between the levels of this script's packets (tests/test_host_conf_gpu.py)


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
