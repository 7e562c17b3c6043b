"""wmx_conf_set_codecs (wmix_amd/csrc/conf.hip) through the Python mirror: a conference in which A-law legs and mu-law legs hear each
other, each in the codec its call negotiated.  Shape, layout and script are those of tests/conf_inputs.py with the payload-type byte
rewritten per leg (rewritten_script); the reference is codec_story() of tests/conf_single_replays.py: the tick-by-tick replay with the
decode replaced by tests/leg_codec_model.py (the rule's table over the oracle's orc_G711a2PCM / orc_G711u2PCM) and one oracle sender
per leg made with the leg's law (CodecReplay, tests/leg_oracle_model.py).  Bytes and integers, np.array_equal."""
import numpy as np
import pytest

from conf_harness import bridge, run
from conf_inputs import CHANGE_AT, EINVAL, G, K, LATER_ULAW_LEG, LAYOUT, RESET_AT, RESET_LEG, STRICT_A_LEG, T, ULAW_LEGS
from conf_single_replays import codec_story, replay_sequenced
from conf_stories import start
from leg_codec_model import BY_PT, LAW_A, LAW_U, PCMA, PCMU
from leg_oracle_model import CodecReplay, Replay
from leg_seq_model import COUNTERS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def story(oracle_port):
    return codec_story(oracle_port)


def test_the_script_reaches_what_it_is_for(oracle_port, story):
    pk, recv, want, rp, seen = story
    assert seen["refused_before_reset"] > 0 and rp.refused[STRICT_A_LEG] >= 3 and rp.refused[[0, 5, 8, 9]].any()  # the other law; payload type 96
    assert rp.in_codec == [0, PCMU, PCMU, PCMU, BY_PT, 0, PCMU, PCMA, 0, 0] and rp.out_law == [0, 1, 1, 1, 0, 0, 1, 0, 0, 0]
    for g in range(G):  # every leg is answered in its own codec: payload type, and silence is the law's code of 0 on the idle leg
        law = [LAW_U if g in ULAW_LEGS or (g == LATER_ULAW_LEG and t >= CHANGE_AT) else LAW_A for t in range(T)]
        assert want[:, g, 1].tolist() == [0x80 if x == LAW_U else 0x88 for x in law]
    assert (want[:, 9, 12:] == 0xD5).all() and all((want[:, g, 12:] != (0xFF if g in ULAW_LEGS else 0xD5)).any() for g in range(9))
    assert want[RESET_AT, RESET_LEG, 2:4].tolist() == [0, 0] and want[RESET_AT - 1, RESET_LEG, 2:4].tolist() == [0, RESET_AT - 1]
    assert want[CHANGE_AT, LATER_ULAW_LEG, 2:4].tolist() == [0, CHANGE_AT]  # a codec change is not a new call
    # with every leg left at the default the same script is sent otherwise: the mu-law legs are noise there
    plain = Replay(oracle_port, G)
    out = np.stack([plain.tick(*plain.decode(pk[t], recv[t]), LAYOUT) for t in range(T)])
    assert not np.array_equal(out[:, 0, 12:], want[:, 0, 12:])  # leg 0 hears leg 1


@pytest.mark.parametrize("slots,mode", [(1, "wait"), (3, "ahead"), (3, "resident")])
def test_every_datagram_is_the_replays(cuda, story, slots, mode):
    pk, recv, want, rp, seen = story
    cb, at_reset = bridge(slots=slots), {}
    start(cb)

    def new_call(c):
        at_reset["before"] = c.export_codecs()
        c.reset_legs([RESET_LEG])
        at_reset["after"] = c.export_codecs()

    got = run(cb, pk, recv, mode, before={CHANGE_AT: lambda c: c.set_codecs([LATER_ULAW_LEG], PCMU, LAW_U), RESET_AT: new_call})
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    st = cb.export_codecs()
    assert np.array_equal(st["refused"], rp.refused), (st["refused"], rp.refused)
    assert st["in_codec"].tolist() == rp.in_codec and st["out_law"].tolist() == rp.out_law
    assert at_reset["before"]["refused"][RESET_LEG] == seen["refused_before_reset"] and at_reset["after"]["refused"][RESET_LEG] == 0
    assert at_reset["after"]["in_codec"][RESET_LEG] == PCMU and at_reset["after"]["out_law"][RESET_LEG] == LAW_U
    others = [g for g in range(G) if g != RESET_LEG]
    assert np.array_equal(at_reset["after"]["refused"][others], at_reset["before"]["refused"][others])
    assert cb.sender_state(RESET_LEG) == (T - RESET_AT, 160 * (T - RESET_AT)) and cb.sender_state(0) == (T, 160 * T)
    assert not cb.export_legs()["dropped"].any()
    cb.close()


def test_a_refused_packet_is_not_late_not_a_duplicate_and_not_heard(cuda, oracle_port, story):
    """sequence(True, 3) and speakers(2, floor, 3) on: the sequence model and the selection model are fed d_len as the codec rule leaves
    it.  A refused packet has consumed a sequence number, so what the sequence rule sees of it is a gap: lost, never late or dup."""
    pk, recv = story[:2]
    levels = []
    probe = CodecReplay(oracle_port, G)
    start(probe)
    for t in range(T):
        pcm, lens = probe.decode(pk[t], recv[t])
        levels += [int(np.abs(pcm[g, k].astype(np.int64)).sum()) for g in range(G) for k in range(K) if lens[g, k] == 320]
    select = (2, int(np.percentile(levels, 40)), 3)

    def replay(codecs):
        return replay_sequenced(oracle_port, pk, recv, select, codecs)

    want, model, sel, rp = replay(True)
    deaf, deaf_model, _, _ = replay(False)
    counted = model.export()
    assert not counted["late"].any() and not counted["dup"].any() and counted["lost"][STRICT_A_LEG] >= rp.refused[STRICT_A_LEG] >= 3
    assert counted["lost"][STRICT_A_LEG] > deaf_model.export()["lost"][STRICT_A_LEG]  # at the default the leg's PCMU packets are calls
    assert not np.array_equal(want, deaf)
    seen = []
    cb = bridge()
    start(cb)
    cb.sequence(True, 3)
    cb.speakers(*select)
    got = run(cb, pk, recv, "ahead", after=lambda t, c: seen.append(c.export_legs()))
    for t in range(T):
        assert np.array_equal(seen[t]["speaking"], sel[t][0]) and np.array_equal(seen[t]["env"], sel[t][1]), ("speaking / env, tick", t)
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    sq = cb.export_sequence()
    for name in COUNTERS:
        assert np.array_equal(sq[name], counted[name]), (name, sq[name], counted[name])
    assert np.array_equal(cb.export_codecs()["refused"], rp.refused)
    cb.close()


def test_codec_refusals_change_nothing(cuda, wmx):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    cb = bridge()
    start(cb)
    before = cb.export_codecs()
    bad, good = np.array([3, G], np.int32), np.array([3], np.int32)
    assert wmx.wmx_conf_set_codecs(cb._h, bad.ctypes.data, 2, PCMA, LAW_A, stream) == EINVAL
    assert wmx.wmx_conf_set_codecs(cb._h, good.ctypes.data, 1, 4, LAW_A, stream) == EINVAL
    assert wmx.wmx_conf_set_codecs(cb._h, good.ctypes.data, 1, PCMA, 2, stream) == EINVAL
    assert wmx.wmx_conf_set_codecs(None, None, 0, PCMA, LAW_A, stream) == EINVAL and wmx.wmx_conf_export_codecs(None, None, None, None, stream) == EINVAL
    after = cb.export_codecs()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    cb.close()
    cb = bridge()  # never told anything: the default, with the law of create going out
    st = cb.export_codecs()
    assert not st["in_codec"].any() and not st["out_law"].any() and not st["refused"].any()
    cb.close()
