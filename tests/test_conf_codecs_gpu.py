"""wmx_conf_set_codecs (wmix_amd/csrc/conf.hip) through the Python mirror: a conference in which A-law legs and mu-law legs hear each
other, each in the codec its call negotiated.  Shape, layout and script are those of tests/test_conf_gpu.py with the payload-type byte
rewritten per leg; the reference is that file's tick-by-tick replay with the decode replaced by tests/leg_codec_model.py (the rule's
table over the oracle's orc_G711a2PCM / orc_G711u2PCM) and one oracle sender per leg made with the leg's law.  Bytes and integers,
np.array_equal."""
import numpy as np
import pytest

from leg_codec_model import BY_PT, LAW_A, LAW_U, PCMA, PCMU, REFERENCE, Decoders, ingest
from leg_seq_model import COUNTERS, LegsSeqModel, repaired_rows
from speakers_legs_model import SpeakersLegsModel
from test_conf_gpu import G, K, LAYOUT, SEED, T, Replay, bridge, run
from test_conf_sequence_gpu import seq_raw_of
from test_host_tick_bridge_rtp_gpu import arrivals

pytestmark = pytest.mark.gpu

ULAW_LEGS, BY_PT_LEG, STRICT_A_LEG, LATER_ULAW_LEG, CHANGE_AT, RESET_LEG, RESET_AT = [1, 3, 6], 4, 7, 2, 15, 6, 25
START = [(ULAW_LEGS, PCMU, LAW_U), ([BY_PT_LEG], BY_PT, LAW_A), ([STRICT_A_LEG], PCMA, LAW_A)]  # the rest: the default


def rewritten_script():
    """arrivals() with the payload type of every G.711 datagram rewritten: 0 on the mu-law legs (and on leg 2 from the tick it goes to
    mu-law), alternating 8 / 0 per packet on the BY_PT leg, 8 with every fifth packet 0 on the strict A-law leg.  Payload type 96
    (one packet in sixteen) stays on every leg, the default legs keep their 8s and 0s."""
    pk, recv = arrivals(SEED, T, G)
    nth = [0] * G
    for t in range(T):
        for g in range(G):
            for k in range(K):
                if recv[t, g, k] <= 0 or (pk[t, g, k, 1] & 0x7F) not in (8, 0):
                    continue
                pt = pk[t, g, k, 1] & 0x7F
                if g in ULAW_LEGS or (g == LATER_ULAW_LEG and t >= CHANGE_AT):
                    pt = 0
                elif g == BY_PT_LEG:
                    pt = 8 if nth[g] % 2 == 0 else 0
                elif g == STRICT_A_LEG:
                    pt = 0 if nth[g] % 5 == 4 else 8
                nth[g] += 1
                pk[t, g, k, 1] = 0x80 | pt
    return pk, recv


class CodecReplay(Replay):
    """Replay of tests/test_conf_gpu.py with a codec per leg: the decode is the rule's, a leg's oracle sender is made with its law"""

    def __init__(self, lib, n):
        super().__init__(lib, n)
        self.dec, self.in_codec, self.out_law, self.refused = Decoders(lib), [REFERENCE] * n, [LAW_A] * n, np.zeros(n, np.uint32)

    def set_codecs(self, legs, in_codec, out_law):
        for g in legs:
            self.in_codec[g] = in_codec
            if out_law != self.out_law[g]:  # the call goes on: seq and timestamp (the sender's first 8 bytes) stay
                was = bytes(self.senders[g][:8])
                self.init(self.senders[g], out_law)
                for i, b in enumerate(was):
                    self.senders[g][i] = b
                self.out_law[g] = out_law

    def decode(self, pk, recv, slots=K):
        rows, lens, _ = ingest(self.dec, pk, recv, self.in_codec, self.refused)
        pcm = np.zeros((self.n, slots, 161), np.int16)
        pcm[:, :, :160] = rows
        return pcm, lens

    def fresh(self, legs):
        super().fresh(legs)
        for g in legs:  # a new call keeps the leg's codec; its sender starts again in the leg's law
            self.init(self.senders[g], self.out_law[g])
            self.refused[g] = 0


def start(target):
    for legs, in_codec, out_law in START:
        target.set_codecs(legs, in_codec, out_law)


@pytest.fixture(scope="module")
def story(oracle_port):
    """the script, every datagram the replay sends, its codec state at the end and leg 6's refused count in front of its reset"""
    pk, recv = rewritten_script()
    rp, out, seen = CodecReplay(oracle_port, G), np.zeros((T, G, 172), np.uint8), {}
    start(rp)
    for t in range(T):
        if t == CHANGE_AT:
            rp.set_codecs([LATER_ULAW_LEG], PCMU, LAW_U)
        if t == RESET_AT:
            seen["refused_before_reset"] = int(rp.refused[RESET_LEG])
            rp.fresh([RESET_LEG])
        pcm, lens = rp.decode(pk[t], recv[t])
        out[t] = rp.tick(pcm, lens, LAYOUT)
    return pk, recv, out, rp, seen


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


def replay_sequenced(lib, pk, recv, select, codecs):
    """the replay with sequence(True, 3) and speakers(*select); codecs: the legs as START sets them, else every leg at the default
    -> (datagrams, the sequence model, per tick (speaking, env), the replay)"""
    rp, model, spk = CodecReplay(lib, G), LegsSeqModel(G), SpeakersLegsModel(G)
    if codecs:
        start(rp)
    out, sel = np.zeros((T, G, 172), np.uint8), []
    for t in range(T):
        pcm, lens = rp.decode(pk[t], recv[t])
        _, new_lens, lists = model.tick(seq_raw_of(pk[t], recv[t]), lens, 3)
        sp, mute = spk.step_legs(LAYOUT, pcm, new_lens, 320, select[0], select[1], select[2], None)
        sel.append((sp.copy(), spk.env.copy()))
        rows, rlens = repaired_rows(pcm, lists)
        out[t] = rp.tick(rows, rlens, LAYOUT, mute)
    return out, model, sel, rp


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
    from test_bridge_gpu import EINVAL
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
