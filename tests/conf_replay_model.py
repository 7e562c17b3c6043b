"""The conference handle (wmx_conf, include/wmix_amd.h "a conference bridge of RTP/G.711 legs as a pipeline") with every stage it has,
composed of the models each stage already has, in the order the header states:

    decode by the leg's codec (CodecReplay of tests/leg_oracle_model.py; a refused packet is invisible from here on)
    -> if sequencing is on: tests/leg_seq_model.py, which rewrites the lens and makes the call lists
    -> the stages per leg, each if it is on, each on the rows the one before it left: tests/leg_dtmf_model.py (on the row as it
       arrived; a suppressed key leaves zeros), tests/leg_denoise_model.py, tests/leg_level_model.py, tests/leg_gate_model.py
    -> if max_speakers > 0: tests/speakers_legs_model.py on the rows as those stages left them and the rewritten lens; the host's mute
       goes in, the mask comes out
    -> the load: sequencing and concealment on: the four rows of tests/leg_plc_model.py, all data, under the mask;
                 sequencing alone: repaired_rows(); neither: the rows as decoded
    -> the drain -> the oracle's egress, one sender per leg in that leg's law (Replay / LegsOracle).

State moves only for a stage that is launched: with sequencing off neither the sequence model nor the concealment model is ticked, with
concealment off the concealment model is not, and a stage per leg that is off is not ticked either.  The leveller's model is made by
the first level(True, ...), as the handle makes its AGC, and the gate's by the first gate(True), as it makes its VAD: before that
export_gate() says what the handle says, reduce 4 and counts 0.  The setters are those of wmix_amd/conf.py, so one story (a function that calls
setters, tests/conf_stories.py) drives the handle and this class alike.  This is the only text of the per-tick rule in the tests: a new
stage is one setter and one line in tick().  Nothing of wmix_amd is imported or read."""
import numpy as np

from conf_inputs import seq_raw_of
from leg_denoise_model import LegsDenoiseModel
from leg_dtmf_model import LegsDtmfModel
from leg_gate_model import LegsGateModel
from leg_level_model import LegsLevelModel
from leg_oracle_model import CodecReplay
from leg_plc_model import LegsPlcModel
from leg_seq_model import LegsSeqModel, repaired_rows
from speakers_legs_model import SpeakersLegsModel


class ConfReplay:
    def __init__(self, lib, n_legs, max_packets=3):
        self.lib, self.n, self.K = lib, n_legs, max_packets
        self.rp = CodecReplay(lib, n_legs)  # every leg REFERENCE in, A-law out: the handle as created
        self.seq, self.plc, self.spk = LegsSeqModel(n_legs), LegsPlcModel(n_legs), SpeakersLegsModel(n_legs)
        self.layout, self.host_mute = [], None
        self.max_speakers, self.floor, self.decay_shift = 0, 0, 3
        self.seq_on, self.max_gap, self.conceal_on = False, 3, False
        self.keys, self.dn, self.lv, self.gt = LegsDtmfModel(n_legs), LegsDenoiseModel(lib, n_legs), None, None
        self.dtmf_on, self.dtmf_suppress, self.dtmf_pt, self.denoise_on, self.level_on, self.level_value = False, False, 101, False, False, None
        self.gate_on, self.gate_seen = False, []  # export_gate() behind every tick
        self.levels = []  # of every row the selection was shown, as it was shown it: for a story's choice of floor
        self.lists = [[] for _ in range(n_legs)]  # the call lists of the last tick in which the sequencer ran: for the tests' reach
        self.load_mute = None  # what the last tick's load was given

    # ---- the setters of wmix_amd/conf.py
    def set_conferences(self, conferences):
        self.layout = [list(c) for c in conferences]

    def mute(self, mask=None):
        self.host_mute = None if mask is None else np.array(mask, np.uint8)

    def speakers(self, max_speakers, floor=0, decay_shift=3):
        assert 0 <= max_speakers <= 32 and 0 <= decay_shift <= 31
        self.max_speakers, self.floor, self.decay_shift = max_speakers, floor, decay_shift

    def sequence(self, on, max_gap=3):
        assert 0 <= max_gap <= 3
        self.seq_on, self.max_gap = bool(on), max_gap

    def conceal(self, on):
        self.conceal_on = bool(on)

    def set_codecs(self, legs, in_codec, out_law):
        self.rp.set_codecs(range(self.n) if legs is None else legs, in_codec, out_law)

    def dtmf(self, on, suppress=False, event_pt=101):
        self.dtmf_on, self.dtmf_suppress, self.dtmf_pt = bool(on), bool(suppress), event_pt

    def denoise(self, on):
        self.denoise_on = bool(on)

    def level(self, on, value=20):
        if on:
            if self.lv is None:
                self.lv = LegsLevelModel(self.lib, self.n, value)
            elif value != self.level_value:
                self.lv.set_gain(value)  # agc_addition for every leg
            self.level_value = value
        self.level_on = bool(on)

    def set_leg_gain(self, legs, value):
        self.lv.set_gain(value, legs)

    def gate(self, on):
        if on and self.gt is None:
            self.gt = LegsGateModel(self.lib, self.n)
        self.gate_on = bool(on)

    def reset_legs(self, legs=None):
        """a new call in a used slot: cursor, dropped, env, ring, sender, sequence state, refused, concealment state, keypad, suppressor,
        AGC and gate (shut, its counts zero); the codec and the leg's gain stay"""
        legs = list(range(self.n) if legs is None else legs)
        self.rp.fresh(legs)
        for model in (self.spk, self.seq, self.plc, self.keys, self.dn, self.lv, self.gt):
            if model is not None:
                model.reset(legs)

    # ---- one tick
    def tick(self, pk_t, recv_t):
        """datagram rows [n_legs, max_packets, >= 172] and what recvfrom returned [n_legs, max_packets] -> datagrams [n_legs, 172]"""
        assert recv_t.shape == (self.n, self.K) and self.layout
        pcm, lens = self.rp.decode(pk_t, recv_t, self.K)
        heard = lens
        if self.seq_on:
            _, heard, self.lists = self.seq.tick(seq_raw_of(pk_t, recv_t), lens, self.max_gap)
        lists = self.lists if self.seq_on else None
        if self.dtmf_on:  # on the row as it arrived
            self.keys.tick(pk_t, recv_t, pcm, heard, lists, self.dtmf_pt, self.dtmf_suppress)
        if self.denoise_on:  # a suppressed key goes in as the zeros it became
            self.dn.tick(pcm, heard, lists)
        if self.level_on:  # directly behind the suppressor
            self.lv.tick(pcm, heard, lists)
        if self.gate_on:  # directly behind the leveller
            self.gt.tick(pcm, heard, lists)
        self.levels += [int(np.abs(pcm[g, k, :160].astype(np.int64)).sum()) for g, k in np.argwhere(heard == 320)]
        mute = self.host_mute
        if self.max_speakers > 0:
            _, mute = self.spk.step_legs(self.layout, pcm, heard, 320, self.max_speakers, self.floor, self.decay_shift, self.host_mute)
        if self.seq_on and self.conceal_on:  # the history is the audio the stages left, and is not fed to them again
            rows, rlens = self.plc.tick(pcm, heard, self.lists)
            load = np.zeros((self.n, rows.shape[1], 161), np.int16)  # the oracle's look-ahead element
            load[:, :, :160] = rows
        elif self.seq_on:
            load, rlens = repaired_rows(pcm, self.lists)
        else:
            load, rlens = pcm, lens
        self.load_mute = None if mute is None else np.array(mute, np.uint8)
        out = self.rp.tick(load, rlens, self.layout, mute)
        self.gate_seen.append(self.export_gate())
        return out

    # ---- what the handle exports
    def export_legs(self):
        head, tick = self.rp.orc.cursors()
        return {"head": head, "tick": tick, "dropped": self.rp.orc.dropped.copy(), "env": self.spk.env.copy(), "speaking": self.spk.speaking.copy()}

    def export_sequence(self):
        return self.seq.export()

    def export_conceal(self):
        return self.plc.export()["concealed"]

    def export_gate(self):
        if self.gt is None:
            return {"reduce": np.full(self.n, 4, np.uint8), "voiced": np.zeros(self.n, np.uint32), "unvoiced": np.zeros(self.n, np.uint32)}
        return self.gt.export()

    def export_codecs(self):
        return {"in_codec": np.array(self.rp.in_codec, np.uint8), "out_law": np.array(self.rp.out_law, np.uint8), "refused": self.rp.refused.copy()}


def replay_story(lib, n_legs, max_packets, pk, recv, setup=None, before=None, watch=None):
    """the composed replay over a script: setup(model) in front of the first tick, before[t](model) in front of tick t -- the hooks
    run() of tests/conf_harness.py gives the handle -- and watch(t, model, pk[t], recv[t]) behind it.
    -> (datagrams [ticks, n_legs, 172], export_legs() after every tick, the model)"""
    m = ConfReplay(lib, n_legs, max_packets)
    if setup:
        setup(m)
    out, legs = np.zeros((recv.shape[0], n_legs, 172), np.uint8), []
    for t in range(recv.shape[0]):
        if before and t in before:
            before[t](m)
        out[t] = m.tick(pk[t], recv[t])
        legs.append(m.export_legs())
        if watch:
            watch(t, m, pk[t], recv[t])
    return out, legs, m
