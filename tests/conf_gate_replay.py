"""The composed replay of the conference handle with the voice-activity gate (wmx_conf_gate): ConfReplay of tests/conf_replay_model.py
with tests/leg_gate_model.py where include/wmix_amd.h places the stage -- directly behind the leveller and in front of the selection,
concealment and the load, which all see the gated rows; DTMF is judged on the row as it arrived.  The gate's model is made by the
first gate(True), as the handle makes its VAD; off, it is not ticked; reset_legs gives the listed legs a fresh one (reduce 4, counts 0)
once it has been made.  The stories of tests/test_conf_gate_gpu.py are built here, from the setters wmix_amd/conf.py and this class
share, and expected() keeps a story's replay for the modes that run it, in the shape tests/conf_harness.py's handle_equals_replay
takes.  Nothing of wmix_amd is imported or read."""
import numpy as np

from conf_inputs import G, LAYOUT, SEED, T, arrivals, seq_raw_of
from conf_replay_model import ConfReplay
from conf_stories import everything
from leg_gate_model import LegsGateModel
from leg_seq_model import repaired_rows


class ConfGateReplay(ConfReplay):
    def __init__(self, lib, n_legs, max_packets=3):
        super().__init__(lib, n_legs, max_packets)
        self.gt, self.gate_on = None, False
        self.gate_seen = []  # export_gate() behind every tick

    def gate(self, on):
        if on and self.gt is None:
            self.gt = LegsGateModel(self.lib, self.n)
        self.gate_on = bool(on)

    def reset_legs(self, legs=None):
        super().reset_legs(legs)
        if self.gt is not None:
            self.gt.reset(list(range(self.n) if legs is None else legs))

    def export_gate(self):
        if self.gt is None:
            return {"reduce": np.full(self.n, 4, np.uint8), "voiced": np.zeros(self.n, np.uint32), "unvoiced": np.zeros(self.n, np.uint32)}
        return self.gt.export()

    def tick(self, pk_t, recv_t):
        """ConfReplay.tick with one more stage per leg behind the leveller"""
        assert recv_t.shape == (self.n, self.K) and self.layout
        pcm, lens = self.rp.decode(pk_t, recv_t, self.K)
        heard = lens
        if self.seq_on:
            _, heard, self.lists = self.seq.tick(seq_raw_of(pk_t, recv_t), lens, self.max_gap)
        lists = self.lists if self.seq_on else None
        if self.dtmf_on:  # on the row as it arrived
            self.keys.tick(pk_t, recv_t, pcm, heard, lists, self.dtmf_pt, self.dtmf_suppress)
        if self.denoise_on:
            self.dn.tick(pcm, heard, lists)
        if self.level_on:
            self.lv.tick(pcm, heard, lists)
        if self.gate_on:  # directly behind the leveller
            self.gt.tick(pcm, heard, lists)
        self.levels += [int(np.abs(pcm[g, k, :160].astype(np.int64)).sum()) for g, k in np.argwhere(heard == 320)]
        mute = self.host_mute
        if self.max_speakers > 0:
            _, mute = self.spk.step_legs(self.layout, pcm, heard, 320, self.max_speakers, self.floor, self.decay_shift, self.host_mute)
        if self.seq_on and self.conceal_on:
            rows, rlens = self.plc.tick(pcm, heard, self.lists)
            load = np.zeros((self.n, rows.shape[1], 161), np.int16)
            load[:, :, :160] = rows
        elif self.seq_on:
            load, rlens = repaired_rows(pcm, self.lists)
        else:
            load, rlens = pcm, lens
        self.load_mute = None if mute is None else np.array(mute, np.uint8)
        out = self.rp.tick(load, rlens, self.layout, mute)
        self.gate_seen.append(self.export_gate())
        return out


def replay_story(lib, n_legs, max_packets, pk, recv, setup=None, before=None):
    """replay_story of tests/conf_replay_model.py on the replay with the gate -> (datagrams, export_legs() after every tick, the model)"""
    m = ConfGateReplay(lib, n_legs, max_packets)
    if setup:
        setup(m)
    out, legs = np.zeros((recv.shape[0], n_legs, 172), np.uint8), []
    for t in range(recv.shape[0]):
        if before and t in before:
            before[t](m)
        out[t] = m.tick(pk[t], recv[t])
        legs.append(m.export_legs())
    return out, legs, m


REPLAYED = {}


def expected(key, lib, n, max_packets, story):
    """conf_harness.expected on the replay with the gate: story() -> (pk, recv, setup, before)"""
    if key not in REPLAYED:
        pk, recv, setup, before = story()
        want, legs, m = replay_story(lib, n, max_packets, pk, recv, setup, before)
        REPLAYED[key] = {"pk": pk, "recv": recv, "setup": setup, "before": before, "want": want, "legs": legs, "model": m}
    return REPLAYED[key]


# ---- the stories
def plain_setup(c):
    c.set_conferences(LAYOUT)


def gate_alone():
    """the family's script with the gate on from the first tick"""
    def setup(c):
        c.set_conferences(LAYOUT)
        c.gate(True)

    return arrivals(SEED, T, G) + (setup, None)


def every_stage(lib, gate=True):
    """conf_stories.everything -- codecs, sequence, conceal, speakers, mutes, dtmf with suppress, denoise, level, on the impaired script,
    with its floor -- and the gate behind them (gate False: the same story, floor included, without it)"""
    pk, recv, setup0, before = everything(lib, True, True)

    def setup(c):
        setup0(c)
        if gate:
            c.gate(True)

    return pk, recv, setup, before


ON_AT, RESET_ON_AT, RESET_ON_LEG, OFF_AT, RESET_OFF_AT, RESET_OFF_LEG, ON_AGAIN_AT = 8, 16, 1, 22, 26, 6, 30


def switched():
    """on at tick 8; leg 1 a new call at 16 while the gate is on; off at 22; leg 6 reset at 26 while it is off; on again at 30"""
    before = {ON_AT: lambda c: c.gate(True), RESET_ON_AT: lambda c: c.reset_legs([RESET_ON_LEG]), OFF_AT: lambda c: c.gate(False),
              RESET_OFF_AT: lambda c: c.reset_legs([RESET_OFF_LEG]), ON_AGAIN_AT: lambda c: c.gate(True)}
    return arrivals(SEED, T, G) + (plain_setup, before)
