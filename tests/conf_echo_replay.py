"""The conference handle with echo control (wmx_conf_echo, include/wmix_amd.h): ConfReplay of tests/conf_replay_model.py with the one
stage it lacks.  The tick is restated with one line between the denoiser and the leveller -- tests/leg_echo_model.py over the rows the
load will consume, the heartbeat's order NS -> AEC -> AGC -> VAD -- and the far step behind the egress: what the tick sent to each leg,
its 160 codes decoded by the oracle with the law they were encoded in, is that leg's far row.  State moves only while the stage is on;
the model is made by the first echo(True, ...), as the handle makes its canceller, and before that export_echo() says what the handle
says: 1, 0, 0, -2.  Nothing of wmix_amd is imported or read."""
import numpy as np

from conf_inputs import seq_raw_of
from conf_replay_model import ConfReplay
from leg_codec_model import LAW_A, Decoders
from leg_echo_model import LegsEchoModel
from leg_seq_model import repaired_rows

ECHO_FIELDS = ("startup", "far_ms", "known_delay", "delay_blocks")


class ConfEchoReplay(ConfReplay):
    def __init__(self, lib, n_legs, max_packets=3):
        super().__init__(lib, n_legs, max_packets)
        self.ec, self.echo_on, self.echo_seen, self.dec = None, False, [], Decoders(lib)
        self.far_rows = []  # what every tick sent to every leg, decoded: [n_legs, 160] per tick

    # ---- the setters of wmix_amd/conf.py
    def echo(self, on, delay_ms=20):
        if on:
            assert 0 <= delay_ms <= 500
            if self.ec is None:
                self.ec = LegsEchoModel(self.lib, self.n, delay_ms)
            for leg in self.ec.legs:
                leg.delay_ms = delay_ms
        self.echo_on = bool(on)

    def set_leg_echo_delay(self, legs, delay_ms):
        for g in legs:
            self.ec.legs[g].delay_ms = delay_ms

    def reset_legs(self, legs=None):
        super().reset_legs(legs)
        if self.ec is not None:
            self.ec.reset(list(range(self.n) if legs is None else legs))

    def sent(self, out):
        """datagrams [n_legs, 172] -> what each leg's speaker plays [n_legs, 160]"""
        return np.stack([self.dec("a" if self.rp.out_law[g] == LAW_A else "u", out[g, 12:172]) for g in range(self.n)])

    # ---- one tick: ConfReplay.tick with the echo stage's two steps
    def tick(self, pk_t, recv_t):
        assert recv_t.shape == (self.n, self.K) and self.layout
        pcm, lens = self.rp.decode(pk_t, recv_t, self.K)
        heard = lens
        if self.seq_on:
            _, heard, self.lists = self.seq.tick(seq_raw_of(pk_t, recv_t), lens, self.max_gap)
        lists = self.lists if self.seq_on else None
        if self.dtmf_on:
            self.keys.tick(pk_t, recv_t, pcm, heard, lists, self.dtmf_pt, self.dtmf_suppress)
        if self.denoise_on:
            self.dn.tick(pcm, heard, lists)
        if self.echo_on:  # behind the suppressor, in front of the leveller: the rows only
            self.ec.tick(pcm, heard, lists)
        if self.level_on:
            self.lv.tick(pcm, heard, lists)
        if self.gate_on:
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
        far = self.sent(out)
        self.far_rows.append(far)
        if self.echo_on:  # behind the egress: the far row only
            self.ec.far(far)
        self.gate_seen.append(self.export_gate())
        self.echo_seen.append(self.export_echo())
        return out

    def export_echo(self):
        if self.ec is None:
            fresh = {"startup": 1, "far_ms": 0, "known_delay": 0, "delay_blocks": -2}
            return {name: np.full(self.n, fresh[name], np.int32) for name in ECHO_FIELDS}
        return dict(zip(ECHO_FIELDS, self.ec.export()))


def replay_echo_story(lib, n_legs, max_packets, pk, recv, setup=None, before=None):
    """replay_story of tests/conf_replay_model.py on ConfEchoReplay -> (datagrams [ticks, n_legs, 172], export_legs() after every tick,
    the model)"""
    m = ConfEchoReplay(lib, n_legs, max_packets)
    if setup:
        setup(m)
    out, legs = np.zeros((recv.shape[0], n_legs, 172), np.uint8), []
    for t in range(recv.shape[0]):
        if before and t in before:
            before[t](m)
        out[t] = m.tick(pk[t], recv[t])
        legs.append(m.export_legs())
    return out, legs, m
