"""The reference daemon's side of a bridge of legs, made of the oracle's own functions: n reference rings (OracleRings), one cursor per
source leg over them (LegsOracle), and on top of those the conference of RTP legs one tick at a time -- the oracle's ingest, the load,
the drain, the oracle's egress with one sender per leg (Replay), and the same with a codec per leg (CodecReplay over
tests/leg_codec_model.py).  Nothing of wmix_amd is imported or read."""
import ctypes as C

import numpy as np

from conf_inputs import NULL_HEAD, K
from leg_codec_model import LAW_A, REFERENCE, Decoders, ingest
from oracle import loader as L


class OracleRings:
    """n rings of one format, heads at byte `start`"""

    def __init__(self, lib, n, ring_chn, ring_freq, start, rmode):
        L.mix_bind(lib)
        self.lib, self.size = lib, ring_chn * 2 * ring_freq
        self.store = [np.zeros(self.size + 64, np.uint8) for _ in range(n)]
        self.r = [L.MixRing() for _ in range(n)]
        for k in range(n):
            lib.orc_mix_ring_init(C.byref(self.r[k]), self.store[k].ctypes.data_as(C.c_void_p), ring_chn, ring_freq)
            self.r[k].head_off, self.r[k].reduce_mode = start, rmode
        self.play_correct = self.r[0].play_correct

    def load(self, k, row, sbytes, freq, chn, head, tick, rarg):
        """one wmix_load_data call into ring k; row holds the source and its look-ahead frame.  -> (head, tick)"""
        row = np.ascontiguousarray(row)
        t = C.c_uint32(tick)
        h = self.lib.orc_load_data(C.byref(self.r[k]), row.ctypes.data_as(C.c_void_p), sbytes, freq, chn, 16, C.c_uint32(head), rarg, C.byref(t))
        return h, t.value

    def ring(self, k):
        return self.store[k][:self.size].view(np.int16).copy()


class LegsOracle:
    """One reference ring per leg and one cursor per source leg.  `drop_rule`: leave out the calls include/wmix_amd.h names (the end
    cursor more than one ring ahead of the mixer's tick, and that leg's later slots of the tick) and count them; without it every
    call is made and the oracle itself asserts that none laps the play head."""

    def __init__(self, lib, n, ring, rmode, play_correct, drop_rule=False):
        self.rings = OracleRings(lib, n, ring[0], ring[1], 0, rmode)
        self.size, self.pkg = self.rings.size, self.rings.size // 50  # 20 ms of ring
        if play_correct is not None:
            for r in self.rings.r:
                r.play_correct = play_correct
        self.correct = self.rings.r[0].play_correct
        self.cursor = [(NULL_HEAD, 0)] * n
        self.dropped = np.zeros(n, np.uint32)
        self.drop_rule, self.n = drop_rule, n

    @staticmethod
    def samples_of_a_call(lib, ring, sbytes, freq, chn):
        """ring samples one wmix_load_data call of this source format writes: the tick a fresh call on a scratch ring ends with"""
        scratch = OracleRings(lib, 1, ring[0], ring[1], 0, 1)
        end = scratch.load(0, np.zeros(sbytes // 2 + chn, np.int16), sbytes, freq, chn, NULL_HEAD, 0, 1)[1]
        return (end - scratch.play_correct) // 2

    def drain(self):
        """the play thread's 20 ms (src/wmix.c:1347-1366) on every ring -> int16 [n, pkg / 2]"""
        out = np.zeros((self.n, self.pkg // 2), np.int16)
        for k, r in enumerate(self.rings.r):
            ring = self.rings.store[k][:self.size].view(np.int16)
            pos = (r.head_off // 2 + np.arange(self.pkg // 2)) % (self.size // 2)
            out[k] = ring[pos]
            ring[pos] = 0
            r.head_off = (r.head_off + self.pkg) % self.size
            r.tick += self.pkg
        return out

    def reset(self, legs):
        for s in legs:
            self.cursor[s], self.dropped[s] = (NULL_HEAD, 0), 0

    def load(self, layout, src, lens, sbytes, freq, chn, n_out, mute):
        """src [n, K, row], lens [n, K]: one tick.  Ring q <- for every other member s in list order, its valid slots in slot order."""
        zeros = np.zeros(src.shape[2], np.int16)
        for mem in layout:
            if len(mem) < 2:
                continue
            for s in mem:
                calls = [k for k in range(lens.shape[1]) if lens[s, k] == sbytes]
                mix_tick = self.rings.r[s].tick
                if self.drop_rule:  # the rule, restated: where would the call end?
                    made, (h, tk) = [], self.cursor[s]
                    for k in calls:
                        tk = mix_tick + self.correct if h == NULL_HEAD or tk < mix_tick else tk
                        if tk + 2 * n_out - mix_tick > self.size:
                            break
                        made.append(k)
                        h, tk = 0, tk + 2 * n_out
                    self.dropped[s] += len(calls) - len(made)
                    calls = made
                if not calls:
                    continue
                ends = set()
                for q in mem:
                    if q == s:
                        continue
                    h, tk = self.cursor[s]
                    for k in calls:
                        h, tk = self.rings.load(q, zeros if mute is not None and mute[s] else src[s, k], sbytes, freq, chn, h, tk, 1)
                        assert tk - mix_tick <= self.size, "the reference laps the play head: leg %d" % s
                    ends.add((h, tk))
                assert len(ends) == 1
                self.cursor[s] = ends.pop()

    def cursors(self):
        return np.array([c[0] for c in self.cursor], np.uint32), np.array([c[1] for c in self.cursor], np.uint32)


class Replay:
    """the conference of RTP legs one tick at a time: every leg REFERENCE in, A-law out"""

    def __init__(self, lib, n, platform="alsa"):
        self.ing = L._fn(lib, "orc_rtp_ingest", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
        self.eg = L._fn(lib, "orc_rtp_egress", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p])
        self.init = L._fn(lib, "orc_rtp_sender_init", None, [C.c_void_p, C.c_int])
        self.senders = [(C.c_uint8 * 16)() for _ in range(n)]
        for s in self.senders:
            self.init(s, 0)
        self.orc, self.n = LegsOracle(lib, n, (1, 8000), 1, L.PLATFORMS[platform][1]), n

    def decode(self, pk, recv, slots=K):
        pcm, lens = np.zeros((self.n, slots, 161), np.int16), np.zeros((self.n, slots), np.uint32)
        for g in range(self.n):
            for k in range(slots):
                if recv[g, k] > 0:
                    row, dec = np.ascontiguousarray(pk[g, k]), np.zeros(160, np.int16)
                    lens[g, k] = self.ing(row.ctypes.data, dec.ctypes.data, None)
                    pcm[g, k, :160] = dec
        return pcm, lens

    def tick(self, pcm, lens, layout, mute=None):
        self.orc.load(layout, pcm, lens, 320, 8000, 1, 160, mute)
        play, out = self.orc.drain(), np.zeros((self.n, 172), np.uint8)
        for g in range(self.n):
            row = np.ascontiguousarray(play[g])
            assert self.eg(self.senders[g], 1, 8000, row.ctypes.data, 320, 1, 8000, out[g].ctypes.data) == 172
        return out

    def fresh(self, legs):
        """a new call in these legs' slots: the reference ring, the receive thread's cursor and the sender as a new task makes them"""
        self.orc.reset(legs)
        for g in legs:
            self.orc.rings.store[g][:] = 0
            self.init(self.senders[g], 0)


class CodecReplay(Replay):
    """Replay with a codec per leg: the decode is the rule's, a leg's oracle sender is made with its law"""

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
