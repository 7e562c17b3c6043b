"""The conference handle with recording taps (wmx_conf_recorders / _record / _record_stop, include/wmix_amd.h): any composed replay --
ConfReplay of tests/conf_replay_model.py, ConfEchoReplay, with_prompts(...) and with_duck(...) of them -- with the taps of
tests/leg_record_model.py beside it.  with_recording(base) restates no tick: its `rp` makes the legs' load and the prompts' calls as the
base's does, and the taps take the rows that rp's own orc.drain() returns -- what the reference's play thread hands the speaker, and the
oracle's egress encodes -- and for every running tap append oracle.loader.mix_zoom(lib, 1, 8000, play[g], chn, freq): ONE wmix_pcm_zoom
call per package.  So every recorded sample is the reference's wmix_load_data, its drain and its wmix_pcm_zoom.  tap_first = True is
the control: the taps read the ring head behind the legs' load and IN FRONT OF the prompts' calls, the place the handle must NOT tap
at.  Nothing of wmix_amd is imported or read."""
import numpy as np

from conf_replay_model import ConfReplay
from leg_record_model import RecordModel
from oracle.loader import mix_zoom


def with_recording(base=ConfReplay, tap_first=False):
    """-> a class like `base` with the recording setters of wmix_amd/conf.py; after every tick rec_legs[t] is the leg per tap (-1: no
    row), rec_rows[t] the row per tap (None: no row) and rec_seen[t] export_record()"""
    class WithRecording(base):
        def __init__(self, lib, n_legs, max_packets=3):
            super().__init__(lib, n_legs, max_packets)
            self.rec, self.rec_format, self.rec_legs, self.rec_rows, self.rec_seen = None, None, [], [], []
            orc, drain = self.rp.orc, self.rp.orc.drain
            self._peeked = None

            def tapped_drain():
                play = drain()
                self._take(self._peeked if tap_first and self._peeked is not None else play)
                self._peeked = None
                return play

            orc.drain = tapped_drain
            if tap_first and hasattr(self.rp, "play_prompts"):
                prompts = self.rp.play_prompts

                def peek_then_prompts():
                    self._peeked = np.stack([orc.rings.ring(k)[(r.head_off // 2 + np.arange(160)) % (orc.size // 2)]
                                             for k, r in enumerate(orc.rings.r)])
                    prompts()

                self.rp.play_prompts = peek_then_prompts

        def _take(self, play):
            if self.rec is None:  # no store yet: the tick has no rows
                self.rec_legs.append(None), self.rec_rows.append(None), self.rec_seen.append(None)
                return
            legs = self.rec.tick()
            chn, freq = self.rec_format
            self.rec_legs.append(np.array(legs, np.int32))
            self.rec_rows.append([None if g < 0 else mix_zoom(self.lib, 1, 8000, np.ascontiguousarray(play[g]), chn, freq) for g in legs])
            self.rec_seen.append(self.rec.export())

        # ---- the setters of wmix_amd/conf.py
        def recorders(self, max_taps, channels=1, freq=8000):
            assert self.rec is None
            self.rec, self.rec_format = RecordModel(max_taps), (channels, freq)
            self.rec_row_samples = mix_zoom(self.lib, 1, 8000, np.zeros(160, np.int16), channels, freq).size

        def set_play_correct(self, n_bytes):
            """VIEW_PLAY_CORRECT of every leg's daemon, as wmx_conf_set_play_correct sets the handle's: with the platform's 200 ms a
            story of a dozen ticks would record little but the lead's silence"""
            self.rp.orc.correct = n_bytes
            for r in self.rp.orc.rings.r:
                r.play_correct = n_bytes

        def record(self, legs, seconds=0, ticks=None):
            return np.array(self.rec.start(list(legs), int(ticks) if ticks is not None else 50 * int(seconds)), np.int32)

        def record_stop(self, legs=None):
            self.rec.stop(None if legs is None else list(legs))

        def reset_legs(self, legs=None):
            super().reset_legs(legs)
            if self.rec is not None:
                self.rec.reset(list(range(self.n) if legs is None else legs))

        def export_record(self):
            return self.rec.export()

    return WithRecording


def replay_record_story(lib, n_legs, max_packets, pk, recv, setup=None, before=None, base=ConfReplay, tap_first=False):
    """replay_story of tests/conf_replay_model.py on with_recording(base) -> (datagrams [ticks, n_legs, 172], export_legs() after every
    tick, the model)"""
    m = with_recording(base, tap_first)(lib, n_legs, max_packets)
    if setup:
        setup(m)
    out, legs = np.zeros((recv.shape[0], n_legs, 172), np.uint8), []
    for t in range(recv.shape[0]):
        if before and t in before:
            before[t](m)
        out[t] = m.tick(pk[t], recv[t])
        legs.append(m.export_legs())
    return out, legs, m
