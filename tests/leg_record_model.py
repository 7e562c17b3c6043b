"""The recording taps of the bridge (wmx_rtp_record_rings / wmx_conf_record), written from the TEXT of wmix_amd/csrc/leg_record.h:

A store has max_taps taps.  Per tap: leg (-1: free), left (the ticks still to record, 0: until stopped), written (the rows written
since the tap was started).
  start(legs, ticks)  a leg that has a tap is restarted in place, the others take the lowest free taps: leg, left = ticks, written = 0.
                      All or nothing: with fewer free taps than legs that need one, nothing starts.
  stop(legs)          those legs' taps (None: every tap) are free: leg = -1, left = 0; written stays.
  reset(legs)         a stop with written = 0.
  tick                a free tap: nothing.  A running tap writes one row of its leg and written++; left == 1: free behind that row;
                      left > 1: left--; left == 0 stays.
Nothing of wmix_amd is imported or read."""
import numpy as np


class Refused(Exception):
    """fewer free taps than legs that need one: nothing started"""


class RecordModel:
    def __init__(self, max_taps):
        self.leg, self.left, self.written = [-1] * max_taps, [0] * max_taps, [0] * max_taps

    def start(self, legs, ticks=0):
        taps, free = [], [k for k, g in enumerate(self.leg) if g < 0]
        for i, g in enumerate(legs):
            if g in self.leg:
                taps.append(self.leg.index(g))
            elif g in legs[:i]:
                taps.append(taps[legs.index(g)])
            elif free:
                taps.append(free.pop(0))
            else:
                raise Refused(legs)
        for g, k in zip(legs, taps):
            self.leg[k], self.left[k], self.written[k] = g, ticks, 0
        return taps

    def _end(self, legs, keep_written):
        for k, g in enumerate(self.leg):
            if legs is None or (g >= 0 and g in legs):
                self.leg[k], self.left[k] = -1, 0
                if not keep_written:
                    self.written[k] = 0

    def stop(self, legs=None):
        self._end(legs, True)

    def reset(self, legs=None):
        self._end(legs, False)

    def running(self):
        return any(g >= 0 for g in self.leg)

    def tick(self):
        """-> per tap the leg whose row this tick writes, -1 for none"""
        rows = list(self.leg)
        for k, g in enumerate(self.leg):
            if g < 0:
                continue
            self.written[k] += 1
            if self.left[k] == 1:
                self.leg[k], self.left[k] = -1, 0
            elif self.left[k]:
                self.left[k] -= 1
        return rows

    def export(self):
        return {"leg": np.array(self.leg, np.int32), "left": np.array(self.left, np.uint32), "written": np.array(self.written, np.uint32)}
