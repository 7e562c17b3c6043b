"""A model of the bridge's per-leg gain control (wmx_agc_process_legs), written from the text in include/wmix_amd.h: per leg the ordered
rows fed so far and the leg's compression gain; per tick the leg's PCM rows, lens and, with sequencing, the call list.  The rows a
leg's load will consume (rows_taken of tests/leg_rows_model.py, whose history-based tick this model shares) are appended to the
leg's history and the oracle's AGC (oracle/orc_agc.c, 1 x 8000, 80 frames a call: two calls a row) is run over the whole history from a fresh handle: the last rows of its output are the tick's
levelled rows.  The outputs of a prefix do not depend on what follows, so running again from the start each tick is the stream a
persistent AGC produces.  A leg's gain that changed on the way (agc_addition) is replayed in front of the call it was in force from.
Nothing of wmix_amd is imported or read."""
import numpy as np

from leg_rows_model import ROW, LegsHistoryModel
from oracle import loader as L

CALLS_PER_ROW = 2  # the AGC's packet at 8 kHz is 80 samples


def level(lib, rows, value, additions=None):
    """rows int16 [n, 160], one leg's whole ordered history -> the AGC's output for it, [n, 160].  value: the gain the handle is made
    with; additions: {row index: value}, agc_addition in front of that row"""
    rows = np.ascontiguousarray(rows, np.int16).reshape(-1, ROW)
    if not len(rows):
        return rows.copy()
    if not additions:
        return L.run_agc(lib, 1, 8000, int(value), rows.reshape(-1), 80, prefix="orc").reshape(-1, ROW)
    add = {CALLS_PER_ROW * int(r): int(v) for r, v in additions.items()}
    return L.run_agc_handle(lib, 1, 8000, int(value), rows.reshape(-1), 80, additions=add, prefix="orc").reshape(-1, ROW)


class LegsLevelModel(LegsHistoryModel):
    """n legs; tick() takes what the ingest, the sequencer, the DTMF stage and the denoiser left and leaves what the kernel leaves"""

    def __init__(self, lib, n, value):
        super().__init__(lib, n)
        self.first = [int(value)] * n                # the gain the leg's handle was made with (agc_init)
        self.gain = [int(value)] * n                 # the gain in force
        self.additions = [{} for _ in range(n)]      # {rows fed before it: value}

    def set_gain(self, value, legs=None):
        """agc_addition for the listed legs (None = every leg): the state stays, the curve changes from the next row on"""
        for g in (range(len(self.history)) if legs is None else legs):
            self.gain[g] = int(value)
            self.additions[g][len(self.history[g])] = int(value)

    def reset(self, legs=None):
        """agc_release + agc_init with the gain the leg has"""
        for g in (range(len(self.history)) if legs is None else legs):
            self.history[g], self.additions[g], self.first[g] = [], {}, self.gain[g]

    def run(self, g):
        return level(self.lib, self.history[g], self.first[g], self.additions[g])
