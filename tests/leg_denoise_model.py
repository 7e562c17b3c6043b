"""A model of the bridge's per-leg noise suppression (wmx_nsx_process_legs), written from the text in include/wmix_amd.h: per leg the
ordered rows fed so far; per tick the leg's PCM rows, lens and, with sequencing, the call list.  The rows a leg's load will consume
(rows_taken of tests/leg_rows_model.py, whose history-based tick this model shares) are appended to the leg's history and the oracle's fixed-point suppressor (oracle/orc_nsx.c, 1 x 8000) is run
over the whole history from a fresh state: the last rows of its output are the tick's cleaned rows.  The outputs of a prefix do not
depend on what follows, so running again from the start each tick is the stream a persistent suppressor produces.  Nothing of wmix_amd
is imported or read."""
import numpy as np

from leg_rows_model import ROW, LegsHistoryModel
from oracle import loader as L


def suppress(lib, rows):
    """rows int16 [n, 160], one leg's whole ordered history -> the suppressor's output for it, [n, 160]"""
    rows = np.ascontiguousarray(rows, np.int16).reshape(-1, ROW)
    if not len(rows):
        return rows.copy()
    return L.run_nsx(lib, 1, 8000, rows.reshape(-1), 80, prefix="orc").reshape(-1, ROW)


class LegsDenoiseModel(LegsHistoryModel):
    """n legs; tick() takes what the ingest, the sequencer and the DTMF stage left and leaves what the kernel leaves"""

    def run(self, g):
        return suppress(self.lib, self.history[g])
