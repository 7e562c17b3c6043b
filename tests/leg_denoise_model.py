"""A model of the bridge's per-leg noise suppression (wmx_nsx_process_legs), written from the text in include/wmix_amd.h: per leg the
ordered rows fed so far; per tick the leg's PCM rows, lens and, with sequencing, the call list.  The rows a leg's load will consume --
without a list the slots with len == 320 in slot order, with one the list's data calls that name such a slot, in list order; a silence
call feeds nothing -- are appended to the leg's history and the oracle's fixed-point suppressor (oracle/orc_nsx.c, 1 x 8000) is run
over the whole history from a fresh state: the last rows of its output are the tick's cleaned rows.  The outputs of a prefix do not
depend on what follows, so running again from the start each tick is the stream a persistent suppressor produces.  Nothing of wmix_amd
is imported or read."""
import numpy as np

from oracle import loader as L

ROW = 160


def rows_taken(lens, calls=None):
    """the slots of one leg whose rows are fed this tick, in feeding order.  lens [K]; calls None or [("D", slot) / ("S", None)]"""
    n_slots = len(lens)
    if calls is None:
        return [k for k in range(n_slots) if int(lens[k]) == 320]
    return [slot for kind, slot in calls[:4] if kind == "D" and slot < n_slots and int(lens[slot]) == 320]


def suppress(lib, rows):
    """rows int16 [n, 160], one leg's whole ordered history -> the suppressor's output for it, [n, 160]"""
    rows = np.ascontiguousarray(rows, np.int16).reshape(-1, ROW)
    if not len(rows):
        return rows.copy()
    return L.run_nsx(lib, 1, 8000, rows.reshape(-1), 80, prefix="orc").reshape(-1, ROW)


class LegsDenoiseModel:
    """n legs; tick() takes what the ingest, the sequencer and the DTMF stage left and leaves what the kernel leaves"""

    def __init__(self, lib, n):
        self.lib, self.history = lib, [[] for _ in range(n)]

    def reset(self, legs=None):
        for g in (range(len(self.history)) if legs is None else legs):
            self.history[g] = []

    def tick(self, pcm, lens, lists=None):
        """pcm int16 [n, K, >= 160] (rewritten in place), lens [n, K], lists: None or per leg the call list -> per leg the slots fed"""
        fed = []
        for g, history in enumerate(self.history):
            fed.append(rows_taken(lens[g], None if lists is None else lists[g]))
            assert len(set(fed[g])) == len(fed[g]), "a call list names a slot twice"
            if fed[g]:
                history += [np.array(pcm[g][slot][:ROW], np.int16) for slot in fed[g]]
                clean = suppress(self.lib, history)[-len(fed[g]):]
                for slot, row in zip(fed[g], clean):
                    pcm[g][slot][:ROW] = row
        return fed
