"""What the models of the bridge's per-leg stages share (tests/leg_denoise_model.py, leg_level_model.py, leg_gate_model.py), written from
the text in include/wmix_amd.h: which rows of a leg a stage is fed this tick and in which order, and the tick of a model that keeps a
leg's ordered rows and runs the oracle over the whole history.  The rows a leg's load will consume -- without a list the slots with
len == 320 in slot order, with one the list's data calls that name such a slot, in list order; a silence call feeds nothing.  The
outputs of a prefix do not depend on what follows, so running the oracle again from the start each tick is the stream a persistent
stage produces.  Nothing of wmix_amd is imported or read."""
import numpy as np

ROW = 160


def rows_taken(lens, calls=None):
    """the slots of one leg whose rows are fed this tick, in feeding order.  lens [K]; calls None or [("D", slot) / ("S", None)]"""
    n_slots = len(lens)
    if calls is None:
        return [k for k in range(n_slots) if int(lens[k]) == 320]
    return [slot for kind, slot in calls[:4] if kind == "D" and slot < n_slots and int(lens[slot]) == 320]


def legs_fed(lens, lists=None):
    """lens [n, K], lists: None or per leg the call list -> per leg the slots fed, in feeding order"""
    fed = [rows_taken(lens[g], None if lists is None else lists[g]) for g in range(len(lens))]
    assert all(len(set(f)) == len(f) for f in fed), "a call list names a slot twice"
    return fed


class LegsHistoryModel:
    """n legs, per leg the ordered rows fed so far; a subclass says what the oracle makes of leg g's history: run(g) -> [rows, 160]"""

    def __init__(self, lib, n):
        self.lib, self.history = lib, [[] for _ in range(n)]

    def reset(self, legs=None):
        for g in (range(len(self.history)) if legs is None else legs):
            self.history[g] = []

    def tick(self, pcm, lens, lists=None):
        """pcm int16 [n, K, >= 160] (rewritten in place), lens [n, K], lists: None or per leg the call list -> per leg the slots fed"""
        fed = legs_fed(lens, lists)
        for g, slots in enumerate(fed):
            if slots:
                self.history[g] += [np.array(pcm[g][slot][:ROW], np.int16) for slot in slots]
                for slot, row in zip(slots, self.run(g)[-len(slots):]):
                    pcm[g][slot][:ROW] = row
        return fed
