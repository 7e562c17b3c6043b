"""The talker-selection rule over leg packets (wmix_amd/csrc/speakers.h: speakers_level_legs / speakers_step_legs) as a numpy model: the
model of tests/speakers_model.py, wrapped, with one change -- a leg's level is the largest level among its slots that are calls
(lens[r, k] == src_bytes), and 0 when it has none.  No test in here: tests/test_speakers_legs_host.py compares the header with it,
tests/test_speakers_legs_gpu.py and tests/test_conf_gpu.py the device."""
import numpy as np

from speakers_model import SpeakersModel, level_of


def levels_of_legs(rows, lens, src_bytes, slots=None):
    """rows [n, K, >= src_bytes / 2] int16, lens [n, K] -> one level per ring.  `slots`: look at these slots only (slots=[0] is the rule
    the row-per-leg form applies to a leg's first row)."""
    rows, lens = np.asarray(rows), np.asarray(lens)
    n, K = lens.shape
    levels = np.zeros(n, np.uint64)
    for r in range(n):
        for k in (range(K) if slots is None else slots):
            if int(lens[r, k]) == src_bytes:
                levels[r] = max(int(levels[r]), level_of(rows[r, k, :src_bytes // 2]))
    return levels


class SpeakersLegsModel(SpeakersModel):
    def step_legs(self, layout, rows, lens, src_bytes, max_speakers, floor, decay_shift, mute=None, slots=None):
        """Returns (speaking, mute_out), by ring."""
        return self.step_levels(layout, levels_of_legs(rows, lens, src_bytes, slots), max_speakers, floor, decay_shift, mute)
