"""The duck of one leg of the bridge, written from the REDUCE paragraph at the head of wmix_amd/csrc/leg_prompt.h over the prompt rule of
tests/leg_prompt_model.py: a play carries the reference's `reduce` (0 .. 15), and in a tick in which the leg's prompt makes a call
everything the other legs load into the leg's ring is divided by reduce + 1.  Python integers.  Nothing of wmix_amd is imported or
read."""
from leg_prompt_model import LegPrompt, LegsPromptModel

MAX_REDUCE = 15


class DuckPrompt(LegPrompt):
    """LegPrompt with the divisor of its play; `reduce` is no part of state(), which stays the plain model's"""

    def __init__(self):
        self.reduce = 0
        super().__init__()

    def play(self, clip, repeat, gap, reduce=0):
        assert 0 <= reduce <= MAX_REDUCE
        super().play(clip, repeat, gap)
        self.reduce = reduce  # a play over a playing leg replaces the divisor as it replaces everything else

    def stop(self):
        super().stop()
        self.reduce = 0  # stop, reset and the end of the last pass release the duck

    def ducks(self, samples):
        """the divisor this tick's load of the legs applies, on the state as the tick finds it (in front of step()); 1: none.  The leg
        is ducked exactly when its prompt makes a call in this tick and was started with reduce > 0"""
        calls = self.clip >= 0 and self.wait == 0 and self.pos < samples
        return self.reduce + 1 if calls else 1


class LegsDuckModel(LegsPromptModel):
    def __init__(self, n_legs):
        super().__init__(n_legs)
        self.legs = [DuckPrompt() for _ in range(n_legs)]

    def play(self, legs, clip, repeat=1, gap_ticks=0, reduce=0):
        assert self.cap is not None and 0 <= clip < len(self.clips)
        for g in self._legs(legs):
            self.legs[g].play(clip, repeat, gap_ticks, reduce)

    def ducks(self, g):
        leg = self.legs[g]
        return leg.ducks(self.clips[leg.clip].size) if leg.clip >= 0 else 1

    def export_duck(self):
        import numpy as np
        return np.array([self.ducks(g) for g in range(self.n)], np.uint8)
