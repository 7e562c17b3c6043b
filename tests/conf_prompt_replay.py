"""The conference handle with prompts (wmx_conf_prompts / _add_clip / _play / _stop, include/wmix_amd.h): the composed replay of
tests/conf_replay_model.py, or of tests/conf_echo_replay.py, with another `rp`.  PromptReplay is CodecReplay of
tests/leg_oracle_model.py whose tick makes the legs' load, THEN the prompts' calls -- one orc_load_data per playing leg into that leg's
own reference ring, handed the cursor tests/leg_prompt_model.py keeps for it (for the first call of a pass the cursor the reference's
play task holds there: the ring's head and tick 0) -- then the drain and the egress.  The reference stays the
reference: every sample of every ring is the oracle's, and the cursor the oracle's call ends with must be the one the rule's text
gives.  prompt_first = True makes the prompts' calls in front of the legs' instead: the order the handle must NOT have.  Neither tick of
the composed replays is restated: with_prompts() installs the `rp` and adds the setters a story calls on handle and model alike.
Nothing of wmix_amd is imported or read."""
import numpy as np

from conf_replay_model import ConfReplay
from leg_oracle_model import CodecReplay
from leg_prompt_model import NULL_HEAD, LegsPromptModel


class PromptReplay(CodecReplay):
    def __init__(self, lib, n, prompt_first=False):
        super().__init__(lib, n)
        self.pm, self.prompt_first, self.prompt_seen, self.prompt_calls = LegsPromptModel(n), prompt_first, [], 0

    def play_prompts(self):
        for g, r in enumerate(self.orc.rings.r):
            call = self.pm.step(g, (r.head_off, r.tick, r.play_correct, self.orc.size))
            if call is None:
                continue
            row, (head, tick), after = call
            if head == NULL_HEAD and r.tick > 0:
                # a fresh cursor.  What the reference's task holds behind its sleep is not a NULL head but `head = wmix->head, tick = 0`
                # (src/wmixTask.c:1580-1581): hand the oracle exactly that, so that it is the reference that says the two are one
                head, tick = r.head_off, 0
            end = self.orc.rings.load(g, row, 2 * (len(row) - 1), 8000, 1, head, tick, 1)
            assert end == after, ("leg", g, "the oracle's call ends at", end, "the rule's text at", after)
            self.prompt_calls += 1

    def tick(self, pcm, lens, layout, mute=None):
        if self.prompt_first:
            self.play_prompts()
        self.orc.load(layout, pcm, lens, 320, 8000, 1, 160, mute)
        if not self.prompt_first:
            self.play_prompts()
        play, out = self.orc.drain(), np.zeros((self.n, 172), np.uint8)
        for g in range(self.n):
            row = np.ascontiguousarray(play[g])
            assert self.eg(self.senders[g], 1, 8000, row.ctypes.data, 320, 1, 8000, out[g].ctypes.data) == 172
        self.prompt_seen.append(self.pm.export())
        return out

    def fresh(self, legs):
        super().fresh(legs)
        if self.pm.cap is not None:  # only once the store exists
            self.pm.reset(legs)


def with_prompts(base=ConfReplay, prompt_first=False):
    """-> a class like `base` (ConfReplay, ConfEchoReplay) whose rp is a PromptReplay, with the prompt setters of wmix_amd/conf.py"""
    class WithPrompts(base):
        def __init__(self, lib, n_legs, max_packets=3):
            super().__init__(lib, n_legs, max_packets)
            self.rp = PromptReplay(lib, n_legs, prompt_first)  # as created: nothing set on the one it replaces

        def prompts(self, max_clips, max_samples):
            self.rp.pm.prompts(max_clips, max_samples)

        def add_clip(self, pcm, freq=8000, channels=1):
            assert (freq, channels) == (8000, 1)
            return self.rp.pm.add_clip(pcm)

        def play(self, legs, clip, repeat=1, gap_ticks=0):
            self.rp.pm.play(legs, clip, repeat, gap_ticks)

        def stop(self, legs=None):
            self.rp.pm.stop(legs)

        def export_prompts(self):
            return self.rp.pm.export()

    return WithPrompts


def replay_prompt_story(lib, n_legs, max_packets, pk, recv, setup=None, before=None, base=ConfReplay, prompt_first=False):
    """replay_story of tests/conf_replay_model.py on with_prompts(base) -> (datagrams [ticks, n_legs, 172], export_legs() after every
    tick, the model; model.rp.prompt_seen holds export_prompts() after every tick)"""
    m = with_prompts(base, prompt_first)(lib, n_legs, max_packets)
    if setup:
        setup(m)
    out, legs = np.zeros((recv.shape[0], n_legs, 172), np.uint8), []
    for t in range(recv.shape[0]):
        if before and t in before:
            before[t](m)
        out[t] = m.tick(pk[t], recv[t])
        legs.append(m.export_legs())
    return out, legs, m
