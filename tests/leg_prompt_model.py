"""The prompt rule of one leg of the bridge, written from the text at the head of wmix_amd/csrc/leg_prompt.h: a clip played into the
leg's own ring by a task with a cursor of its own, one wmix_load_data call of at most 160 samples per 20 ms tick.  Python integers held
to uint32 where the reference's are; numpy only for the clips and the exports.  Nothing of wmix_amd is imported or read."""
import numpy as np

NULL_HEAD, U32, ROW, MAX_GAP = 0xFFFFFFFF, 0xFFFFFFFF, 160, 65535


def cursor_begin(mix, head, tick):
    """mix = (head_off, tick, play_correct, ring_bytes) of the leg's ring; where a call handed (head, tick) starts: a task without a
    cursor, or one that fell behind the play head, jumps to head + VIEW_PLAY_CORRECT, or to the ring's start when that lies behind its
    end (src/wmix.c:1666-1673)"""
    head_off, mix_tick, correct, size = mix
    if head == NULL_HEAD or tick < mix_tick:
        head, tick = (head_off + correct) & U32, (mix_tick + correct) & U32
        if head >= size:
            head = 0
    return head, tick


def cursor_end(mix, n, head, tick):
    """the cursor a call of n ring samples that started at (head, tick) ends with (src/wmix.c:1942-1956)"""
    head_off, mix_tick, _, size = mix
    add = 2 * n
    new_head = ((head + add) & U32) % size
    if tick < mix_tick:
        new_head = (head_off + add) & U32
        add = (add + mix_tick) & U32
        if new_head >= size:
            new_head -= size
    else:
        add = (add + tick) & U32
    return new_head, add


class LegPrompt:
    FIELDS = ("clip", "pos", "left", "done", "wait", "gap", "head", "tick")

    def __init__(self):
        self.done = 0
        self.stop()

    def state(self):
        return tuple(getattr(self, f) for f in self.FIELDS)

    def play(self, clip, repeat, gap):
        """a new task: a fresh cursor; done stays"""
        assert clip >= 0 and repeat >= 0 and 0 <= gap <= MAX_GAP
        self.clip, self.pos, self.left, self.wait, self.gap, self.head, self.tick = clip, 0, repeat, 0, gap, NULL_HEAD, 0

    def stop(self):
        self.clip, self.pos, self.left, self.wait, self.gap, self.head, self.tick = -1, 0, 0, 0, 0, NULL_HEAD, 0

    def reset(self):
        self.stop()
        self.done = 0

    def step(self, mix, samples):
        """one tick -> None (no call), or (n, the clip sample the call starts at, the cursor (head, tick) it is handed, the byte offset
        in the ring of its first sample, the cursor it ends with); that cursor is kept inside a pass, and is fresh again behind one"""
        if self.clip < 0:
            return None
        if self.pos >= samples:  # a state the clip table does not bear out
            self.stop()
            return None
        if self.wait > 0:
            self.wait -= 1
            return None
        n, at, handed = min(ROW, samples - self.pos), self.pos, (self.head, self.tick)
        head, tick = cursor_begin(mix, self.head, self.tick)
        start = head
        self.head, self.tick = ended = cursor_end(mix, n, head, tick)
        self.pos += n
        if self.pos == samples:
            if self.left == 1:
                self.stop()
                self.done = (self.done + 1) & U32
            else:
                if self.left:
                    self.left -= 1
                # the next pass starts over with a fresh cursor, as the reference resets head and tick behind its sleep
                self.pos, self.wait, self.head, self.tick = 0, self.gap, NULL_HEAD, 0
        return n, at, handed, start, ended


class LegsPromptModel:
    """the store and one LegPrompt per leg, with the setters of wmix_amd/conf.py"""

    def __init__(self, n_legs):
        self.n, self.legs, self.clips, self.cap = n_legs, [LegPrompt() for _ in range(n_legs)], [], None

    def prompts(self, max_clips, max_samples):
        assert self.cap is None and max_clips >= 1 and max_samples >= 1
        self.cap = (max_clips, max_samples)

    def add_clip(self, pcm):
        pcm = np.array(pcm, np.int16).reshape(-1)
        assert self.cap is not None and pcm.size >= 1 and len(self.clips) < self.cap[0]
        assert sum(c.size for c in self.clips) + pcm.size <= self.cap[1]
        self.clips.append(pcm)
        return len(self.clips) - 1

    def _legs(self, legs):
        legs = list(range(self.n) if legs is None else legs)
        assert all(0 <= g < self.n for g in legs)
        return legs

    def play(self, legs, clip, repeat=1, gap_ticks=0):
        assert self.cap is not None and 0 <= clip < len(self.clips)
        for g in self._legs(legs):
            self.legs[g].play(clip, repeat, gap_ticks)

    def stop(self, legs=None):
        assert self.cap is not None
        for g in self._legs(legs):
            self.legs[g].stop()

    def reset(self, legs):
        for g in self._legs(legs):
            self.legs[g].reset()

    def step(self, g, mix):
        """-> None, or (the call's samples with the look-ahead element the oracle's call reads past them, the cursor it is handed,
        the cursor the rule says it ends with)"""
        leg = self.legs[g]
        if leg.clip < 0:
            return None
        clip = self.clips[leg.clip]
        call = leg.step(mix, clip.size)
        if call is None:
            return None
        n, at, handed, _, ended = call
        row = np.zeros(n + 1, np.int16)
        row[:n] = clip[at:at + n]
        return row, handed, ended

    def export(self):
        return {"clip": np.array([p.clip for p in self.legs], np.int32), "pos": np.array([p.pos for p in self.legs], np.uint32),
                "left": np.array([p.left for p in self.legs], np.uint32), "done": np.array([p.done for p in self.legs], np.uint32)}
