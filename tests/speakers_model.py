"""The talker-selection rule of wmix_amd/csrc/speakers.h as a small numpy model (no test in here: tests/test_speakers_host.py compares
the header with it, tests/test_speakers_gpu.py the device).

Per ring r one uint32 env[r], zero at first.  One step with max_speakers, floor, decay_shift, for the member at list position p (ring r)
of a conference of at least 2 members:
    level    = sum |x| over the row's int16 elements (|-32768| = 32768)
    env'     = max(level, env - (env >> decay_shift))                  stored for every member, the host-muted ones too
    eligible = not host_mute[r] and env' >= floor
    rank     = eligible s of the conference with env'[s] > env'[p], or env'[s] == env'[p] and s < p   (list positions)
    speaking = eligible and rank < max_speakers
Every other ring: speaking 0, env untouched.  mute_out = 1 - speaking."""
import numpy as np

M32 = 0xFFFFFFFF


def level_of(row):
    return int(np.abs(np.asarray(row).astype(np.int64)).sum())


class SpeakersModel:
    def __init__(self, n_groups):
        self.env = np.zeros(n_groups, np.uint32)
        self.speaking = np.zeros(n_groups, np.uint8)

    def reset(self, rings=None):
        if rings is None:
            self.env[:] = 0
        else:
            self.env[list(rings)] = 0

    def step_levels(self, layout, levels, max_speakers, floor, decay_shift, mute=None):
        """layout: list of conferences, each the ordered list of its rings; levels: one per ring.  Returns (speaking, mute_out)."""
        assert 1 <= max_speakers <= 32 and 0 <= decay_shift <= 31
        speaking = np.zeros(len(self.env), np.uint8)
        for mem in layout:
            if len(mem) < 2:
                continue
            nxt = []
            for r in mem:
                lv, env = int(levels[r]), int(self.env[r])
                assert 0 <= lv <= M32
                nxt.append(max(lv, (env - (env >> decay_shift)) & M32))
            ok = [not (mute is not None and mute[r]) and e >= floor for r, e in zip(mem, nxt)]
            for p, r in enumerate(mem):
                rank = sum(1 for s in range(len(mem)) if ok[s] and (nxt[s] > nxt[p] or (nxt[s] == nxt[p] and s < p)))
                speaking[r] = 1 if ok[p] and rank < max_speakers else 0
                self.env[r] = nxt[p]
        self.speaking = speaking
        return speaking, (1 - speaking).astype(np.uint8)

    def step(self, layout, rows, max_speakers, floor, decay_shift, mute=None):
        """rows[r]: the int16 source row of ring r (only the members' rows are looked at)"""
        levels = np.zeros(len(self.env), np.uint64)
        for mem in layout:
            if len(mem) >= 2:
                for r in mem:
                    levels[r] = level_of(rows[r])
        return self.step_levels(layout, levels, max_speakers, floor, decay_shift, mute)


def uniform_layout(n_groups, parties):
    return [list(range(c * parties, (c + 1) * parties)) for c in range(n_groups // parties)]


def row_of_level(level, n_elements, rng=None):
    """an int16 row of n_elements whose level is exactly `level` (0 <= level <= 32768 * n_elements), signs mixed"""
    assert 0 <= level <= 32768 * n_elements
    row = np.zeros(n_elements, np.int64)
    base, extra = divmod(level, n_elements)
    row[:] = base
    row[:extra] += 1
    sign = np.where(np.arange(n_elements) % 2 == 0, -1, 1)
    row = np.where(row == 32768, -32768, row * sign)  # 32768 exists only as -32768
    if rng is not None:
        row = row[rng.permutation(n_elements)]
    assert level_of(row) == level
    return row.astype(np.int16)
