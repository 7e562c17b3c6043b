"""The fold the bridge applies to a ducked ring (wmix_amd/csrc/leg_prompt.h, REDUCE; duck_fold_kernel in mix.hip), against the reference
alone: ONE reference ring whose reduce_mode the play task holds at D, the other members' orc_load_data calls with reduce 1 in list
order, then the prompt's with reduce D.  What it must equal is the rule as the header states it, in ten lines of numpy: trunc(c / D)
per term, a saturating add per term in order, the prompt undivided and last.  Nothing of wmix_amd is imported or read.  Integers."""
import numpy as np
import pytest

from conf_inputs import NULL_HEAD
from leg_oracle_model import OracleRings

N, OTHERS, AT = 160, 5, 1600  # a call of 160 samples; a fresh cursor starts play_correct = 3 200 bytes behind the head


def inputs(D):
    """-> (what lies in the ring before, the others' rows [OTHERS, N], the prompt's row): near full scale, odd negative samples, and
    three columns made for the three ways of getting the rule wrong"""
    rng = np.random.default_rng(100 + D)
    before = rng.integers(-9000, 9000, N).astype(np.int16)
    rows = rng.integers(-32768, 32768, (OTHERS, N)).astype(np.int16)
    rows[:, 40:80] = -(np.abs(rows[:, 40:80].astype(np.int32)) | 1).clip(1, 32767).astype(np.int16)  # odd and negative
    prompt = rng.integers(-30000, 30000, N).astype(np.int16)
    before[:3], rows[:, :3], prompt[:3] = 0, 0, 0
    rows[0, 0], rows[1, 0] = 30000, 30000  # saturates undivided, not when ducked: 2 * (30000 / D) <= 30000
    rows[2, 1] = -(D + 1)                  # trunc gives -1, a floor (for D = 2 and 16: an arithmetic shift) gives -2
    rows[0, 2], rows[3, 2] = D - 1, 1      # the terms divide to 0 + 0, their sum to 1
    return before, rows, prompt


def oracle(lib, D, before, rows, prompt):
    """the reference's ring samples AT .. AT + N: `before` loaded while nobody ducks, then the others and the prompt on reduceMode D"""
    rings = OracleRings(lib, 1, 1, 8000, 0, 1)
    look = lambda row: np.concatenate([row, np.zeros(1, np.int16)])  # noqa: E731  the look-ahead frame the call reads past its samples
    rings.load(0, look(before), 2 * N, 8000, 1, NULL_HEAD, 0, 1)
    rings.r[0].reduce_mode = D  # the play task takes the mode (src/wmixTask.c:1416-1423)
    for row in rows:
        rings.load(0, look(row), 2 * N, 8000, 1, NULL_HEAD, 0, 1)  # rdce = (1 == D) ? 1 : D
    rings.load(0, look(prompt), 2 * N, 8000, 1, NULL_HEAD, 0, D)   # rdce = (D == D) ? 1 : D
    ring = rings.ring(0)
    assert not ring[:AT].any() and not ring[AT + N:].any()
    return ring[AT:AT + N].astype(np.int64)


def rule(D, before, rows, prompt):
    x = before.astype(np.int64)
    for c in rows.astype(np.int64):
        x = np.clip(x + np.sign(c) * (np.abs(c) // D), -32768, 32767)  # trunc(c / D), then the saturating add
    return np.clip(x + prompt, -32768, 32767)  # the prompt undivided, last


@pytest.mark.parametrize("D", [2, 3, 16])
def test_the_fold_is_trunc_per_term_saturating_in_order_prompt_undivided(oracle_port, D):
    before, rows, prompt = inputs(D)
    got = oracle(oracle_port, D, before, rows, prompt)
    assert np.array_equal(got, rule(D, before, rows, prompt)), np.flatnonzero(got != rule(D, before, rows, prompt))[:8]
    # what the inputs contain, from the oracle's output alone
    undivided = oracle(oracle_port, 1, before, rows, prompt)
    assert undivided[0] == 32767 and 0 < got[0] < 32767                        # saturates undivided, not when ducked
    assert undivided[1] == -(D + 1) and got[1] == -1 != undivided[1] // D == -2  # truncation toward zero, not a floor or a shift
    assert undivided[2] == D and got[2] == 0 != undivided[2] // D == 1            # the terms are divided, not the finished sum
    assert (got[40:80] != undivided[40:80]).any()
    # the prompt is undivided: the same others without it differ from the ring by the prompt itself wherever nothing saturates
    silent = oracle(oracle_port, D, before, rows, np.zeros(N, np.int16))
    free = np.abs(silent + prompt) < 32767
    assert free.sum() > 50 and np.array_equal(got[free], (silent + prompt)[free])
    assert (np.abs(prompt[free]) > 2 * D).sum() > 40  # and a divided prompt would not have been the same
