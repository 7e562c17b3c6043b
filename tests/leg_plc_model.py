"""A model of the bridge's concealment rule (wmx_rtp_conceal_legs), written from the rule as include/wmix_amd.h states it: per leg the
last 320 samples it emitted and a counter; per tick the leg's rows, lens and call list; out come the emitted rows in call order.
numpy int64 and Python integers; nothing of wmix_amd/csrc/leg_plc.h.  Also the generator of random (history, list, rows) cases that
tests/test_leg_plc_host.py and tests/test_rtp_conceal_gpu.py share."""
import numpy as np

from conf_inputs import alaw_decode, ulaw_decode  # noqa: F401  (tests/test_leg_plc_host.py takes them from here)

HIST, ROW, LAG_MIN, LAG_MAX, BLEND, MAX_CALLS = 320, 160, 40, 120, 32, 4
D, S = (lambda k: ("D", k)), ("S", None)


def best_lag(h0):
    """-> L*: the smallest lag in 40 .. 120 with the largest c(L) = sum over i = 160 .. 319 of q[i] * q[i - L], q = h0 >> 4"""
    q = np.asarray(h0, np.int64) >> 4
    scores = [int((q[160:320] * q[160 - lag:320 - lag]).sum()) for lag in range(LAG_MIN, LAG_MAX + 1)]
    assert max(abs(c) for c in scores) < 2 ** 31
    return LAG_MIN + int(np.argmax(scores))  # argmax: the first of equals


def synthesis(h0, lag, k):
    """samples k (an int64 array) of a run that started from history h0 with lag L*"""
    s = np.asarray(h0, np.int64)[HIST - lag + k % lag]
    g = np.maximum(0, 32768 - 68 * k)
    return (s * g) >> 15


class LegPlc:
    def __init__(self, hist=None):
        self.hist = np.zeros(HIST, np.int64) if hist is None else np.array(hist, np.int64)
        self.concealed = 0
        self.lags = []  # L* of every run, in order: for the tests' known answers

    def tick(self, rows, lens, calls):
        """rows int16 [K, >= 160], lens [K], calls: the list of ("D", slot) / ("S", None) -> (emitted rows int16 [4, 160], of which
        the first len(calls) count; len_out uint32 [4])"""
        n_slots = len(lens)
        out, len_out = np.zeros((MAX_CALLS, ROW), np.int16), np.zeros(MAX_CALLS, np.uint32)
        run, h0, lag = 0, None, None
        for j, (kind, slot) in enumerate(calls):
            silent = kind == "S" or slot >= n_slots or int(lens[slot]) != 320
            i = np.arange(ROW, dtype=np.int64)
            if silent:
                if run == 0:
                    h0 = self.hist.copy()
                    lag = best_lag(h0)
                    self.lags.append(lag)
                run += 1
                y = synthesis(h0, lag, (run - 1) * ROW + i)
                self.concealed += 1
            else:
                y = np.asarray(rows[slot][:ROW], np.int64).copy()
                if run > 0:
                    cont = synthesis(h0, lag, run * ROW + i[:BLEND])
                    y[:BLEND] = (y[:BLEND] * i[:BLEND] + cont * (BLEND - i[:BLEND])) >> 5
                run = 0
            assert y.min() >= -32768 and y.max() <= 32767
            out[j], len_out[j] = y, 320
            self.hist = np.concatenate([self.hist, y])[-HIST:]
        return out, len_out


def unpack(word):
    """the call list of a uint32 as include/wmix_amd.h lays it out (WMX_RTP_CALLS_*)"""
    word = int(word)
    return [S if (word >> (6 + 4 * j)) & 1 else D((word >> (4 + 4 * j)) & 3) for j in range(min(word & 7, MAX_CALLS))]


def pack(calls):
    word = len(calls)
    for j, (kind, k) in enumerate(calls):
        word |= ((k or 0) | (4 if kind == "S" else 0)) << (4 + 4 * j)
    return word


class LegsPlcModel:
    """n legs; tick() takes what the sequencer left and returns what the kernel leaves"""

    def __init__(self, n):
        self.legs = [LegPlc() for _ in range(n)]

    def reset(self, legs=None):
        for g in (range(len(self.legs)) if legs is None else legs):
            self.legs[g] = LegPlc()

    def tick(self, pcm, lens, lists):
        """pcm int16 [n, K, >= 160], lens [n, K], lists: per leg the call list (or the uint32 words) -> (rows int16 [n, 4, 160] in call
        order, zero where there is no call; len_out uint32 [n, 4])"""
        n = len(self.legs)
        rows, len_out = np.zeros((n, MAX_CALLS, ROW), np.int16), np.zeros((n, MAX_CALLS), np.uint32)
        for g, leg in enumerate(self.legs):
            calls = unpack(lists[g]) if np.isscalar(lists[g]) or isinstance(lists[g], np.integer) else lists[g]
            rows[g], len_out[g] = leg.tick(pcm[g], lens[g], calls)
        return rows, len_out

    def export(self):
        return {"hist": np.array([leg.hist for leg in self.legs]).astype(np.int16),
                "concealed": np.array([leg.concealed for leg in self.legs], np.uint32)}


# ---- the generator of cases
def audio(rng, n):
    """n samples of one of the three kinds: random A-law codes, random mu-law codes, a sine at full scale (+-32 767: the rule's
    overflow bounds) with a period somewhere in or around the lag range"""
    kind = int(rng.integers(0, 3))
    if kind == 0:
        return alaw_decode(rng.integers(0, 256, size=n))
    if kind == 1:
        return ulaw_decode(rng.integers(0, 256, size=n))
    period, phase = float(rng.uniform(20, 160)), float(rng.uniform(0, 6.28))
    return np.round(32767 * np.sin(2 * np.pi * np.arange(n) / period + phase)).astype(np.int16)


SHAPES = ["D", "SD", "SSD", "SSSD", "DDDD", "SDSD", "DSD", "DD", "SDD"]


def gen_case(rng, n_slots, shape=None, unreadable=None, row=ROW):
    """-> (calls, rows int16 [n_slots, row], lens uint32 [n_slots]): one leg's tick.  shape: a string of S and D (default: one of
    SHAPES); the data calls name distinct slots while there are enough, and every slot named holds audio.  unreadable (default: one
    case in six that has a data call): one data call names a slot whose lens is 0 -- or, when n_slots < 4 and the coin says so, a slot
    >= n_slots -- which the rule treats as a silence call.  A slot no call names is empty (lens 0, zeros), as ingest leaves it."""
    shape = shape if shape is not None else SHAPES[int(rng.integers(0, len(SHAPES)))]
    n_data = shape.count("D")
    slots = list(rng.permutation(n_slots)[:n_data]) if n_data <= n_slots else list(rng.integers(0, n_slots, size=n_data))
    rows, lens = np.zeros((n_slots, row), np.int16), np.zeros(n_slots, np.uint32)
    for k in set(int(k) for k in slots):
        rows[k, :ROW], lens[k] = audio(rng, ROW), 320
    calls, it = [], iter(slots)
    for c in shape:
        calls.append(S if c == "S" else D(int(next(it))))
    if unreadable is None:
        unreadable = n_data > 0 and rng.integers(0, 6) == 0
    if unreadable and n_data:
        j = [j for j, c in enumerate(calls) if c[0] == "D"][int(rng.integers(0, n_data))]
        if n_slots < MAX_CALLS and rng.integers(0, 2):
            calls[j] = D(int(rng.integers(n_slots, MAX_CALLS)))
        else:
            lens[calls[j][1]] = 0  # every call that names this slot
    return calls, rows, lens


def run_lengths(calls, lens):
    """the lengths of the runs of silence calls in a list, unreadable data calls counted in"""
    runs, run = [], 0
    for kind, k in calls:
        if kind == "S" or k >= len(lens) or int(lens[k]) != 320:
            run += 1
        else:
            if run:
                runs.append(run)
            run = 0
    if run:
        runs.append(run)
    return runs
