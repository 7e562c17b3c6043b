"""A model of the bridge's DTMF rule (wmx_rtp_detect_dtmf_legs), written from the rule's text in the head of wmix_amd/csrc/leg_dtmf.h:
per leg the debounce state, the last event timestamp, a count and a ring of eight; per tick the leg's datagram rows, what recvfrom
returned, its PCM rows, lens and, with sequencing, the call list.  Python integers throughout the recurrence and the decision; nothing
of the header's code.  Also the signals tests/test_leg_dtmf_host.py, tests/test_rtp_dtmf_gpu.py and tests/conf_inputs.py
share."""
import numpy as np

ROW = 160
FREQS = (697, 770, 852, 941, 1209, 1336, 1477, 1633)
COEF = (27980, 26956, 25701, 24219, 19073, 16325, 13085, 9315)
TABLE = (1, 2, 3, 12, 4, 5, 6, 13, 7, 8, 9, 14, 10, 0, 11, 15)
MIN_POWER = 400000000
KEYS = "0123456789*#ABCD"  # KEYS[code]
FROM_PACKET = 0x80


def powers(x):
    """-> ([P of the eight frequencies], E, the largest |s| reached) of one block of 160 samples"""
    x = [int(v) for v in x[:ROW]]
    assert len(x) == ROW
    out, reach = [], 0
    for coef in COEF:
        s1 = s2 = 0
        for v in x:
            s0 = v + ((coef * s1) >> 14) - s2
            s2, s1 = s1, s0
            reach = max(reach, abs(s1))
        out.append(s1 * s1 + s2 * s2 - ((coef * s1) >> 14) * s2)
    return out, sum(v * v for v in x), reach


def decide(p, e):
    """-> the block's digit, or None"""
    rows, cols = p[:4], p[4:]
    r, c = rows.index(max(rows)), cols.index(max(cols))  # index: the first of equals
    pr, pc = rows[r], cols[c]
    ok = (pr >= MIN_POWER and pc >= MIN_POWER and pc <= 4 * pr and pr <= 8 * pc
          and all(8 * rows[i] <= pr for i in range(4) if i != r) and all(8 * cols[i] <= pc for i in range(4) if i != c)
          and pr + pc >= 32 * e)
    return TABLE[4 * r + c] if ok else None


_seen = {}


def block_digit(x):
    """decide(powers(x)), remembered by the row's bytes: the scripts repeat their rows"""
    key = np.ascontiguousarray(x[:ROW], np.int16).tobytes()
    if key not in _seen:
        p, e, _ = powers(x)
        _seen[key] = decide(p, e)
    return _seen[key]


class LegDtmf:
    def __init__(self):
        self.count, self.ring, self.ts, self.cand, self.cur = 0, [0] * 8, None, None, None

    def report(self, byte):
        self.ring[self.count & 7] = byte
        self.count += 1

    def packets(self, rows, recv, event_pt):
        """rows uint8 [K, >= 16], recv [K]: every slot in slot order"""
        for k in range(len(recv)):
            if int(recv[k]) < 16:
                continue
            row = [int(b) for b in rows[k][:16]]
            if (row[1] & 0x7F) != event_pt or row[12] > 15:
                continue
            ts = tuple(row[4:8])
            if self.ts is None or ts != self.ts:
                self.report(row[12] | FROM_PACKET)
            self.ts = ts

    def block(self, digit):
        if digit is not None:
            if self.cand == digit and self.cur != digit:
                self.report(digit)
                self.cur = digit
        elif self.cand is None:
            self.cur = None
        self.cand = digit

    def tick(self, rows, recv, pcm, lens, calls, event_pt=101, suppress=False):
        """rows uint8 [K, >= 16], recv [K], pcm int16 [K, >= 160] (zeroed in place where suppress says so), lens [K], calls: None (slot
        order) or the list of ("D", slot) / ("S", None) -> the per-block digits"""
        self.packets(rows, recv, event_pt)
        n_slots = len(lens)
        if calls is None:
            calls = [("D", k) for k in range(n_slots) if int(lens[k]) == 320]
        digits = []
        for kind, slot in calls[:4]:
            quiet = kind == "S" or slot >= n_slots or int(lens[slot]) != 320
            digits.append(None if quiet else block_digit(pcm[slot]))
        for d in digits:
            self.block(d)
        for (kind, slot), d in zip(calls, digits):
            if suppress and d is not None:
                pcm[slot][:ROW] = 0
        return digits


class LegsDtmfModel:
    """n legs; tick() takes what the ingest (and the sequencer) left and leaves what the kernel leaves"""

    def __init__(self, n):
        self.legs = [LegDtmf() for _ in range(n)]

    def reset(self, legs=None):
        for g in (range(len(self.legs)) if legs is None else legs):
            self.legs[g] = LegDtmf()

    def tick(self, rows, recv, pcm, lens, lists=None, event_pt=101, suppress=False):
        """rows uint8 [n, K, >= 16], recv [n, K], pcm int16 [n, K, >= 160] (rewritten in place), lens [n, K], lists: None or per leg the
        call list -> per leg the per-block digits"""
        return [leg.tick(rows[g], recv[g], pcm[g], lens[g], None if lists is None else lists[g], event_pt, suppress)
                for g, leg in enumerate(self.legs)]

    def export(self):
        return {"count": np.array([leg.count for leg in self.legs], np.uint32), "ring": np.array([leg.ring for leg in self.legs], np.uint8)}


def digits_of(count, ring, since=0):
    """what a host reads from (count, ring [8]) of one leg: the reports since `since` as (key, from_packet), at most the last eight"""
    return [(KEYS[int(ring[n & 7]) & 0x7F], bool(int(ring[n & 7]) & FROM_PACKET)) for n in range(max(since, int(count) - 8), int(count))]


# ---- signals
def tone(code, amp_row=4000.0, amp_col=4000.0, n0=0, off_row=0.0, off_col=0.0, ph_row=0.0, ph_col=0.0, n=ROW):
    """n samples from sample n0 on of the key `code`: its two sines, each off nominal by a relative offset"""
    at = TABLE.index(code)
    fr, fc = FREQS[at // 4] * (1 + off_row), FREQS[4 + at % 4] * (1 + off_col)
    t = np.arange(n0, n0 + n, dtype=np.float64)
    x = amp_row * np.sin(2 * np.pi * fr * t / 8000 + ph_row) + amp_col * np.sin(2 * np.pi * fc * t / 8000 + ph_col)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def single(f, amp=8000.0, n=ROW):
    return np.round(amp * np.sin(2 * np.pi * f * np.arange(n) / 8000)).astype(np.int16)


def square(f, n=ROW):
    """a full-scale square wave at f Hz: the bound on the recurrence's state"""
    return np.where(np.sin(2 * np.pi * f * (np.arange(n) + 0.5) / 8000) >= 0, 32767, -32768).astype(np.int16)


def noise(rng, amp=3000.0, n=ROW):
    return np.clip(np.round(rng.normal(0, amp, size=n)), -32768, 32767).astype(np.int16)


def event_row(event, ts, pt=101, seq=0, end=False, marker=False, duration=160):
    """the first 16 bytes of an RFC 4733 datagram: the RTP header and the four bytes of the event payload"""
    row = np.zeros(16, np.uint8)
    row[0], row[1] = 0x80, (0x80 if marker else 0) | pt
    row[2], row[3] = (seq >> 8) & 0xFF, seq & 0xFF
    row[4:8] = [(ts >> 24) & 0xFF, (ts >> 16) & 0xFF, (ts >> 8) & 0xFF, ts & 0xFF]
    row[12], row[13] = event, (0x80 if end else 0) | 10
    row[14], row[15] = (duration >> 8) & 0xFF, duration & 0xFF
    return row
