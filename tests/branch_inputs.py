"""A catalogue of inputs chosen with the reference's CONTROL FLOW in mind (not a test module; tests/test_branches_gpu.py,
tests/test_oracle_extremes.py and tests/test_oracle_branches.py use it).

The other generators of the suite (the *_case_input recipes, extreme_signals, the perfect echoes, tones and click trains,
_edge_signals, synth.*) are loud, stationary or full-scale; a data-dependent branch none of them takes is compared nowhere -- not in a
kernel against the oracle, and not in the oracle against the real reference.  Every entry here exists for branch outcomes of
oracle/orc_*.c that those generators leave untaken (its `claims`: keys of tools_dev/oracle_branches.py, kept as data in
tests/golden/branch_claims.json); tests/test_oracle_branches.py fails when an entry stops taking one of them.

An entry is a deterministic function of its seed: a named signal recipe (SIGNALS), for the cancellers a named far end (FARS) and a
named schedule of reported delays (SCHEDULES), and the stage's configuration.  Its length is the shortest of a coarse grid at which
the claimed outcomes are taken, plus 100 packets, so that what the branch decided reaches compared output.

The recipes no entry uses stay: together they are the search the entries were chosen from (every signal x every rate of a stage, for
the cancellers x far ends x echo paths x delay schedules; greedy cover of the outcomes newly taken, then the shortest length), and
the `open` rows of tests/golden/oracle_unreached.json say "tried" about exactly this set.
"""
import json
import os
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CLAIMS_JSON = os.path.join(HERE, "golden", "branch_claims.json")


# ---------------------------------------------------------------- signal recipes: f(rng, freq, n packets) -> float or int array
def _noise(rng, amp, size):
    return rng.integers(-amp, amp + 1, size)


def _tone(freq, size, hz, amp):
    return np.round(amp * np.sin(2 * np.pi * hz * np.arange(size) / freq))


def _level_steps(levels):
    """noise whose amplitude is levels[k] from packet p_k on: levels = ((packet, amplitude), ...), amplitude 0 = digital silence"""
    def f(rng, freq, n):
        pkt = freq // 100
        x = np.zeros(n * pkt)
        for k, (p, a) in enumerate(levels):
            q = min(levels[k + 1][0] if k + 1 < len(levels) else n, n)
            p = min(p, n)
            if a and q > p:
                x[p * pkt:q * pkt] = _noise(rng, a, (q - p) * pkt)
        return x
    return f


def _alternate(period, lo=30, hi=12000):
    def f(rng, freq, n):
        pkt = freq // 100
        loud = (np.arange(n * pkt) // (pkt * period)) % 2 == 1
        return np.where(loud, _noise(rng, hi, n * pkt), _noise(rng, lo, n * pkt))
    return f


def _fade_out(rng, freq, n):
    N = n * (freq // 100)
    g = np.clip(1.0 - np.arange(N) / (0.6 * N), 0.0, 1.0)
    return np.trunc(_noise(rng, 8000, N) * g)


def _ramp_up(rng, freq, n):
    N = n * (freq // 100)
    g = np.clip((np.arange(N) - 0.2 * N) / (0.8 * N), 0.0, 1.0)
    return np.trunc(_noise(rng, 12000, N) * g)


def _gated_tone(rng, freq, n):
    pkt = freq // 100
    on = (np.arange(n * pkt) // (pkt * 40)) % 2 == 1
    return _tone(freq, n * pkt, 300.0, 8000) * on + _noise(rng, 4, n * pkt)


def _walk(rng, freq, n):
    x, out = 0, np.empty(n * (freq // 100))
    steps = rng.integers(-300, 301, out.size)
    for i, s in enumerate(steps):
        x += s
        if abs(x) > 20000:
            x -= 2 * s
        out[i] = x
    return out


def _silence_then(amp, frac=0.4):
    def f(rng, freq, n):
        N = n * (freq // 100)
        x = _noise(rng, amp, N)
        x[: int(frac * N)] = 0
        return x
    return f


def _two_peaks(rng, freq, n):
    """two levels close together, switched every 3 packets: the per-block features (flatness, spectral difference, LRT) fall into two
    neighbouring histogram bins"""
    pkt = freq // 100
    k = (np.arange(n * pkt) // (pkt * 3)) % 2
    return np.where(k == 0, _noise(rng, 900, n * pkt), _tone(freq, n * pkt, 700.0, 1100) + _noise(rng, 500, n * pkt))


def _clipping_both_sides(rng, freq, n):
    """a tone over noise that the suppressors' synthesis (and the AGC's gain) pushes past +32767 and below -32768"""
    N = n * (freq // 100)
    return np.clip(_tone(freq, N, 1000.0, 32767) * 1.0 + _noise(rng, 6000, N), -32768, 32767)


SIGNALS = {
    "fade_out": _fade_out,
    "ramp_up": _ramp_up,
    "gated_tone": _gated_tone,
    "alt200": _alternate(200),
    "alt7": _alternate(7),
    "tone440": lambda rng, freq, n: _tone(freq, n * (freq // 100), 440.0, 10000),
    "tone_nyq": lambda rng, freq, n: _tone(freq, n * (freq // 100), freq / 2 - 50.0, 10000),
    "tone50": lambda rng, freq, n: _tone(freq, n * (freq // 100), 50.0, 10000),
    "walk": _walk,
    "silence_then_5": _silence_then(5),
    "silence_then_2000": _silence_then(2000, 0.1),
    "two_tones": lambda rng, freq, n: _tone(freq, n * (freq // 100), 1000.0, 6000) + _tone(freq, n * (freq // 100), 1031.25, 6000),
    # aimed at the once-per-500-blocks model update of NS / NSX: a level step or a gap just before / across the window's end
    "step_at_480": _level_steps(((0, 100), (480, 5000))),
    "step_down_at_480": _level_steps(((0, 5000), (480, 40))),
    "gap_450_560": _level_steps(((0, 3000), (450, 0), (560, 3000))),
    "quiet_loud_quiet": _level_steps(((0, 20), (300, 9000), (520, 20), (900, 9000))),
    "two_peaks": _two_peaks,
    "clip_both": _clipping_both_sides,
    "silence": lambda rng, freq, n: np.zeros(n * (freq // 100)),
    "alt200_loud": _alternate(200, 3, 32767),
    "alt7_loud": _alternate(7, 3, 32767),
    "tone_bin_full": lambda rng, freq, n: _tone(freq, n * (freq // 100), 16 * min(freq, 16000) / 256.0, 32767),
    "tone440_full": lambda rng, freq, n: _tone(freq, n * (freq // 100), 440.0, 32767),
    "tone50_full": lambda rng, freq, n: _tone(freq, n * (freq // 100), 50.0, 32767),
    "ramp_full": lambda rng, freq, n: np.trunc(_noise(rng, 32767, n * (freq // 100)) * np.linspace(0, 1, n * (freq // 100))),
    "dc_step": lambda rng, freq, n: np.where(np.arange(n * (freq // 100)) // (freq // 100 * 150) % 2 == 0, -30000, 30000) + _noise(rng, 20, n * (freq // 100)),
    # period = half / a quarter of the suppressors' FFT length (256 at 16 / 32 kHz, 128 at 8 kHz): all the energy in every 2nd / 4th bin,
    # so the inverse FFT's intermediate values are at full size stages before the last one
    "clicks_half_fft": lambda rng, freq, n: (np.arange(n * (freq // 100)) % (64 if freq == 8000 else 128) == 0) * 32767.0,
    "clicks_quarter_fft": lambda rng, freq, n: (np.arange(n * (freq // 100)) % (32 if freq == 8000 else 64) == 0) * 32767.0,
    "square_half_fft": lambda rng, freq, n: np.where(np.arange(n * (freq // 100)) // (16 if freq == 8000 else 32) % 2 == 0, 32767.0, -32768.0),
    "clicks_in_quiet": lambda rng, freq, n: (np.arange(n * (freq // 100)) % 4001 == 0) * 32767.0 + _noise(rng, 2, n * (freq // 100)),
}
for _a in (1, 3, 12, 60, 300, 1500, 7000, 30000):
    SIGNALS["noise_%d" % _a] = (lambda a: lambda rng, freq, n: _noise(rng, a, n * (freq // 100)))(_a)


# ---------------------------------------------------------------- far ends of the cancellers
FARS = {
    "noise": lambda rng, freq, n: _noise(rng, 8000, n * (freq // 100)),
    "quiet": lambda rng, freq, n: _noise(rng, 40, n * (freq // 100)),
    # the same energy in every block from the first one on (AECM's start-up far-energy tracking sees no change)
    "square": lambda rng, freq, n: np.where((np.arange(n * (freq // 100)) // 8) % 2 == 0, 6000, -6000),
    "late": _level_steps(((0, 0), (120, 8000))),
    # nothing for the first 512 blocks and more (AECM leaves its start-up state by the block count alone), then loud
    "late450": _level_steps(((0, 0), (450, 8000))),
    "step450": _level_steps(((0, 40), (450, 8000))),
    "drop450": _level_steps(((0, 8000), (450, 300))),
    "drop450_square": lambda rng, freq, n: np.where((np.arange(n * (freq // 100)) // 8) % 2 == 0, 1, -1) * np.where(np.arange(n * (freq // 100)) < 450 * (freq // 100), 8000, 2000),
    "bursts": _alternate(25, 0, 14000),
    "silence": lambda rng, freq, n: np.zeros(n * (freq // 100)),
}
# how the far end gets into the near end: near = signal + echo
ECHOES = {
    "half37": lambda far: np.roll(far, 37) // 2,           # the sweep's: half of the far end, 37 samples late
    "x4": lambda far: np.roll(far, 37) * 4,                 # echo stronger than the far end (NLP gains at their clamps)
    "late400": lambda far: np.roll(far, 3237) // 2,        # an echo path longer than the filter at start-up
    "none": lambda far: np.zeros_like(far),
}


# ---------------------------------------------------------------- reported delays, one per call: f(rng, n calls) -> int32 [n]
def _const(ms):
    return lambda rng, n: np.full(n, ms, np.int32)


def _with_bad_calls(ms, bad):
    """a steady delay with single calls that report `bad`: aec_process2 returns -1 for those and leaves their output unwritten
    (src/webrtc.c:382-387); the handle lives on"""
    def f(rng, n):
        d = np.full(n, ms, np.int32)
        d[5::41] = bad
        return d
    return f


def _jumping_start(rng, n):
    d = np.full(n, 120, np.int32)
    d[:70] = np.where(np.arange(70) % 2 == 0, 20, 400)[:n]
    return d


def _step(rng, n):
    d = np.zeros(n, np.int32)
    d[n // 3:] = 300
    d[2 * n // 3:] = 40
    return d


SCHEDULES = {
    "d0": _const(0),
    "d250": _const(250),
    "d500": _const(500),
    "neg5": _with_bad_calls(40, -5),
    "over600": _with_bad_calls(40, 600),
    "random": lambda rng, n: rng.integers(0, 501, n).astype(np.int32),
    "jumping_start": _jumping_start,
    "step": _step,
}


# ---------------------------------------------------------------- entries
Entry = namedtuple("Entry", "name stage chn freq n seed signal interval value far echo schedule")


def E(stage, chn, freq, n, signal, seed=1, interval=10, value=5, far="noise", echo="half37", schedule="d0"):
    if stage in ("aec", "aecm"):
        name = "%s_%dx%d_%dms_%s_%s_%s_%s" % (stage, chn, freq, interval, signal, far, echo, schedule)
    elif stage == "agc":
        name = "agc_%dx%d_v%d_%s" % (chn, freq, value, signal)
    elif stage == "vad":
        name = "vad_%dx%d_%dms_%s" % (chn, freq, interval, signal)
    else:
        name = "%s_%dx%d_%s" % (stage, chn, freq, signal)
    return Entry(name, stage, chn, freq, n, seed, signal, interval, value, far, echo, schedule)


def packet(e):
    """samples per channel of one wrapper packet (src/webrtc.c: 10 ms; 20 ms for AEC / VAD when rate and interval allow it)"""
    if e.stage in ("aec", "aecm"):
        return e.freq // 1000 * (20 if e.freq <= 8000 and e.interval % 20 == 0 else 10)
    if e.stage == "vad":
        return e.freq // 1000 * (20 if e.freq <= 16000 and e.interval % 20 == 0 else 10)
    return e.freq // 100


def _i16(x, chn):
    x = np.clip(x, -32768, 32767).astype(np.int16)
    if chn == 2:  # the wrappers average the channels (NS / NSX take them as bands): the second carries the negated signal's half
        y = np.empty(x.size * 2, np.int16)
        y[0::2] = x
        y[1::2] = -(x // 2)
        return y
    return x


def make(e):
    """(far or None, near, delays or None): int16 [n packets * packet * chn], int32 [n packets]"""
    rng = np.random.default_rng(e.seed)
    n10 = e.n * packet(e) // (e.freq // 100)  # the recipes count 10 ms packets
    x = np.asarray(SIGNALS[e.signal](rng, e.freq, n10), np.float64)
    if e.stage not in ("aec", "aecm"):
        return None, _i16(x, e.chn), None
    far = np.asarray(FARS[e.far](rng, e.freq, n10)).astype(np.int64)
    near = x + ECHOES[e.echo](far)
    return _i16(far, e.chn), _i16(near, e.chn), SCHEDULES[e.schedule](rng, e.n)


def run(lib, e, prefix, data=None):
    """The entry through the restatement (prefix "orc") or the real reference (prefix "ref"; NSX and AECM: its nsx_ns_* / aecm_aec_*
    builds).  Returns (output, return codes per call or None)."""
    from oracle import loader as L
    far, near, delays = data if data is not None else make(e)
    p = packet(e)
    if e.stage == "ns":
        return L.run_ns(lib, e.chn, e.freq, near, p, prefix=prefix), None
    if e.stage == "nsx":
        return L.run_nsx(lib, e.chn, e.freq, near, p, prefix=prefix), None
    if e.stage == "agc":
        return L.run_agc(lib, e.chn, e.freq, e.value, near, p, prefix=prefix), None
    if e.stage == "vad":
        return L.run_vad(lib, e.chn, e.freq, e.interval, near, p, prefix=prefix), None
    return L.run_canceller_calls(lib, e.stage, e.chn, e.freq, e.interval, far, near, p, delays, prefix=prefix)


# stage, chn, freq, packets, signal, then what differs from E's defaults
CATALOGUE = [
    E("ns", 1, 16000, 900, "alt200_loud"),
    E("ns", 1, 16000, 140, "tone_nyq"),
    E("nsx", 1, 8000, 140, "tone_nyq"),
    E("nsx", 1, 8000, 700, "walk"),
    E("nsx", 1, 16000, 900, "alt200"),
    E("nsx", 1, 16000, 1100, "alt7"),
    E("nsx", 1, 16000, 1100, "fade_out"),
    E("nsx", 1, 16000, 1100, "tone50"),
    E("nsx", 1, 16000, 700, "two_peaks"),
    E("nsx", 1, 32000, 1100, "step_at_480"),
    E("aec", 1, 8000, 200, "noise_60", interval=20, schedule="jumping_start"),
    E("aec", 1, 16000, 200, "noise_60", schedule="neg5"),
    E("aec", 1, 16000, 140, "noise_60", schedule="over600"),
    E("aec", 1, 16000, 140, "noise_60", schedule="d500"),
    E("aecm", 1, 8000, 250, "noise_3", far="bursts", echo="half37"),
    E("aecm", 1, 8000, 140, "noise_60", interval=20, schedule="jumping_start"),
    E("aecm", 1, 16000, 1000, "clicks_in_quiet", schedule="random"),
    E("aecm", 1, 16000, 1000, "noise_1", far="square", echo="half37"),
    E("aecm", 1, 16000, 160, "noise_60", schedule="neg5"),
    E("aecm", 1, 16000, 160, "noise_60", schedule="over600"),
    E("aecm", 1, 16000, 160, "noise_60", schedule="d500"),
    E("aecm", 1, 16000, 1200, "tone440", far="step450", echo="none"),
    E("agc", 1, 32000, 500, "fade_out", value=5),
]
assert len({e.name for e in CATALOGUE}) == len(CATALOGUE)
with open(CLAIMS_JSON) as _f:
    CLAIMS = json.load(_f)   # {entry name: [outcome keys it exists for]}
assert set(CLAIMS) <= {e.name for e in CATALOGUE}, sorted(set(CLAIMS) - {e.name for e in CATALOGUE})

