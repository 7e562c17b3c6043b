"""The bridge's DTMF rule on the CPU (wmix_amd/csrc/leg_dtmf.h: what wmx_rtp_detect_dtmf_legs applies on the device per leg and tick).
tools_dev/san/leg_dtmf_san.cpp, a stand-alone program compiled with g++ against the header the kernel includes and with
AddressSanitizer + UndefinedBehaviorSanitizer, evaluates the header; tests/leg_dtmf_model.py, written from the rule's text in Python
integers, is what it must equal: the eight powers, E and the decision of every block; the per-block digits, count, the ring bytes and
the rows after suppression of every tick.  Integers, ==."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from leg_dtmf_model import FREQS, KEYS, ROW, TABLE, LegDtmf, decide, digits_of, event_row, noise, powers, single, square, tone
from leg_plc_model import D, S, pack

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Werror",
       "-Wno-unused-function"]
CSRC = os.path.join(ROOT, "wmix_amd", "csrc")
QUIET = np.zeros(ROW, np.int16)
NOTHING = np.zeros(16, np.uint8)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("leg_dtmf") / "leg_dtmf_san"
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tools_dev", "san", "leg_dtmf_san.cpp")])
    return str(exe)


def run(program, mode, stdin):
    r = subprocess.run([program, mode], input=stdin, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    return r.stdout.splitlines()


def blocks(program, rows):
    """-> per row ([P] * 8, E, digit or None, reach) from the header"""
    lines = run(program, "blocks", "".join(" ".join(map(str, x)) + "\n" for x in rows))
    assert len(lines) == len(rows)
    out = []
    for line in lines:
        v = [int(t) for t in line.split()]
        out.append((v[:8], v[8], None if v[9] < 0 else v[9], v[10]))
    return out


def same_blocks(program, rows, what):
    """the header equals the model on every row -> the digits"""
    got = blocks(program, rows)
    for n, (x, g) in enumerate(zip(rows, got)):
        p, e, reach = powers(x)
        assert g[0] == p and g[1] == e and g[3] == reach, (what, n, "powers / E / reach", g, p, e, reach)
        assert g[2] == decide(p, e), (what, n, "decision", g[2], decide(p, e))
    return [g[2] for g in got]


def test_every_key_at_nominal_frequency_quiet_and_loud(program):
    for amp in (500.0, 8000.0):
        rows = [tone(code, amp, amp, ph_row=0.3 * code, ph_col=1.1 + 0.2 * code) for code in range(16)]
        assert same_blocks(program, rows, ("amp", amp)) == list(range(16))
    assert TABLE[4 * 1 + 1] == 5 and KEYS[10] == "*" and KEYS[11] == "#" and KEYS[12] == "A"


def test_both_tones_off_nominal_by_one_and_a_half_percent(program):
    rows, want = [], []
    for code in range(16):
        for off_row, off_col in ((0.015, 0.015), (-0.015, -0.015), (0.015, -0.015), (-0.015, 0.015)):
            rows.append(tone(code, 3000.0, 3000.0, off_row=off_row, off_col=off_col, ph_row=0.7, ph_col=2.0))
            want.append(code)
    assert same_blocks(program, rows, "offsets") == want


def test_the_twist_limits_just_inside_and_just_outside(program):
    """P goes with the square of the amplitude: P_c <= 4 P_r ends at a column twice the row, P_r <= 8 P_c at a row sqrt(8) = 2.83 times
    the column"""
    rows = [tone(5, 3000.0, 3000.0 * 1.9), tone(5, 3000.0, 3000.0 * 2.1), tone(5, 3000.0 * 2.7, 3000.0), tone(5, 3000.0 * 2.95, 3000.0)]
    assert same_blocks(program, rows, "twist") == [5, None, 5, None]
    for x, inside in zip(rows, (True, False, True, False)):
        p, _, _ = powers(x)
        assert (p[5] <= 4 * p[1] and p[1] <= 8 * p[5]) == inside


def test_a_full_scale_square_wave_bounds_the_state(program):
    rows = [square(f) for f in FREQS] + [np.full(ROW, 32767, np.int16), np.full(ROW, -32768, np.int16)]
    assert same_blocks(program, rows, "square") == [None] * len(rows)
    reach = [g[3] for g in blocks(program, rows)]
    assert 5000000 < max(reach) < 2 ** 24 and max(reach) == reach[0]  # the lowest frequency resonates longest


def test_silence_noise_and_single_tones_are_no_key(program):
    rng = np.random.default_rng(5)
    rows = [QUIET] + [noise(rng, amp) for amp in (300.0, 3000.0, 12000.0) for _ in range(8)] + [single(f) for f in FREQS]
    rows += [single(f, 30000.0) for f in (697, 1633)] + [tone(7, 100.0, 100.0)]  # and a key below the absolute threshold
    assert same_blocks(program, rows, "negatives") == [None] * len(rows)


def test_random_blocks_equal_the_model(program):
    rng = np.random.default_rng(6)
    rows = []
    for _ in range(150):
        code = int(rng.integers(0, 16))
        x = tone(code, float(rng.uniform(300, 14000)), float(rng.uniform(300, 14000)), off_row=float(rng.uniform(-0.03, 0.03)),
                 off_col=float(rng.uniform(-0.03, 0.03)), ph_row=float(rng.uniform(0, 6.28)), ph_col=float(rng.uniform(0, 6.28)))
        rows.append(np.clip(x.astype(np.int64) + noise(rng, float(rng.uniform(0, 2000))), -32768, 32767).astype(np.int16))
    got = same_blocks(program, rows, "random")
    assert sum(d is not None for d in got) >= 30 and sum(d is None for d in got) >= 30


# ---- ticks: the debounce, the event packets, the report, suppression
def tick_text(rows, recv, pcm, lens, calls):
    k = len(lens)
    head = "T %d %d %d %s %s" % (k, 0 if calls is None else 1, 0 if calls is None else pack(calls), " ".join(map(str, recv)), " ".join(map(str, lens)))
    return head + "".join(" " + " ".join(map(str, rows[s][:16])) + " " + " ".join(map(str, pcm[s][:ROW])) for s in range(k)) + "\n"


def same_ticks(program, ticks, event_pt=101, suppress=False):
    """ticks: (rows uint8 [K, 16], recv [K], pcm int16 [K, 160], lens [K], calls or None) of one leg -> the model afterwards; the header
    equals it after every tick"""
    lines = run(program, "ticks", "L %d %d\n" % (event_pt, 1 if suppress else 0) + "".join(tick_text(*t) for t in ticks))
    assert len(lines) == len(ticks)
    leg = LegDtmf()
    for n, ((rows, recv, pcm, lens, calls), line) in enumerate(zip(ticks, lines)):
        pcm = np.array(pcm, np.int16)
        digits = leg.tick(rows, recv, pcm, lens, calls, event_pt, suppress)
        v = [int(t) for t in line.split()]
        assert v[0] == len(digits) and v[1:5] == [-1 if d is None else d for d in digits] + [-1] * (4 - len(digits)), ("tick", n, v[:5], digits)
        assert v[5] == leg.count and v[6:14] == leg.ring, ("tick", n, "count / ring", v[5:14], leg.count, leg.ring)
        assert np.array_equal(np.array(v[14:], np.int16).reshape(pcm.shape), pcm), ("tick", n, "rows")
    return leg


def audio_tick(x):
    """one packet of audio in slot order, nothing else"""
    return (np.stack([NOTHING]), [172], np.stack([x]), [320], None)


def key_packets(code, n, n0=0):
    return [tone(code, 4000.0, 4000.0, n0=n0 + ROW * i) for i in range(n)]


def test_a_key_that_fills_one_packet_is_not_reported_two_are(program):
    leg = same_ticks(program, [audio_tick(x) for x in [QUIET] + key_packets(5, 1) + [QUIET, QUIET] + key_packets(9, 2) + [QUIET]])
    assert digits_of(leg.count, leg.ring) == [("9", False)]


def test_the_same_key_again_needs_two_quiet_packets(program):
    one = same_ticks(program, [audio_tick(x) for x in key_packets(3, 3) + [QUIET] + key_packets(3, 3, 640)])
    assert digits_of(one.count, one.ring) == [("3", False)]
    two = same_ticks(program, [audio_tick(x) for x in key_packets(3, 3) + [QUIET, QUIET] + key_packets(3, 3, 800)])
    assert digits_of(two.count, two.ring) == [("3", False), ("3", False)]
    # another key needs no pause at all
    other = same_ticks(program, [audio_tick(x) for x in key_packets(3, 2) + key_packets(4, 2, 320)])
    assert digits_of(other.count, other.ring) == [("3", False), ("4", False)]


def test_ten_keys_wrap_the_ring_of_eight(program):
    ticks = []
    for code in (1, 2, 3, 4, 5, 6, 7, 8, 9, 0):
        ticks += [audio_tick(x) for x in key_packets(code, 2)]
    leg = same_ticks(program, ticks)
    assert leg.count == 10 and leg.ring == [9, 0, 3, 4, 5, 6, 7, 8]
    assert "".join(k for k, _ in digits_of(leg.count, leg.ring, since=4)) == "567890"


def event_tick(rows, recv=None):
    k = len(rows)
    return (np.stack(rows), [172] * k if recv is None else recv, np.zeros((k, ROW), np.int16), [0] * k, None)


def test_event_packets_report_once_per_timestamp(program):
    ticks = [event_tick([event_row(7, 1000, seq=s, marker=s == 1)]) for s in (1, 2, 3)] + [event_tick([event_row(7, 1000, seq=4, end=True)])]
    leg = same_ticks(program, ticks)
    assert digits_of(leg.count, leg.ring) == [("7", True)]
    ticks += [event_tick([event_row(11, 1800, seq=5), event_row(11, 1800, seq=6, end=True)])]  # a second key, two packets in one tick
    ticks += [event_tick([event_row(16, 2600, seq=7)])]                    # flash: ignored
    ticks += [event_tick([event_row(2, 3400, seq=8)], recv=[15])]          # too short to hold an event
    ticks += [event_tick([event_row(2, 3400, seq=9, pt=100)])]             # not the negotiated payload type
    ticks += [event_tick([event_row(2, 3400, seq=10)], recv=[16])]         # the shortest packet that does
    ticks += [event_tick([event_row(7, 1000, seq=11)])]                    # an old timestamp is another timestamp
    leg = same_ticks(program, ticks)
    assert digits_of(leg.count, leg.ring) == [("7", True), ("#", True), ("2", True), ("7", True)]
    other = same_ticks(program, ticks, event_pt=100)
    assert digits_of(other.count, other.ring) == [("2", True)]


def test_a_first_event_at_timestamp_zero_is_reported(program):
    leg = same_ticks(program, [event_tick([event_row(0, 0)]), event_tick([event_row(0, 0, end=True)])])
    assert digits_of(leg.count, leg.ring) == [("0", True)]


def test_packet_reports_come_before_in_band_reports_of_the_tick(program):
    a, b = key_packets(5, 2)
    ticks = [(np.stack([NOTHING, NOTHING, NOTHING]), [172, 0, 0], np.stack([a, QUIET, QUIET]), [320, 0, 0], None),
             (np.stack([NOTHING, event_row(1, 4000), NOTHING]), [172, 172, 0], np.stack([b, QUIET, QUIET]), [320, 0, 0], None)]
    leg = same_ticks(program, ticks)
    assert digits_of(leg.count, leg.ring) == [("1", True), ("5", False)]


def test_a_call_list_is_walked_in_list_order_and_silence_is_no_tone(program):
    a, b, c = key_packets(8, 3)
    rows, recv = np.stack([NOTHING] * 3), [172] * 3
    # slots out of order on the wire: the list puts them right, and two packets in sequence report the key
    leg = same_ticks(program, [(rows, recv, np.stack([b, a, QUIET]), [320, 320, 0], [D(1), D(0)])])
    assert digits_of(leg.count, leg.ring) == [("8", False)]
    # a silence call between two tone packets: no two consecutive blocks, no report; and a data call naming an unreadable row is one
    for calls, lens in (([D(0), S, D(1)], [320, 320, 0]), ([D(0), D(2), D(1)], [320, 320, 0]), ([D(0), D(3), D(1)], [320, 320, 320])):
        leg = same_ticks(program, [(rows, recv, np.stack([a, b, c]), lens, calls)], suppress=True)
        assert leg.count == 0
    # two quiet calls end the key, so it is reported again; without the list the same rows in slot order are one press
    pcm = np.stack([a, b, QUIET])
    again = same_ticks(program, [(rows, recv, pcm, [320, 320, 320], [D(0), D(1)]), (rows, recv, pcm, [320, 320, 320], [S, D(2), D(0), D(1)])])
    assert digits_of(again.count, again.ring) == [("8", False), ("8", False)]


def test_suppression_zeroes_every_tone_block_and_only_those(program):
    rng = np.random.default_rng(8)
    a, b = key_packets(6, 2)
    voice = noise(rng)
    ticks = [(np.stack([NOTHING] * 3), [172] * 3, np.stack([a, voice, b]), [320, 320, 320], None)]
    for suppress in (False, True):
        leg = same_ticks(program, ticks, suppress=suppress)
        assert leg.count == 0  # tone, voice, tone: never two in a row -- and both tone rows are zeroed all the same
    pcm = np.array(ticks[0][2])
    LegDtmf().tick(ticks[0][0], ticks[0][1], pcm, ticks[0][3], None, 101, True)
    assert not pcm[0].any() and not pcm[2].any() and np.array_equal(pcm[1], voice)


def test_a_leg_with_no_block_keeps_its_state(program):
    a, b = key_packets(2, 2)
    nothing = (np.stack([NOTHING]), [0], np.stack([QUIET]), [0], None)
    leg = same_ticks(program, [audio_tick(a), nothing, nothing, nothing, audio_tick(b)])
    assert digits_of(leg.count, leg.ring) == [("2", False)]
