"""examples/host_conf.c --record LEG,CHN,FREQ,SECONDS --record-dir DIR: the C example recording what two legs hear
(wmx_conf_recorders, wmx_conf_record, wmx_conf_rec / wmx_conf_rec_legs), in the manner of tests/test_host_conf_duck_gpu.py.  Each WAV
opens with Python's wave module at the stated format and holds exactly the samples of tests/conf_record_replay.py over the same script;
the datagrams are those of the run without --record.

conf_harness.host_conf runs the family's 40 ticks, which is less than one second: there both taps run until the end.  The tap of one
second needs a longer run to end by itself, so the same command line is run once more over 60 ticks: exactly 50 packages."""
import json
import os
import subprocess
import wave

import numpy as np
import pytest

import conftest
from conf_harness import host_conf
from conf_inputs import G, K, LAYOUT, SEED, T, arrivals
from conf_record_replay import replay_record_story

pytestmark = pytest.mark.gpu

CHN, FREQ, ROW = 2, 16000, 640  # a package of 160 samples of 1 x 8000 is 320 frames of 2 x 16000
LONG_T = 60


def story(c):
    c.set_conferences(LAYOUT)
    c.recorders(2, CHN, FREQ)
    c.record([5], seconds=0)
    c.record([3], seconds=1)


def record_args(tmp_path):
    return ["--record", "5,%d,%d,0" % (CHN, FREQ), "--record", "3,%d,%d,1" % (CHN, FREQ), "--record-dir", str(tmp_path)]


def wav_samples(path):
    with wave.open(str(path), "rb") as w:
        assert (w.getnchannels(), w.getframerate(), w.getsampwidth(), w.getcomptype()) == (CHN, FREQ, 2, "NONE")
        frames = w.getnframes()
        data = np.frombuffer(w.readframes(frames), dtype="<i2")
    assert os.path.getsize(path) == 44 + 2 * data.size and data.size == frames * CHN  # the canonical header, both lengths patched
    return data


def replayed_rows(m, leg):
    rows = [row for legs, now in zip(m.rec_legs, m.rec_rows) for g, row in zip(legs, now) if g == leg]
    return np.concatenate(rows), len(rows)


def check(tmp_path, info, got, want, m, ticks, packages):
    assert info["rc"] == 0 and info["record_taps"] == 2 and info["record_format"] == [CHN, FREQ]
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:6]
    total = 0
    for leg in (5, 3):
        want_pcm, rows = replayed_rows(m, leg)
        assert rows == packages[leg] and want_pcm.size == rows * ROW
        pcm = wav_samples(tmp_path / ("leg%d.wav" % leg))
        assert np.array_equal(pcm, want_pcm), (leg, pcm.size, want_pcm.size)
        assert np.count_nonzero(pcm) > pcm.size // 2
        total += rows
    assert info["record_rows"] == total


def test_host_conf_records_what_the_replay_records(tmp_path, cuda, oracle_port):
    info, got = host_conf(tmp_path, *record_args(tmp_path))
    plain_info, plain = host_conf(tmp_path)
    pk, recv = arrivals(SEED, T, G)
    want, _, m = replay_record_story(oracle_port, G, K, pk, recv, story)
    assert np.array_equal(plain, want) and "record_taps" not in plain_info  # the same datagrams with and without recording
    check(tmp_path, info, got, want, m, T, {5: T, 3: T})  # 40 ticks: the second is not over


def test_the_tap_of_one_second_holds_exactly_fifty_packages(tmp_path, cuda, oracle_port):
    exe = os.path.join(conftest.ROOT, "examples", "host_conf")
    out = tmp_path / "out.rtp"
    r = subprocess.run([exe, str(out), str(G), str(LONG_T), "--sizes", "2,3,4", "--seed", str(SEED)] + record_args(tmp_path), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    info, got = json.loads(r.stdout.strip().splitlines()[-1]), np.fromfile(out, dtype=np.uint8).reshape(LONG_T, G, 172)
    pk, recv = arrivals(SEED, LONG_T, G)
    want, _, m = replay_record_story(oracle_port, G, K, pk, recv, story)
    check(tmp_path, info, got, want, m, LONG_T, {5: LONG_T, 3: 50})
    assert m.rec_seen[-1]["leg"].tolist() == [5, -1] and m.rec_seen[-1]["written"].tolist() == [LONG_T, 50]


def test_host_conf_refuses_two_formats_and_what_the_library_refuses(tmp_path, cuda):
    exe = os.path.join(conftest.ROOT, "examples", "host_conf")
    base = [exe, str(tmp_path / "o.rtp"), str(G), "4", "--sizes", "2,3,4", "--seed", str(SEED), "--record-dir", str(tmp_path)]
    r = subprocess.run(base + ["--record", "1,2,16000", "--record", "2,1,8000"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "ONE format" in r.stderr
    r = subprocess.run(base + ["--record", "1,2,96000"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 4 and "wmx_rtp_recorders" in r.stderr
    r = subprocess.run(base + ["--record", "%d" % G], capture_output=True, text=True, timeout=60)
    assert r.returncode == 4 and "leg" in r.stderr
