"""The codec rule of an RTP leg on the CPU (wmix_amd/csrc/leg_codec.h: what wmx_rtp_ingest_legs_codecs and the egress kernels apply on the
device per leg).  tools_dev/san/leg_codec_san.cpp, a stand-alone program compiled with g++ against the header the kernels include and
with AddressSanitizer + UndefinedBehaviorSanitizer, evaluates the header for all 128 payload types x 4 codecs x arrived / not arrived;
tests/leg_codec_model.py, written from the rule's table, is what it must equal on call, law and refused; for WMX_CODEC_REFERENCE the
call is the length rule of the oracle's orc_rtp_ingest."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from leg_codec_model import BY_PT, LAW_A, LAW_U, PCMA, PCMU, REFERENCE, out_pt, slot
from oracle import loader as L

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Werror",
       "-Wno-unused-function"]
CSRC = os.path.join(ROOT, "wmix_amd", "csrc")


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = tmp_path_factory.mktemp("leg_codec") / "leg_codec_san"
    subprocess.check_call(["g++", "-std=c++17"] + SAN + ["-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tools_dev", "san", "leg_codec_san.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    lines = [line.split() for line in r.stdout.splitlines()]
    cases = {tuple(int(x) for x in w[:3]): tuple(int(x) for x in w[3:]) for w in lines if w[0] not in ("law", "valid")}
    laws = {int(w[1]): int(w[2]) for w in lines if w[0] == "law"}
    valid = {int(w[1]): (int(w[2]), int(w[3])) for w in lines if w[0] == "valid"}
    return cases, laws, valid


def test_every_case_equals_the_model(answers):
    cases, _, _ = answers
    assert len(cases) == 4 * 2 * 128
    seen = set()
    for codec in (REFERENCE, PCMA, PCMU, BY_PT):
        for arrived in (0, 1):
            for pt in range(128):
                call, law, refused = slot(arrived, pt, codec)
                want = (int(call), int(law == "u"), int(refused))
                assert cases[(codec, arrived, pt)] == want, ("in_codec", codec, "arrived", arrived, "pt", pt, cases[(codec, arrived, pt)], want)
                seen.add((codec,) + want)
    # the table's every outcome is reached: each codec calls, refuses and does neither; mu-law only on PCMU and BY_PT
    for codec in (REFERENCE, PCMA, PCMU, BY_PT):
        assert (codec, 0, 0, 0) in seen and (codec, 0, 0, 1) in seen and ((codec, 1, 0, 0) in seen or codec == PCMU)
    assert {c for c, call, ulaw, _ in seen if ulaw} == {PCMU, BY_PT} and (PCMU, 1, 0, 0) not in seen


def test_known_answers(answers):
    cases, laws, valid = answers
    #        codec      arrived pt   call ulaw refused
    known = [(REFERENCE, 1, 8, 1, 0, 0), (REFERENCE, 1, 0, 1, 0, 0), (REFERENCE, 1, 101, 0, 0, 1), (REFERENCE, 1, 97, 0, 0, 1), (REFERENCE, 0, 8, 0, 0, 0),
             (PCMA, 1, 8, 1, 0, 0), (PCMA, 1, 0, 0, 0, 1), (PCMA, 1, 101, 0, 0, 1), (PCMA, 0, 0, 0, 0, 0),
             (PCMU, 1, 0, 1, 1, 0), (PCMU, 1, 8, 0, 0, 1), (PCMU, 1, 97, 0, 0, 1), (PCMU, 0, 0, 0, 0, 0),
             (BY_PT, 1, 8, 1, 0, 0), (BY_PT, 1, 0, 1, 1, 0), (BY_PT, 1, 96, 0, 0, 1), (BY_PT, 0, 0, 0, 0, 0)]
    for codec, arrived, pt, call, ulaw, refused in known:
        assert cases[(codec, arrived, pt)] == (call, ulaw, refused), (codec, arrived, pt)
    assert laws == {LAW_A: 8, LAW_U: 0} == {law: out_pt(law) for law in (LAW_A, LAW_U)}
    assert valid == {-1: (0, 0), 0: (1, 1), 1: (1, 1), 2: (1, 0), 3: (1, 0), 4: (0, 0)}


def test_the_default_is_the_length_rule_of_the_oracles_ingest(answers, oracle_port):
    cases, _, _ = answers
    ing = L._fn(oracle_port, "orc_rtp_ingest", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    row, pcm = np.zeros(172, np.uint8), np.zeros(160, np.int16)
    for marker in (0, 0x80):
        for pt in range(128):
            row[1] = marker | pt
            size = ing(row.ctypes.data, pcm.ctypes.data, None)
            assert size in (0, 320)
            assert cases[(REFERENCE, 1, pt)] == (int(size == 320), 0, int(size == 0)), pt
