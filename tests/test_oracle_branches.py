"""Which data-dependent branches of the oracle do the suite's inputs take?  A guard that stays.

The kernels are held bit for bit to oracle/orc_*.c and the oracle to the real reference -- where the test signals go.  This test
runs, in a fresh child process with the coverage build of the oracle (WMIX_ORACLE_COV=1, oracle/Makefile `cov`), the catalogue of
tests/branch_inputs.py plus the suite's generators that are importable without a GPU (the make_*_golden.py case inputs,
extreme_signals, _edge_signals, the perfect echoes and the tones), reads the counters with tools_dev/oracle_branches.py and asserts
  (a) every outcome a catalogue entry claims is taken by that entry,
  (b) the set never taken EQUALS tests/golden/oracle_unreached.json, both ways: an unlisted untaken outcome fails, a listed one that is
      taken fails as stale,
  (c) the coverage build computes what the ordinary port computes on every catalogue entry.
gcov ships with the gcc the oracle needs: a missing gcov fails, it does not skip.

Measured: 33 s for the whole file on an 8-core x86-64 host (the child 30 s: 23 catalogue entries 5 s, the replay of the existing
generators 24 s, 24 gcov passes 1 s), against 25 s for the replay alone.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
UNREACHED = os.path.join(GOLDEN, "oracle_unreached.json")
CLASSES = ("config", "guard", "driver", "open")


def replay_existing(L, lib):
    """What the GPU parity tests feed the oracle, as far as it is importable without a GPU."""
    for p in (ROOT, HERE, GOLDEN):
        if p not in sys.path:
            sys.path.insert(0, p)
    from make_aec_golden import AEC_CASES, CHAIN_CASES, aec_input
    from make_aecm_golden import AECM_CASES, aecm_case_input
    from make_ns_golden import NS_CASES, ns_case_input
    from make_nsx_golden import NSX_CASES, nsx_case_input
    from make_vadagc_golden import AGC_CASES, VAD_CASES, agc_input, agc_pkg, vad_input, vad_pkg
    from test_edges_gpu import _edge_signals
    from test_extremes_gpu import extreme_signals
    for chn, freq, nf in NS_CASES:
        L.run_ns(lib, chn, freq, ns_case_input(chn, freq, nf), freq // 100, prefix="orc")
    for chn, freq, nf, amp in NSX_CASES:
        L.run_nsx(lib, chn, freq, nsx_case_input(chn, freq, nf, amp), freq // 100, prefix="orc")
    for chn, freq, ims, delay, n in AEC_CASES:
        far, near = aec_input(chn, freq, ims, n)
        L.run_aec(lib, chn, freq, ims, far, near, freq // 1000 * (20 if freq <= 8000 and ims % 20 == 0 else 10), delay, prefix="orc")
    for chn, freq, stages, n in CHAIN_CASES:
        far, near = aec_input(chn, freq, 10, n, seed=4100)
        L.run_chain(lib, chn, freq, 5, stages, far, near, freq // 100, prefix="orc")
    for chn, freq, iv, n, delay, split in AECM_CASES:
        far, near, pkt = aecm_case_input(chn, freq, iv, n)
        L.run_aecm(lib, chn, freq, iv, far, near, pkt, delay_ms=delay, split=split, prefix="orc")
    for chn, freq, ims, k in VAD_CASES:
        L.run_vad(lib, chn, freq, ims, vad_input(chn, freq, ims, k), k * vad_pkg(freq, ims), prefix="orc")
    for chn, freq, value in AGC_CASES:
        L.run_agc(lib, chn, freq, value, agc_input(chn, freq), agc_pkg(freq), prefix="orc")
    for freq in (8000, 16000, 32000):  # tests/test_extremes_gpu.py
        pkt, names, x = extreme_signals(freq, 500)
        for s in x:
            L.run_agc(lib, 1, freq, 5, s, pkt, prefix="orc")
            L.run_vad(lib, 1, freq, 10, s, pkt, prefix="orc")
            L.run_ns(lib, 1, freq, s, pkt, prefix="orc")
            if freq < 32000:
                L.run_nsx(lib, 1, freq, s, pkt, prefix="orc")
                for far_kind in ("loud", "square40", "min"):
                    far = x[names.index(far_kind)]
                    L.run_aecm(lib, 1, freq, 10, far, s, pkt, prefix="orc")
                    L.run_aec(lib, 1, freq, 10, far, s, pkt, prefix="orc")
        for value in (0, 1, 30, 90) if freq == 16000 else ():
            for s in x[:, : 400 * pkt]:
                L.run_agc(lib, 1, freq, value, s, pkt, prefix="orc")
    for freq in (8000, 16000):
        pkt, n = freq // 100, 900  # the perfect echoes of test_echo_cancellers_on_perfect_echoes
        rng = np.random.default_rng(21)
        far = rng.integers(-20000, 20001, n * pkt).astype(np.int16)
        for near in (far, -far, np.roll(far, 3), far // 2, np.zeros_like(far), np.roll(far, 40) // 4 + rng.integers(-3, 4, far.size).astype(np.int16)):
            L.run_aec(lib, 1, freq, 10, far, near, pkt, prefix="orc")
            L.run_aecm(lib, 1, freq, 10, far, near, pkt, prefix="orc")
        far, near = _edge_signals(freq, 3000)  # tests/test_edges_gpu.py
        for s in near:
            L.run_chain(lib, 1, freq, 5, 15, far, s, pkt, prefix="orc")
    for freq in (8000, 16000, 32000):  # the tones and click trains of test_noise_suppressors_on_tones_and_trains
        pkt, n = freq // 100, 600
        t = np.arange(n * pkt)
        fs = min(freq, 16000)
        rng = np.random.default_rng(4)
        for s in (np.round(12000 * np.sin(2 * np.pi * t * (16 * fs / 256) / freq)), np.round(12000 * np.sin(2 * np.pi * t * (16.5 * fs / 256) / freq)),
                  np.round(9000 * np.sin(2 * np.pi * (100 + t * 3000.0 / t.size) * t / freq)), (t % (pkt if freq <= 16000 else pkt // 2) == 0) * 30000.0,
                  np.where((t // (pkt * 30)) % 2 == 0, rng.integers(-8000, 8001, t.size), 0)):
            L.run_ns(lib, 1, freq, s.astype(np.int16), pkt, prefix="orc")
            if freq < 32000:
                L.run_nsx(lib, 1, freq, s.astype(np.int16), pkt, prefix="orc")


def child(out_path):
    """Runs under WMIX_ORACLE_COV=1.  Per catalogue entry: its output's hash and the outcomes it alone was run for; then everything."""
    sys.path[:0] = [ROOT, HERE, os.path.join(ROOT, "tools_dev")]
    import branch_inputs as B
    import oracle_branches as T
    from oracle import loader as L
    lib = L.port()
    total, res = {}, {"entries": {}}

    def add(counts):
        for k, n in counts.items():
            total[k] = total.get(k, 0) + n

    for e in B.CATALOGUE:
        L.cov_reset()
        out, rcs = B.run(lib, e, "orc")
        L.cov_dump()
        counts = T.outcomes()
        add(counts)
        claimed = B.CLAIMS.get(e.name, [])
        res["entries"][e.name] = {"hash": hashlib.sha1(out.tobytes() + (b"" if rcs is None else rcs.tobytes())).hexdigest(),
                                  "missed_claims": [k for k in claimed if not counts.get(k)]}
    L.cov_reset()
    replay_existing(L, lib)
    L.cov_dump()
    add(T.outcomes())
    res["untaken"] = sorted(k for k, n in total.items() if n == 0)
    res["n_outcomes"] = len(total)
    with open(out_path, "w") as f:
        json.dump(res, f)


def test_allow_list_is_well_formed():
    with open(UNREACHED) as f:
        rows = json.load(f)
    head, rows = rows[0], rows[1:]
    assert "counts" in head
    keys = [r["key"] for r in rows]
    assert len(set(keys)) == len(keys)
    for r in rows:
        assert r["class"] in CLASSES and len(r["why"]) > 10, r
    counts = {}
    for r in rows:
        c = counts.setdefault(r["key"].split(" :: ")[0], dict.fromkeys(CLASSES, 0))
        c[r["class"]] += 1
    assert head["counts"] == counts


def test_catalogue_takes_what_it_claims_and_the_rest_is_listed(tmp_path, oracle_port):
    import branch_inputs as B
    from oracle import loader as L
    out = str(tmp_path / "cov.json")
    env = dict(os.environ, WMIX_ORACLE_COV="1")
    env.pop("WMIX_ORACLE_SAN", None)
    env.pop("GCOV_PREFIX", None)
    env.pop("GCOV_PREFIX_STRIP", None)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], check=True, env=env, cwd=ROOT)
    with open(out) as f:
        res = json.load(f)
    # (a)
    missed = {n: r["missed_claims"] for n, r in res["entries"].items() if r["missed_claims"]}
    assert not missed, "catalogue entries no longer take the outcomes they exist for: %r" % missed
    assert all(B.CLAIMS.get(e.name) for e in B.CATALOGUE), "an entry without a claim has no reason to be in the catalogue"
    # (b)
    with open(UNREACHED) as f:
        listed = {r["key"] for r in json.load(f)[1:]}
    untaken = set(res["untaken"])
    assert not untaken - listed, "untaken outcomes with neither an input nor a reason:\n" + "\n".join(sorted(untaken - listed))
    assert not listed - untaken, "stale allow-list rows (taken now, or the line changed):\n" + "\n".join(sorted(listed - untaken))
    # (c)
    for e in B.CATALOGUE:
        o, rcs = B.run(oracle_port, e, "orc")
        h = hashlib.sha1(o.tobytes() + (b"" if rcs is None else rcs.tobytes())).hexdigest()
        assert h == res["entries"][e.name]["hash"], "coverage build and port differ on " + e.name


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child(sys.argv[2])
