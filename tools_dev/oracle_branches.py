#!/usr/bin/env python3
"""tools_dev/oracle_branches.py -- TEST INFRASTRUCTURE ONLY.

Which branch outcomes of the oracle restatement (oracle/orc_*.c) did a run take?  Reads the counters the coverage build
(oracle/Makefile `cov`, loaded with WMIX_ORACLE_COV=1) left in oracle/build/cov/ -- or in any directories given, whose counts are
added -- through `gcov -b -c -j`, and prints per file the outcomes never taken.

An outcome is keyed by   file :: function :: stripped text of the source line :: b<index of the branch on that line>
(" @k" after the text for the k-th further line of the function with the same text), never by line number: an edit elsewhere in the
file leaves the keys as they are.  Left out by rule, not by list: functions named orc_run_* (whole-run drivers of the tests),
*_probe (state probes) and, inside functions named *_init, the returns for a failed allocation or a failed inner *_init.

    python tools_dev/oracle_branches.py                      # the six stateful stages, from oracle/build/cov
    python tools_dev/oracle_branches.py --all DIR [DIR ...]   # every orc_*.c, counters of several runs added
    python tools_dev/oracle_branches.py --json                # machine-readable: {key: count}
"""
import argparse
import gzip
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
COV_DIR = os.path.join(ORACLE, "build", "cov")
STAGES = ("orc_ns.c", "orc_nsx.c", "orc_aec.c", "orc_aecm.c", "orc_agc.c", "orc_vad.c")

_INIT_FAIL = re.compile(r"^if \(!\w+\) return NULL;|^if \(\w*_init\(.*\) != 0\)")


def left_out(function, text):
    """The rule of the module docstring."""
    if function.startswith("orc_run_") or function.endswith("_probe"):
        return True
    return function.endswith("_init") and bool(_INIT_FAIL.match(text))


def _gcov_json(gcda, notes_dir):
    """gcov's JSON for one counter file.  The notes (.gcno) lie in notes_dir; gcov wants both side by side."""
    if shutil.which("gcov") is None:
        raise RuntimeError("gcov not found (it ships with the gcc the oracle needs)")
    with tempfile.TemporaryDirectory() as t:
        base = os.path.basename(gcda)[:-5]
        shutil.copy(gcda, t)
        shutil.copy(os.path.join(notes_dir, base + ".gcno"), t)
        subprocess.run(["gcov", "-b", "-c", "-j", base + ".gcda"], cwd=t, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        with gzip.open(os.path.join(t, base + ".gcov.json.gz"), "rt") as f:
            return json.load(f)


def outcomes(dirs=(COV_DIR,), files=STAGES, notes_dir=COV_DIR):
    """{key: times taken} over the counter files of `dirs` (added up), for the sources named in `files` (None: all)."""
    res = {}
    for d in dirs:
        for name in sorted(os.listdir(d)):
            if not name.endswith(".gcda") or (files is not None and name[:-5] + ".c" not in files):
                continue
            for fobj in _gcov_json(os.path.join(d, name), notes_dir)["files"]:
                src = os.path.basename(fobj["file"])
                if src != name[:-5] + ".c":
                    continue  # a header's inline functions
                with open(os.path.join(ORACLE, src)) as f:
                    text = [ln.strip() for ln in f]
                seen = {}
                for ln in sorted(fobj["lines"], key=lambda x: x["line_number"]):
                    if not ln.get("branches"):
                        continue
                    fn, tx = ln.get("function_name", "?"), text[ln["line_number"] - 1]
                    k = seen.get((fn, tx), 0)
                    seen[(fn, tx)] = k + 1
                    if left_out(fn, tx):
                        continue
                    for i, b in enumerate(ln["branches"]):
                        key = "%s :: %s :: %s%s :: b%d" % (src, fn, tx, " @%d" % k if k else "", i)
                        res[key] = res.get(key, 0) + int(b["count"])
    return res


def table(res):
    """per file: (outcomes, taken at least once, never taken)"""
    t = {}
    for key, n in res.items():
        row = t.setdefault(key.split(" :: ")[0], [0, 0, 0])
        row[0] += 1
        row[1 if n else 2] += 1
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[1])
    ap.add_argument("dirs", nargs="*", default=[COV_DIR], help="directories with *.gcda (default oracle/build/cov)")
    ap.add_argument("--all", action="store_true", help="every orc_*.c, not only the six stateful stages")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    res = outcomes(a.dirs, None if a.all else STAGES)
    if a.json:
        json.dump(res, sys.stdout, indent=0, sort_keys=True)
        return 0
    print("| file | outcomes | taken >= once | never taken |\n|---|---|---|---|")
    for f, (n, hit, miss) in sorted(table(res).items()):
        print("| `%s` | %d | %d %% | %d |" % (f, n, round(100.0 * hit / n), miss))
    for key in sorted(k for k, n in res.items() if n == 0):
        print(key)
    return 0


if __name__ == "__main__":
    sys.exit(main())
