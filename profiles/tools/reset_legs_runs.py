#!/usr/bin/env python3
"""profiles/bridge/reset_legs_ab.json: what wmx_conf_reset_legs costs, the parent commit's library against this tree's.

    WMIX_AMD_LIB=parent.so python profiles/tools/reset_legs_runs.py --run parent_1.json      (one process per run, one sitting)
    python profiles/tools/reset_legs_runs.py --run this_1.json
    python profiles/tools/reset_legs_runs.py --parent parent_1.json parent_2.json --this this_1.json --out profiles/bridge/reset_legs_ab.json

--run: a handle of 4 096 legs in conferences of 8 with sequencing, concealment, DTMF, the gate and talker selection on, three ticks so
that every state exists, then CALLS calls of wmx_conf_reset_legs per list length (8 and 512 legs, another window of legs every call).
Per call, from an idle stream: the host time of the call, and the time until the stream has completed what it queued.
The other form: per list length and clock the runs' medians, the parent's mean and two-run spread, and whether this library is slower
than that mean by more than the spread."""
import argparse
import json
import statistics
import sys
import time
import os

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
LEGS, CALLS, WARM, LISTS = 4096, 200, 10, (8, 512)


def run(out):
    import torch
    from wmix_amd._lib import LIB_PATH, check, lib
    from wmix_amd.conf import ConfBridge
    cb = ConfBridge(LEGS, 3, 3)
    cb.set_conferences([list(range(c, c + 8)) for c in range(0, LEGS, 8)])
    cb.sequence(True, 3)
    cb.conceal(True)
    cb.dtmf(True, suppress=True)
    cb.gate(True)
    cb.speakers(3)
    rng = np.random.default_rng(13)
    for t in range(3):  # one packet per leg and tick, in order
        k = cb.next_slot()
        cb.rows_in[k][:] = rng.integers(0, 256, cb.rows_in[k].shape, dtype=np.uint8)
        cb.rows_in[k][:, :, :12] = 0
        cb.rows_in[k][:, :, 0], cb.rows_in[k][:, :, 1], cb.rows_in[k][:, :, 3] = 0x80, 0x88, t
        cb.recv[k][:] = 0
        cb.recv[k][:, 0] = 172
        cb.submit()
        cb.wait(k)
    L, stream, res = lib(), cb._stream(), {}
    for n in LISTS:
        host, complete = [], []
        for i in range(WARM + CALLS):
            idx = ((np.arange(n) + i * n) % LEGS).astype(np.int32)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            check(L.wmx_conf_reset_legs(cb._h, idx.ctypes.data, n, stream), "wmx_conf_reset_legs")
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host.append((t1 - t0) * 1e3)
            complete.append((t2 - t0) * 1e3)
        res[str(n)] = {"host_ms": round(statistics.median(host[WARM:]), 5), "complete_ms": round(statistics.median(complete[WARM:]), 5),
                       "host_ms_p90": round(float(np.percentile(host[WARM:], 90)), 5), "complete_ms_p90": round(float(np.percentile(complete[WARM:], 90)), 5)}
    gate = cb.export_gate()
    assert (gate["reduce"] == 4).all() and not gate["voiced"].any()  # every leg has been reset
    cb.close()
    r = {"library": os.path.basename(os.path.dirname(LIB_PATH)) + "/" + os.path.basename(LIB_PATH), "device": torch.cuda.get_device_name(0),
         "legs": LEGS, "calls": CALLS, "unit": "median ms per call", "lists": res}
    with open(out, "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps(r))


def summarise(parent, this, out):
    parent, this = [json.load(open(f)) for f in parent], [json.load(open(f)) for f in this]
    s = {}
    for n in map(str, LISTS):
        for clock in ("host_ms", "complete_ms"):
            p, t = [r["lists"][n][clock] for r in parent], statistics.mean(r["lists"][n][clock] for r in this)
            mean, spread = statistics.mean(p), max(p) - min(p)
            s["%s_legs_%s" % (n, clock)] = {"parent_runs": p, "parent_mean": round(mean, 5), "parent_spread": round(spread, 5), "this": round(t, 5),
                                            "this_minus_mean": round(t - mean, 5), "not_slower_by_more_than_the_spread": bool(t - mean <= spread)}
    r = {"tool": "profiles/tools/reset_legs_runs.py, one process per run, one sitting: the parent's library twice, then this tree's",
         "device": this[0]["device"], "legs": LEGS, "calls": CALLS, "criterion": "the 8-leg list, both clocks", "summary": s,
         "runs": {"parent": parent, "this": this}}
    with open(out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
    print(json.dumps(s))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", default="")
    ap.add_argument("--parent", nargs="+")
    ap.add_argument("--this", nargs="+")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    run(args.run) if args.run else summarise(args.parent, args.this, args.out)
