#!/usr/bin/env python3
"""profiles/bridge/bridge_record_bench.json from single runs of `tools_dev/bridge_bench.py --record N [--record-format CHN,FREQ] --out FILE`.

    python profiles/tools/record_runs.py --parent parent_1.json ... --alone alone_1.json ... --this this_1.json ... --out profiles/bridge/bridge_record_bench.json

--parent: runs made with the parent commit's library in WMIX_AMD_LIB (it has no recording store, so the tool measures "no store" alone);
--alone: runs of this tree's library with --record-alone: the same program as the parent's runs, so that the two are comparable;
--this: runs of this tree's library (no store, a store of N taps none of which runs, the N taps running), one process per file, grouped
by the store's format.  Per side and clock (the resident step in device time, the handle with 3 slots in wall time): the run medians,
their median, smallest and largest, and for the recording side the difference to the same run's side without a store and to the same handle with its taps stopped.  The runs
themselves go along as they were written."""
import argparse
import json
import statistics


def side(runs, key):
    v = [r["record"][key]["median_ms"] for r in runs]
    return {"run_medians_ms": v, "median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", nargs="+", required=True)
    ap.add_argument("--alone", nargs="+", required=True)
    ap.add_argument("--this", nargs="+", required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    parent, alone, this = ([json.load(open(f)) for f in files] for files in (args.parent, args.alone, args.this))
    summary = {"parent_library": {clock: side(parent, clock + "_ms_per_tick_no_store") for clock in ("resident", "handle_wall")},
               "this_library_no_store_alone": {clock: side(alone, clock + "_ms_per_tick_no_store") for clock in ("resident", "handle_wall")}}
    formats = sorted({tuple(r["record"]["format"]) for r in this})
    for fmt in formats:
        runs = [r for r in this if tuple(r["record"]["format"]) == fmt]
        rec = runs[0]["record"]
        s = {"taps": rec["taps"], "row_bytes": rec["row_bytes"], "d2h_bytes_per_tick_datagrams": rec["d2h_bytes_per_tick_datagrams"],
             "d2h_bytes_per_tick_added_while_recording": rec["d2h_bytes_per_tick_added_while_recording"]}
        for clock in ("resident", "handle_wall"):
            for name in ("no_store", "store_idle", "recording"):
                s["%s_%s" % (clock, name)] = side(runs, "%s_ms_per_tick_%s" % (clock, name))
            d = [r["record"][clock + "_ms_per_tick_recording"]["median_ms"] - r["record"][clock + "_ms_per_tick_no_store"]["median_ms"] for r in runs]
            s[clock + "_recording_minus_no_store_ms"] = {"per_run": [round(x, 5) for x in d], "median_ms": round(statistics.median(d), 5)}
            d = [r["record"][clock + "_ms_per_tick_recording"]["median_ms"] - r["record"][clock + "_ms_per_tick_store_idle"]["median_ms"] for r in runs]
            s[clock + "_recording_minus_store_idle_same_handle_ms"] = {"per_run": [round(x, 5) for x in d], "median_ms": round(statistics.median(d), 5)}
        summary["%dx%d" % fmt] = s
    first = this[0]
    out = {"tool": "profiles/tools/record_runs.py over single runs of tools_dev/bridge_bench.py --record %d, one process per run; the parent's "
                   "library through WMIX_AMD_LIB" % first["record"]["taps"],
           "device": first["device"], "legs": first["record"]["legs"], "reps": first["reps"], "summary": summary,
           "runs": {"parent": [r["record"] for r in parent], "alone": [r["record"] for r in alone], "this": [r["record"] for r in this]}}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
