#!/usr/bin/env python3
"""profiles/bridge/bridge_duck_bench.json from single runs of `tools_dev/bridge_bench.py --prompts N [--duck R] --out FILE`.

    python profiles/tools/duck_runs.py --parent parent_*.json --this this_*.json --duck duck_*.json --resources resources.json \
        --out profiles/bridge/bridge_duck_bench.json

--parent: runs made with the parent commit's library in WMIX_AMD_LIB (three sides: no store, a store nobody plays from, N legs playing);
--this: the same three sides on this tree's library; --duck: this tree's library with --duck R (the three sides and the two ducking
ones), one process per file, the three kinds of run taking turns.  Per side: the run medians, their median, smallest and largest; the
runs themselves go along as they were written.  --resources: the compiler's figures for the new and the touched kernels, copied in."""
import argparse
import json
import statistics

SIDES = ("no_store", "store_idle", "playing", "duck_all", "duck_one_per_conference")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", nargs="+", required=True)
    ap.add_argument("--this", nargs="+", required=True)
    ap.add_argument("--duck", nargs="+", required=True)
    ap.add_argument("--resources")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    runs = {k: [json.load(open(f)) for f in files] for k, files in (("parent", args.parent), ("this", args.this), ("duck", args.duck))}
    summary = {}
    for kind in runs:
        for side in SIDES:
            v = [r["prompts"]["ms_per_tick_" + side]["median_ms"] for r in runs[kind] if "ms_per_tick_" + side in r["prompts"]]
            if v:
                summary[kind + "/" + side] = {"run_medians_ms": v, "median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
    base = summary["duck/playing"]["median_ms"]
    added = {side: round(summary["duck/" + side]["median_ms"] - base, 5) for side in ("duck_all", "duck_one_per_conference")}
    first = runs["duck"][0]
    out = {"tool": "profiles/tools/duck_runs.py over single runs of tools_dev/bridge_bench.py --prompts %d [--duck %d], one process per run, the "
                   "kinds of run taking turns; the parent's library through WMIX_AMD_LIB" % (first["prompts"]["legs_asked_to_play"], first["prompts"]["reduce"]),
           "device": first["device"], "legs": first["prompts"]["legs"], "conferences": first["prompts"]["conferences"], "reps": first["reps"],
           "summary": summary, "ms_per_tick_added_over_reduce_0_in_the_same_process": added,
           "rings_ducked_at_the_end": first["prompts"]["rings_ducked_at_the_end"]}
    if args.resources:
        out["kernel_resources"] = json.load(open(args.resources))
    out["runs"] = {k: [r["prompts"] for r in v] for k, v in runs.items()}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["median_ms"], v["min_ms"], v["max_ms"]) for k, v in summary.items()}, indent=1))
    print(json.dumps(added))


if __name__ == "__main__":
    main()
