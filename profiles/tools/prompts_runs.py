#!/usr/bin/env python3
"""profiles/bridge/bridge_prompts_bench.json from single runs of `tools_dev/bridge_bench.py --prompts N --out FILE`.

    python profiles/tools/prompts_runs.py --parent parent_1.json parent_2.json ... --this this_1.json this_2.json ... --out profiles/bridge/bridge_prompts_bench.json

--parent: runs made with the parent commit's library in WMIX_AMD_LIB (it has no prompts, so the tool measures "no store" alone);
--this: runs of this tree's library (no store, a store nobody plays from, N legs playing), one process per file.  Per side: the run
medians, their median, smallest and largest; the runs themselves go along as they were written."""
import argparse
import json
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", nargs="+", required=True)
    ap.add_argument("--this", nargs="+", required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    runs = {"parent": [json.load(open(f)) for f in args.parent], "this": [json.load(open(f)) for f in args.this]}
    summary = {}
    for name, kind, side in (("parent_library", "parent", "no_store"), ("no_store", "this", "no_store"),
                             ("store_nobody_playing", "this", "store_idle"), ("every_leg_playing", "this", "playing")):
        v = [r["prompts"]["ms_per_tick_" + side]["median_ms"] for r in runs[kind]]
        summary[name] = {"run_medians_ms": v, "median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
    first = runs["this"][0]
    out = {"tool": "profiles/tools/prompts_runs.py over single runs of tools_dev/bridge_bench.py --prompts %d, one process per run; the "
                   "parent's library through WMIX_AMD_LIB" % first["prompts"]["legs_asked_to_play"],
           "device": first["device"], "legs": first["prompts"]["legs"], "reps": first["reps"], "summary": summary,
           "hbm_bytes_per_playing_leg_and_tick": first["prompts"]["hbm_bytes_per_playing_leg_and_tick"],
           "runs": {k: [r["prompts"] for r in v] for k, v in runs.items()}}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
