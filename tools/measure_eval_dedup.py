#!/usr/bin/env python3
"""Request dedup (engine.SelfPlayEngine(eval_dedup=True)): the merged share of requests and what it buys.

    python tools/measure_eval_dedup.py a --parent-tree <dir> --preset cfg1 --weights peaked --repeats 3 --out profiles/<name>.json
    python tools/measure_eval_dedup.py steps --dedup on|off   (a short eager run: take `rocprofv3 --kernel-trace --stats` around
        `python tools/measure_eval_dedup.py --child '{"mode": "steps", "preset": "cfg1", "dedup": "on", "steps": 400}'`)

Mode a is measure_common.off_on_child per run: `off` on a built checkout of the parent commit, `on` on this tree, alternated, each
in a fresh child under `timeout -k`; the first failing run ends it.  Complete games from a lockstep start (games/hour, rows per
step, the merged share, a hash of the records: `record_hashes_equal_in_every_pair` must be true) and replayed steps from a
staggered, refilling start (us per step, step_* figures over the timed steps).  The margin is the spread of the parent's own runs.
"""
import argparse
import json
import sys

import measure_common as mc
from measure_common import PRESETS


def figures(st, steps):
    req, merged = st.get("eval_dedup_requests", 0), st.get("eval_dedup_merged", 0)
    return {"rows_per_step": round(st["rows_evaluated"] / steps, 3), "requests": req, "merged": merged,
            "collisions": st.get("eval_dedup_collisions", 0), "mismatches": st.get("eval_dedup_mismatches", 0),
            "merged_share": round(merged / req, 5) if req else 0.0}


OPT = dict(job_key="dedup", config_key="eval_dedup", engine_kw="eval_dedup", extra=figures)


def summarise(out, job, row):
    hashes = [r["record_hash"] for r in out["runs"]]
    out["record_hashes_equal_in_every_pair"] = all(a == b for a, b in zip(hashes[0::2], hashes[1::2]))
    mc.parent_this_summary(out, ("games_per_hour", "step_us_mean", "step_us_median", "rows_per_step", "step_rows_per_step"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("a", "steps"), nargs="?", default="a")
    ap.add_argument("--preset", choices=sorted(PRESETS), default="cfg1")
    ap.add_argument("--weights", choices=sorted(mc.GAINS), default="peaked", help="mode a")
    ap.add_argument("--parent-tree", default=None, help="mode a: a built checkout of the parent commit, for the `off` runs")
    ap.add_argument("--repeats", type=int, default=3, help="mode a: parent/this pairs")
    ap.add_argument("--step-steps", type=int, default=2000, help="mode a: replayed steps timed per run")
    ap.add_argument("--dedup", choices=("on", "off"), default="on", help="mode steps")
    ap.add_argument("--steps", type=int, default=400, help="mode steps")
    args = mc.parse_args(ap, 400, lambda job: (mc.off_on_child if job["mode"] == "a" else mc.off_on_steps_child)(
        job, PRESETS[job["preset"]], OPT))
    out = {"tool": "tools/measure_eval_dedup.py", "mode": args.mode, "preset": dict(PRESETS[args.preset], name=args.preset),
           "weights": args.weights, "runs": []}
    jobs = [dict(mode="steps", tree="this", tree_path=mc.ROOT, preset=args.preset, dedup=args.dedup, steps=args.steps)]
    if args.mode == "a":
        jobs = mc.off_on_jobs(args.parent_tree, args.repeats, "dedup", mode="a", preset=args.preset, weights=args.weights,
                              step_steps=args.step_steps)
    ok = mc.run_children(__file__, jobs, args.timeout, out, args.out, cwd=lambda job: job["tree_path"],
                         after_each=summarise if args.mode == "a" else None)
    print(json.dumps(out.get("summary", {}), indent=1))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
