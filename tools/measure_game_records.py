#!/usr/bin/env python3
"""Game records (engine.SelfPlayEngine(record_games=True)) against the engine without them and against the parent commit: what
the option costs.  Complete games through run_games on peaked weights with one seed, the kinds of run alternated, each run in a
fresh child process under `timeout -k`; the first failing run ends the measurement.

    python tools/measure_game_records.py games --preset cfg1 --parent-tree <checkout of the parent commit, library built> \\
        --out profiles/r18_game_records_cfg1.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_game_records.py trace --records 0
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_game_records.py trace --records 1
    python tools/measure_game_records.py spread --stats off=<csv>,<csv>,<csv> on=<csv>,... parent=<csv>,... --out <json>

Presets: cfg1 = BASELINE configs[1] (1024 slots x 400 sims x 128x6, games_target 1024); small = 256 slots x 64 sims x 64x2 (a
quick look).  Kinds of run: `parent` (the parent commit's tree, given by --parent-tree: its own Python and its own library; it
has no option), `off` (this tree, the option off) and `on`.  Per run: games/hour, samples/hour, steps, mean game length, and for
`on` the records' own counts, the share of games each reason ended and the mean opening length -- the first figures the records
make available.  The summary gives every kind's runs with its own run-to-run spread and says whether `off` lies within the
parent's spread and `on` within it as well.
`trace` runs replayed steps at a preset from a staggered start for a kernel trace; `spread` reads the `*_kernel_stats.csv` files of
several such traces and writes the mean time per launch of k_select (and of k_flush_records, which only `on` launches) for every
run with each group's own spread.
"""
import argparse
import json
import os
import sys

import measure_common as mc
from measure_common import ROOT

PRESETS = {k: mc.PRESETS[k] for k in ("cfg1", "small")}


def child_games(job):
    import numpy as np
    import torch
    from xiangqi_alphazero_amd import selfplay
    p = PRESETS[job["preset"]]
    # through the config key, as a training loop sets it
    cfg = mc.selfplay_config(p, **({"record_games": True} if job["kind"] == "on" else {}))
    samples, results, st, elapsed = selfplay.run_games(mc.make_net(p["channels"], p["blocks"]), cfg, p["games"], "cuda",
                                                       n_slots=p["slots"], seed=11, poll_every=mc.poll_every(p))
    torch.cuda.synchronize()
    row = {"preset": job["preset"], "kind": job["kind"], "path": st["path"], "launch": st["launch"], "games": int(len(results)),
           "samples": int(len(samples)), "wall_s": round(elapsed, 2), "games_per_hour": round(len(results) * 3600.0 / elapsed, 1),
           "samples_per_hour": round(len(samples) * 3600.0 / elapsed, 1), "steps": int(st["steps"]),
           "mean_plies": round(float(results["steps"].mean()), 2), "moves": int(st["moves_played"]), "sims": int(st["sims"]),
           "overflow": int(st["overflow"])}
    if job["kind"] == "on":
        rec = st["game_records"]
        row.update(records=int(len(rec)), recorded=int(st["game_records_recorded"]), dropped=int(st["game_records_dropped"]),
                   mean_opening_plies=round(float(rec["opening_plies"].mean()), 3),
                   reasons={str(r): int((rec["reason"] == r).sum()) for r in (1, 2, 3, 4)},
                   moves_in_records=int(rec["n_moves"].astype(np.int64).sum()))
    return row


def trace(preset, records, steps):
    kw = {"record_games": True} if records else {}     # records 0 also runs on a tree without the option (the parent commit's)
    mc.trace(PRESETS[preset], steps, kw, lambda eng, st: {"preset": preset, "records": bool(records),
                                                          "games_finished": st["games_finished"]},
             drain=(lambda eng: eng.drain_games_device()) if records else None)


def spread(groups, out_path):
    out = {"tool": "tools/measure_game_records.py spread", "unit": "microseconds per launch, mean of a run",
           **mc.spread_groups(groups, {"k_select": ("k_select", ("k_select_multi",)), "k_flush_records": ("k_flush_records", ())},
                              kinds=("off", "on"))}
    print(json.dumps(out, indent=1))
    mc.save_json(out, out_path)


def summarise(out, job, row):
    s = out["summary"] = {kind: mc.group([r["games_per_hour"] for r in out["runs"] if r["kind"] == kind])
                          for kind in ("parent", "off", "on")}
    for kind in ("off", "on"):
        if s["parent"] and s[kind]:
            s[f"{kind}_within_parent_spread"] = mc.within_spread(s["parent"], s[kind])
            s[f"{kind}_over_parent_mean"] = round(s[kind]["mean"] / s["parent"]["mean"], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["games", "trace", "spread"])
    ap.add_argument("--preset", choices=sorted(PRESETS), default="cfg1")
    ap.add_argument("--runs", choices=("parent", "off", "on"), nargs="*", default=["parent", "off", "on"] * 3)
    ap.add_argument("--parent-tree", default=None, help="games: a checkout of the parent commit with its library built")
    ap.add_argument("--records", type=int, default=1, help="trace: 1 = game records on, 0 = the engine without the option")
    ap.add_argument("--steps", type=int, default=700, help="trace: replayed steps")
    ap.add_argument("--stats", nargs="*", default=[], help="spread: name=<kernel_stats.csv>,<kernel_stats.csv>,... per group")
    args = mc.parse_args(ap, 400)
    if args.part == "spread":
        spread(args.stats, args.out)
        return
    # a child of a `parent` run imports the parent commit's package: its Python goes with its library
    tree = json.loads(args.child).get("tree") if args.child else None
    sys.path.insert(0, tree or ROOT)
    if args.part == "trace":
        trace(args.preset, args.records, args.steps)
        return
    if args.child:
        mc.emit_result(child_games(json.loads(args.child)))
        return
    if "parent" in args.runs and not args.parent_tree:
        sys.exit("runs of kind `parent` need --parent-tree")
    out = {"tool": "tools/measure_game_records.py games", "preset": dict(PRESETS[args.preset], name=args.preset), "weights": "peaked",
           "runs": []}
    jobs = [dict(preset=args.preset, kind=kind, tree=os.path.abspath(args.parent_tree) if kind == "parent" else None)
            for kind in args.runs]
    ok = mc.run_children(__file__, jobs, args.timeout, out, args.out, argv=lambda job: ["games"],
                         cwd=lambda job: job["tree"] or ROOT, after_each=summarise)
    print(json.dumps(out.get("summary", {}), indent=1))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
