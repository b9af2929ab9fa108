#!/usr/bin/env python3
"""The perpetual-check rule (engine.SelfPlayEngine(perpetual_check=True)) against the engine without it: how often it decides a
self-play game, and what it costs.  Complete games through run_games on peaked weights, off and on alternated with the same seed,
each run in a fresh child process under `timeout -k`; the first failing run ends the measurement.

    python tools/measure_perpetual_check.py games --preset standard_train --out profiles/r14_perpetual_check_standard_train.json
    python tools/measure_perpetual_check.py games --preset cfg1 --out profiles/r14_perpetual_check_cfg1_games.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_perpetual_check.py trace --rule 0
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_perpetual_check.py trace --rule 1
    python tools/measure_perpetual_check.py spread --stats off=<csv>,<csv>,<csv> on=<csv>,... parent=<csv>,... --out <json>

Presets: cfg1 = BASELINE configs[1] (1024 slots x 400 sims x 128x6, games_target 1024); standard_train = the reference's
standard_train preset (20 games x 200 sims x 128x6); small = 256 slots x 64 sims x 64x2 (a quick look).
Per run: games/hour, samples/hour, mean plies, and the endings: the results' reasons (1 rules, 2 max_game_length, 3 resign,
4 repetition decided by the rule) and the draws among the rules endings -- with the rule off an upper bound on the games the rule
could decide (a rules draw is a repetition, 120 no-capture plies or an even ply-200 count).
`trace` runs replayed steps at a preset from a staggered start for a kernel trace of k_select; `spread` reads the
`*_kernel_stats.csv` files of several such traces (this tree off and on, the parent commit's tree) and writes k_select's mean
time per launch of every run with each group's own run-to-run spread.
"""
import argparse
import json
import sys

import measure_common as mc
from measure_common import PRESETS

sys.path.insert(0, mc.ROOT)


def child_games(job):
    import numpy as np
    import torch
    from xiangqi_alphazero_amd import engine, selfplay
    p = PRESETS[job["preset"]]
    cfg = mc.selfplay_config(p, perpetual_check_loses=job["rule"] == "on")     # through the config key, as a training loop sets it
    samples, results, st, elapsed = selfplay.run_games(mc.make_net(p["channels"], p["blocks"]), cfg, p["games"], "cuda",
                                                       n_slots=p["slots"], seed=11, poll_every=mc.poll_every(p))
    torch.cuda.synchronize()
    n = max(len(results), 1)
    reasons = {str(r): int((results["reason"] == r).sum()) for r in (1, 2, 3, 4)}
    rules = np.isin(results["reason"], engine.RULES_REASONS)
    return {"preset": job["preset"], "rule": job["rule"], "perpetual_check": bool(st["perpetual_check"]), "path": st["path"],
            "launch": st["launch"], "games": int(len(results)), "samples": int(len(samples)), "wall_s": round(elapsed, 2),
            "games_per_hour": round(len(results) * 3600.0 / elapsed, 1), "samples_per_hour": round(len(samples) * 3600.0 / elapsed, 1),
            "steps": int(st["steps"]), "mean_plies": round(float(results["steps"].mean()), 2), "reasons": reasons,
            "share_by_reason": {k: round(v / n, 5) for k, v in reasons.items()},
            "perpetual_check_games": int(st["perpetual_check_games"]),
            "rules_draws": int((rules & (results["winner"] == 0)).sum()), "draws": int((results["winner"] == 0).sum()),
            "red_wins": int((results["winner"] == 1).sum()), "black_wins": int((results["winner"] == -1).sum()),
            "sims": int(st["sims"]), "terminal_sims": int(st["terminal_sims"]), "overflow": int(st["overflow"])}


def trace(preset, rule, steps):
    kw = {"perpetual_check": True} if rule else {}     # rule 0 also runs on a tree without the option (the parent commit's)
    mc.trace(PRESETS[preset], steps, kw, lambda eng, st: {"preset": preset, "perpetual_check": bool(rule),
                                                          "terminal_sims": st["terminal_sims"]})


def spread(groups, out_path):
    out = {"tool": "tools/measure_perpetual_check.py spread", "unit": "microseconds per k_select launch, mean of a run",
           **mc.spread_groups(groups, {"groups": ("k_select", ("k_select_multi",))})}
    print(json.dumps(out, indent=1))
    mc.save_json(out, out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["games", "trace", "spread"])
    ap.add_argument("--preset", choices=sorted(PRESETS), default="standard_train")
    ap.add_argument("--rules", choices=("off", "on"), nargs="*", default=["off", "on", "off", "on"])
    ap.add_argument("--rule", type=int, default=1, help="trace: 1 = the rule on, 0 = the engine without the option")
    ap.add_argument("--steps", type=int, default=700, help="trace: replayed steps")
    ap.add_argument("--stats", nargs="*", default=[], help="spread: name=<kernel_stats.csv>,<kernel_stats.csv>,... per group")
    args = mc.parse_args(ap, 400, child_games)
    if args.part == "trace":
        trace(args.preset, args.rule, args.steps)
        return
    if args.part == "spread":
        spread(args.stats, args.out)
        return
    out = {"tool": "tools/measure_perpetual_check.py", "preset": dict(PRESETS[args.preset], name=args.preset), "weights": "peaked",
           "seed": 11, "runs": []}
    jobs = [dict(preset=args.preset, rule=rule) for rule in args.rules]
    sys.exit(0 if mc.run_children(__file__, jobs, args.timeout, out, args.out, argv=lambda job: ["games"]) else 1)


if __name__ == "__main__":
    main()
