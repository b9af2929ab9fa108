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
import csv
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAKED_GAIN = 8.0
PRESETS = {
    "cfg1": dict(slots=1024, games=1024, sims=400, channels=128, blocks=6, temperature_threshold=20, max_game_length=400,
                 random_opening_moves=8),
    "standard_train": dict(slots=20, games=20, sims=200, channels=128, blocks=6, temperature_threshold=20, max_game_length=300,
                           random_opening_moves=6),
    "small": dict(slots=256, games=256, sims=64, channels=64, blocks=2, temperature_threshold=20, max_game_length=120,
                  random_opening_moves=6),
}


def _net(channels, blocks):
    from xiangqi_alphazero_amd import model, weights
    net = model.XiangqiNet(channels, blocks)
    net.load_state_dict(weights.make_state_dict(channels, blocks, policy_gain=PEAKED_GAIN))
    return net


def child_games(job):
    import numpy as np
    import torch
    from xiangqi_alphazero_amd import engine, selfplay
    p = PRESETS[job["preset"]]
    cfg = types.SimpleNamespace(num_simulations=p["sims"], c_puct=1.5, temperature_threshold=p["temperature_threshold"],
                                max_game_length=p["max_game_length"], random_opening_moves=p["random_opening_moves"],
                                enable_resign=True, resign_threshold=-0.9, resign_check_steps=5,
                                perpetual_check_loses=job["rule"] == "on")       # through the config key, as a training loop sets it
    samples, results, st, elapsed = selfplay.run_games(_net(p["channels"], p["blocks"]), cfg, p["games"], "cuda", n_slots=p["slots"],
                                                       seed=11, poll_every=64 if p["slots"] < 64 else 256)
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
    import torch
    from xiangqi_alphazero_amd import engine, evaluator
    c = PRESETS[preset]
    ev = evaluator.make_evaluator(_net(c["channels"], c["blocks"]), "cuda", "hip")[0]
    cfg = engine.make_config(c["slots"], c["sims"], seed=5, start_stagger=True, max_out_samples=c["slots"] * 16)
    kw = {"perpetual_check": True} if rule else {}     # rule 0 also runs on a tree without the option (the parent commit's)
    eng = engine.SelfPlayEngine(cfg, evaluator=ev, **kw)
    assert eng.capture_step()
    t0 = time.time()
    for i in range(steps):
        eng.step()
        if i % 256 == 255:
            eng.drain_device()
    torch.cuda.synchronize()
    st = eng.stats()
    print(json.dumps({"preset": preset, "perpetual_check": bool(rule), "steps": eng.steps, "launch": eng.launch_mode,
                      "wall_s": round(time.time() - t0, 1), "moves": st["moves_played"], "sims": st["sims"],
                      "terminal_sims": st["terminal_sims"], "overflow": st["overflow"]}), flush=True)


def _k_select_mean_us(path):
    """Mean time per launch of the k_select instances in a rocprofv3 `*_kernel_stats.csv` (calls-weighted), in microseconds."""
    calls = total = 0
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "k_select" in row["Name"] and "k_select_multi" not in row["Name"]:
                calls += int(row["Calls"])
                total += float(row["TotalDurationNs"])
    return round(total / calls / 1000.0, 3) if calls else None


def spread(groups, out_path):
    out = {"tool": "tools/measure_perpetual_check.py spread", "unit": "microseconds per k_select launch, mean of a run", "groups": {}}
    for spec in groups:
        name, files = spec.split("=", 1)
        runs = [_k_select_mean_us(p) for p in files.split(",")]
        out["groups"][name] = {"runs": runs, "min": min(runs), "max": max(runs), "spread": round(max(runs) - min(runs), 3),
                               "mean": round(sum(runs) / len(runs), 3)}
    g = out["groups"]
    if "on" in g and "parent" in g:
        out["on_within_parent_spread"] = g["parent"]["min"] <= g["on"]["mean"] <= g["parent"]["max"]
    print(json.dumps(out, indent=1))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["games", "trace", "spread"])
    ap.add_argument("--preset", choices=sorted(PRESETS), default="standard_train")
    ap.add_argument("--rules", choices=("off", "on"), nargs="*", default=["off", "on", "off", "on"])
    ap.add_argument("--rule", type=int, default=1, help="trace: 1 = the rule on, 0 = the engine without the option")
    ap.add_argument("--steps", type=int, default=700, help="trace: replayed steps")
    ap.add_argument("--stats", nargs="*", default=[], help="spread: name=<kernel_stats.csv>,<kernel_stats.csv>,... per group")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.part == "trace":
        trace(args.preset, args.rule, args.steps)
        return
    if args.part == "spread":
        spread(args.stats, args.out)
        return
    if args.child:
        print("RESULT " + json.dumps(child_games(json.loads(args.child))), flush=True)
        return
    out = {"tool": "tools/measure_perpetual_check.py", "preset": dict(PRESETS[args.preset], name=args.preset), "weights": "peaked",
           "seed": 11, "runs": []}
    for rule in args.rules:
        job = dict(preset=args.preset, rule=rule)
        t0 = time.time()
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "games", "--child", json.dumps(job)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = next((l for l in r.stdout.splitlines() if l.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(r.stdout[-3000:], file=sys.stderr)
            print(f"child failed (exit {r.returncode}) on {job}: stopping", file=sys.stderr)
            out["failed"] = dict(job=job, exit=r.returncode)
            break
        row = json.loads(line[7:])
        row["child_wall_s"] = round(time.time() - t0, 1)
        print(json.dumps(row), flush=True)
        out["runs"].append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    sys.exit(1 if "failed" in out else 0)


if __name__ == "__main__":
    main()
