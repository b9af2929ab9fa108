#!/usr/bin/env python3
"""The proven-result search (engine.SelfPlayEngine(solver=True)) against the engine without it: what it decides and what it costs.
Complete games through run_games on peaked weights, off and on alternated with the same seed, each run in a fresh child process
under `timeout -k`; the first failing run ends the measurement.

    python tools/measure_solver.py games --preset standard_train --out profiles/r15_solver_standard_train.json
    python tools/measure_solver.py games --preset cfg1 --out profiles/r15_solver_cfg1_games.json
    python tools/measure_solver.py arena --preset standard_train --out profiles/r15_solver_arena.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_solver.py trace --solver 0
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_solver.py trace --solver 1
    python tools/measure_solver.py spread --stats off=<csv>,<csv>,<csv> on=<csv>,... parent=<csv>,... --out <json>

Presets: cfg1 = BASELINE configs[1] (1024 slots x 400 sims x 128x6, games_target 1024); standard_train = the reference's
standard_train preset (20 games x 200 sims x 128x6); small = 256 slots x 64 sims x 64x2 (a quick look).
Per run: games/hour, samples/hour, mean game length, the five solver counters (proven_nodes, proven_stops, proven_moves,
unspent_sims, removed_visits), terminal simulations per move and the samples marked reserved1.
`arena` plays solver-on against solver-off engines over the SAME two nets under paired openings (arena.play_arena, solver off and
on alternated, one seed): the result tables, the steps each arena took and the on-run's counters.
`trace` runs replayed steps at a preset from a staggered start for a kernel trace of k_select; `spread` reads the
`*_kernel_stats.csv` files of several such traces (this tree off and on, the parent commit's tree, whose plain instance is the
comparison) and writes k_select's mean time per launch of every run with each group's own run-to-run spread.
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
SOLVER_KEYS = ("proven_nodes", "proven_stops", "proven_moves", "unspent_sims", "removed_visits")


def _net(channels, blocks, seed=0):
    from xiangqi_alphazero_amd import model, weights
    net = model.XiangqiNet(channels, blocks)
    net.load_state_dict(weights.make_state_dict(channels, blocks, seed=seed, policy_gain=PEAKED_GAIN))
    return net


def child_games(job):
    import torch
    from xiangqi_alphazero_amd import selfplay
    p = PRESETS[job["preset"]]
    cfg = types.SimpleNamespace(num_simulations=p["sims"], c_puct=1.5, temperature_threshold=p["temperature_threshold"],
                                max_game_length=p["max_game_length"], random_opening_moves=p["random_opening_moves"],
                                enable_resign=True, resign_threshold=-0.9, resign_check_steps=5,
                                mcts_solver=job["solver"] == "on")               # through the config key, as a training loop sets it
    samples, results, st, elapsed = selfplay.run_games(_net(p["channels"], p["blocks"]), cfg, p["games"], "cuda", n_slots=p["slots"],
                                                       seed=11, poll_every=64 if p["slots"] < 64 else 256)
    torch.cuda.synchronize()
    moves = max(int(st["moves_played"]), 1)
    return {"preset": job["preset"], "solver": bool(st["solver"]), "path": st["path"], "launch": st["launch"],
            "games": int(len(results)), "samples": int(len(samples)), "wall_s": round(elapsed, 2),
            "games_per_hour": round(len(results) * 3600.0 / elapsed, 1), "samples_per_hour": round(len(samples) * 3600.0 / elapsed, 1),
            "steps": int(st["steps"]), "mean_plies": round(float(results["steps"].mean()), 2),
            **{k: int(st[k]) for k in SOLVER_KEYS}, "proven_samples": int((samples["reserved1"] == 1).sum()),
            "moves": int(st["moves_played"]), "sims": int(st["sims"]), "terminal_sims": int(st["terminal_sims"]),
            "terminal_sims_per_move": round(int(st["terminal_sims"]) / moves, 4),
            "draws": int((results["winner"] == 0).sum()), "red_wins": int((results["winner"] == 1).sum()),
            "black_wins": int((results["winner"] == -1).sum()), "overflow": int(st["overflow"])}


def child_arena(job):
    import torch
    from xiangqi_alphazero_amd import arena, evaluator
    p = PRESETS[job["preset"]]
    games = max(2, p["games"] - p["games"] % 2)
    en = evaluator.make_evaluator(_net(p["channels"], p["blocks"], seed=1), "cuda", "hip")[0]
    eo = evaluator.make_evaluator(_net(p["channels"], p["blocks"], seed=2), "cuda", "hip")[0]
    info = {}
    t0 = time.time()
    res = arena.play_arena(en, eo, games, p["sims"], p["max_game_length"], opening_plies=4, seed=17, info=info,
                           solver=job["solver"] == "on")
    torch.cuda.synchronize()
    st = info["stats"]
    stats = arena.pair_statistics(res["winner"])
    return {"preset": job["preset"], "solver": job["solver"] == "on", "games": games, "wall_s": round(time.time() - t0, 2),
            "steps": int(info["steps"]), "mean_plies": round(float(res["steps"].mean()), 2), "winners": res["winner"].astype(int).tolist(),
            "plies": res["steps"].astype(int).tolist(), "win_rate_new": stats["win_rate"], "win_rate_se": stats["win_rate_se"],
            **{k: int(st.get(k, 0)) for k in SOLVER_KEYS}, "sims": int(st["sims"]), "terminal_sims": int(st["terminal_sims"]),
            "overflow": int(st["overflow"])}


def trace(preset, solver, steps):
    import torch
    from xiangqi_alphazero_amd import engine, evaluator
    c = PRESETS[preset]
    ev = evaluator.make_evaluator(_net(c["channels"], c["blocks"]), "cuda", "hip")[0]
    cfg = engine.make_config(c["slots"], c["sims"], seed=5, start_stagger=True, max_out_samples=c["slots"] * 16)
    kw = {"solver": True} if solver else {}            # solver 0 also runs on a tree without the option (the parent commit's)
    eng = engine.SelfPlayEngine(cfg, evaluator=ev, **kw)
    assert eng.capture_step()
    t0 = time.time()
    for i in range(steps):
        eng.step()
        if i % 256 == 255:
            eng.drain_device()
    torch.cuda.synchronize()
    st = eng.stats()
    print(json.dumps({"preset": preset, "solver": bool(solver), "steps": eng.steps, "launch": eng.launch_mode,
                      "wall_s": round(time.time() - t0, 1), "moves": st["moves_played"], "sims": st["sims"],
                      "terminal_sims": st["terminal_sims"], **{k: st.get(k, 0) for k in SOLVER_KEYS}, "overflow": st["overflow"]}),
          flush=True)


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
    out = {"tool": "tools/measure_solver.py spread", "unit": "microseconds per k_select launch, mean of a run", "groups": {}}
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
    ap.add_argument("part", choices=["games", "arena", "trace", "spread"])
    ap.add_argument("--preset", choices=sorted(PRESETS), default="standard_train")
    ap.add_argument("--runs", choices=("off", "on"), nargs="*", default=["off", "on", "off", "on"])
    ap.add_argument("--solver", type=int, default=1, help="trace: 1 = the solver on, 0 = the engine without the option")
    ap.add_argument("--steps", type=int, default=700, help="trace: replayed steps")
    ap.add_argument("--stats", nargs="*", default=[], help="spread: name=<kernel_stats.csv>,<kernel_stats.csv>,... per group")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.part == "trace":
        trace(args.preset, args.solver, args.steps)
        return
    if args.part == "spread":
        spread(args.stats, args.out)
        return
    if args.child:
        job = json.loads(args.child)
        print("RESULT " + json.dumps(child_arena(job) if args.part == "arena" else child_games(job)), flush=True)
        return
    out = {"tool": f"tools/measure_solver.py {args.part}", "preset": dict(PRESETS[args.preset], name=args.preset), "weights": "peaked",
           "runs": []}
    for solver in args.runs:
        job = dict(preset=args.preset, solver=solver)
        t0 = time.time()
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), args.part, "--child", json.dumps(job)]
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
