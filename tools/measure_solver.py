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
import json
import sys
import time

import measure_common as mc
from measure_common import PRESETS

sys.path.insert(0, mc.ROOT)
SOLVER_KEYS = ("proven_nodes", "proven_stops", "proven_moves", "unspent_sims", "removed_visits")


def child_games(job):
    import torch
    from xiangqi_alphazero_amd import selfplay
    p = PRESETS[job["preset"]]
    cfg = mc.selfplay_config(p, mcts_solver=job["solver"] == "on")             # through the config key, as a training loop sets it
    samples, results, st, elapsed = selfplay.run_games(mc.make_net(p["channels"], p["blocks"]), cfg, p["games"], "cuda",
                                                       n_slots=p["slots"], seed=11, poll_every=mc.poll_every(p))
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
    en = evaluator.make_evaluator(mc.make_net(p["channels"], p["blocks"], seed=1), "cuda", "hip")[0]
    eo = evaluator.make_evaluator(mc.make_net(p["channels"], p["blocks"], seed=2), "cuda", "hip")[0]
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
    kw = {"solver": True} if solver else {}            # solver 0 also runs on a tree without the option (the parent commit's)
    mc.trace(PRESETS[preset], steps, kw, lambda eng, st: {"preset": preset, "solver": bool(solver),
                                                          "terminal_sims": st["terminal_sims"],
                                                          **{k: st.get(k, 0) for k in SOLVER_KEYS}})


def spread(groups, out_path):
    out = {"tool": "tools/measure_solver.py spread", "unit": "microseconds per k_select launch, mean of a run",
           **mc.spread_groups(groups, {"groups": ("k_select", ("k_select_multi",))})}
    print(json.dumps(out, indent=1))
    mc.save_json(out, out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["games", "arena", "trace", "spread"])
    ap.add_argument("--preset", choices=sorted(PRESETS), default="standard_train")
    ap.add_argument("--runs", choices=("off", "on"), nargs="*", default=["off", "on", "off", "on"])
    ap.add_argument("--solver", type=int, default=1, help="trace: 1 = the solver on, 0 = the engine without the option")
    ap.add_argument("--steps", type=int, default=700, help="trace: replayed steps")
    ap.add_argument("--stats", nargs="*", default=[], help="spread: name=<kernel_stats.csv>,<kernel_stats.csv>,... per group")
    args = mc.parse_args(ap, 400)
    if args.part == "trace":
        trace(args.preset, args.solver, args.steps)
        return
    if args.part == "spread":
        spread(args.stats, args.out)
        return
    if args.child:
        job = json.loads(args.child)
        mc.emit_result(child_arena(job) if args.part == "arena" else child_games(job))
        return
    out = {"tool": f"tools/measure_solver.py {args.part}", "preset": dict(PRESETS[args.preset], name=args.preset), "weights": "peaked",
           "runs": []}
    jobs = [dict(preset=args.preset, solver=solver) for solver in args.runs]
    sys.exit(0 if mc.run_children(__file__, jobs, args.timeout, out, args.out, argv=lambda job: [args.part]) else 1)


if __name__ == "__main__":
    main()
