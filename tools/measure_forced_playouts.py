#!/usr/bin/env python3
"""Forced playouts and policy target pruning (engine.SelfPlayEngine(forced_playouts=k)) against the engine without them: complete
games through run_games, off and on alternated, each run in a fresh child process under `timeout -k`; the first failing run ends
the measurement.

    python tools/measure_forced_playouts.py games --preset cfg1 --out profiles/r10_forced_playouts_cfg1_games.json
    python tools/measure_forced_playouts.py games --preset standard_train --out profiles/r10_forced_playouts_standard_train.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_forced_playouts.py trace --forced 0
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_forced_playouts.py trace --forced 2

Presets: cfg1 = BASELINE configs[1] (1024 slots x 400 sims x 128x6, games_target 1024); standard_train = the reference's
standard_train preset (20 games x 200 sims x 128x6); small = 256 slots x 64 sims x 64x2 (a quick look).  k = 2.  Weights: random
init, and peaked (make_state_dict(policy_gain=8)).  Modes: off, on, and both again with the playout cap (p = 0.25, S_fast = S / 4).
Per run: games/hour, samples/hour, steps, rows evaluated, mean plies, forced simulations per full move, the pruned share of the
samples' visits, pruned_visits / (S x full moves), and the pruned share of the visited children.  Whether training gains from
the option is not measured here.
`trace` runs replayed steps at a preset from a staggered start for a kernel trace of k_select: once with --forced 0 (the
instance the same engine launches without the option: the comparison figure) and once with --forced 2.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GAINS = {"random": 1.0, "peaked": 8.0}
PRESETS = {
    "cfg1": dict(slots=1024, games=1024, sims=400, channels=128, blocks=6, temperature_threshold=20, max_game_length=400,
                 random_opening_moves=8),
    "standard_train": dict(slots=20, games=20, sims=200, channels=128, blocks=6, temperature_threshold=20, max_game_length=300,
                           random_opening_moves=6),
    "small": dict(slots=256, games=256, sims=64, channels=64, blocks=2, temperature_threshold=20, max_game_length=120,
                  random_opening_moves=6),
}
MODES = ("off", "on", "cap", "cap+on")
K_FORCED, CAP_PROB = 2.0, 0.25


def _net(channels, blocks, gain):
    from xiangqi_alphazero_amd import model, weights
    net = model.XiangqiNet(channels, blocks)
    net.load_state_dict(weights.make_state_dict(channels, blocks, policy_gain=gain))
    return net


def child_games(job):
    import numpy as np
    import torch
    from xiangqi_alphazero_amd import selfplay
    p = PRESETS[job["preset"]]
    S = p["sims"]
    cfg = types.SimpleNamespace(num_simulations=S, c_puct=1.5, temperature_threshold=p["temperature_threshold"],
                                max_game_length=p["max_game_length"], random_opening_moves=p["random_opening_moves"],
                                enable_resign=True, resign_threshold=-0.9, resign_check_steps=5)
    cap = (CAP_PROB, max(1, S // 4)) if job["mode"].startswith("cap") else None
    forced = K_FORCED if job["mode"].endswith("on") else None
    samples, results, st, elapsed = selfplay.run_games(_net(p["channels"], p["blocks"], GAINS[job["weights"]]), cfg, p["games"],
                                                       "cuda", n_slots=p["slots"], seed=11, poll_every=64 if p["slots"] < 64 else 256,
                                                       playout_cap=cap, forced_playouts=forced)
    torch.cuda.synchronize()
    moves = int(st["moves_played"])
    full = moves - int(st["fast_moves"])
    visits = samples["visits"].astype(np.int64) if len(samples) else np.zeros((0, 1), np.int64)
    kept_children = int((visits > 0).sum())
    return {"preset": job["preset"], "weights": job["weights"], "mode": job["mode"], "k": forced, "playout_cap": cap,
            "path": st["path"], "launch": st["launch"], "games": int(len(results)), "samples": int(len(samples)),
            "wall_s": round(elapsed, 2), "games_per_hour": round(len(results) * 3600.0 / elapsed, 1),
            "samples_per_hour": round(len(samples) * 3600.0 / elapsed, 1), "steps": int(st["steps"]),
            "steps_per_game": round(st["steps"] / max(len(results), 1), 2), "rows_evaluated": int(st["rows_evaluated"]),
            "mean_plies": round(float(results["steps"].mean()), 2), "moves": moves, "full_moves": full,
            "fast_moves": int(st["fast_moves"]), "sims": int(st["sims"]), "forced_sims": int(st["forced_sims"]),
            "pruned_visits": int(st["pruned_visits"]), "pruned_children": int(st["pruned_children"]),
            "forced_sims_per_full_move": round(st["forced_sims"] / full, 3) if full else 0.0,
            "pruned_visit_share": round(st["pruned_visits"] / (S * full), 5) if full else 0.0,
            "pruned_share_of_visited_children": round(st["pruned_children"] / max(1, kept_children + st["pruned_children"]), 5),
            "sample_visits_add_up": int(visits.sum()) == S * int(len(samples)) - int(st["pruned_visits"]),
            "samples_equal_full_moves": int(len(samples)) == full, "resigns": int(st["resigns"]), "overflow": int(st["overflow"])}


def trace(preset, forced, steps, with_cap):
    import torch
    from xiangqi_alphazero_amd import engine, evaluator
    c = PRESETS[preset]
    ev = evaluator.make_evaluator(_net(c["channels"], c["blocks"], GAINS["peaked"]), "cuda", "hip")[0]
    cfg = engine.make_config(c["slots"], c["sims"], seed=5, start_stagger=True, max_out_samples=c["slots"] * 16)
    eng = engine.SelfPlayEngine(cfg, evaluator=ev, forced_playouts=forced if forced > 0 else None,
                                playout_cap=(CAP_PROB, max(1, c["sims"] // 4)) if with_cap else None)
    assert eng.capture_step()
    t0 = time.time()
    for i in range(steps):
        eng.step()
        if i % 256 == 255:
            eng.drain_device()
    torch.cuda.synchronize()
    st = eng.stats()
    print(json.dumps({"preset": preset, "k": eng.forced_playouts, "playout_cap": eng.playout_cap, "steps": eng.steps,
                      "launch": eng.launch_mode, "wall_s": round(time.time() - t0, 1), "moves": st["moves_played"],
                      "sims": st["sims"], "forced_sims": st["forced_sims"], "pruned_visits": st["pruned_visits"],
                      "overflow": st["overflow"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["games", "trace"])
    ap.add_argument("--preset", choices=sorted(PRESETS), default="cfg1")
    ap.add_argument("--weights", choices=sorted(GAINS), nargs="*", default=sorted(GAINS))
    ap.add_argument("--modes", choices=MODES, nargs="*", default=list(MODES))
    ap.add_argument("--forced", type=float, default=K_FORCED, help="trace: k, 0 = the engine without the option")
    ap.add_argument("--steps", type=int, default=700, help="trace: replayed steps")
    ap.add_argument("--cap", action="store_true", help="trace: with the playout cap")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.part == "trace":
        trace(args.preset, args.forced, args.steps, args.cap)
        return
    if args.child:
        print("RESULT " + json.dumps(child_games(json.loads(args.child))), flush=True)
        return
    p = PRESETS[args.preset]
    jobs = [dict(preset=args.preset, weights=w, mode=m) for w in args.weights for m in args.modes]   # off / on alternate
    out = {"tool": "tools/measure_forced_playouts.py", "preset": dict(p, name=args.preset), "k": K_FORCED, "runs": []}
    for job in jobs:
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
