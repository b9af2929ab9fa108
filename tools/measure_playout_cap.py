#!/usr/bin/env python3
"""Playout cap randomization (engine.SelfPlayEngine(playout_cap=(p, S_fast))) against the engine without it: complete games
through run_games, off and on alternated, each run in a fresh child process under `timeout -k`; the first failing run ends the
measurement.

    python tools/measure_playout_cap.py games --preset cfg1 --out profiles/r09_playout_cap_cfg1_games.json
    python tools/measure_playout_cap.py games --preset standard_train --out profiles/r09_playout_cap_standard_train.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_playout_cap.py trace

Presets: cfg1 = BASELINE configs[1] (1024 slots x 400 sims x 128x6, games_target 1024, cap p = 0.25, S_fast = 100);
standard_train = the reference's standard_train preset (20 games x 200 sims x 128x6, cap p = 0.25, S_fast = 50).  Weights: random
init, and peaked (make_state_dict(policy_gain=8)).  Modes: off, on, and both again with tree reuse.  Per run: games/hour,
SAMPLES/hour (the cap raises the first and lowers the second), steps, rows evaluated, mean plies, the fast share of the moves,
and steps per game beside the count the program controls, (p S + (1 - p) S_fast + 1) / (S + 1) of the cap-off figure without
reuse.  Whether training gains from the trade is not measured here.
`trace` runs replayed cap-on steps at configs[1] from a staggered start for a kernel trace of k_select / k_expand.
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
    "cfg1": dict(slots=1024, games=1024, sims=400, fast_sims=100, full_prob=0.25, channels=128, blocks=6,
                 temperature_threshold=20, max_game_length=400, random_opening_moves=8),
    "standard_train": dict(slots=20, games=20, sims=200, fast_sims=50, full_prob=0.25, channels=128, blocks=6,
                           temperature_threshold=20, max_game_length=300, random_opening_moves=6),
}
MODES = ("off", "on", "reuse", "reuse+on")
TRACE = dict(slots=1024, sims=400, fast_sims=100, full_prob=0.25, channels=128, blocks=6, steps=700)


def _net(channels, blocks, gain):
    from xiangqi_alphazero_amd import model, weights
    net = model.XiangqiNet(channels, blocks)
    net.load_state_dict(weights.make_state_dict(channels, blocks, policy_gain=gain))
    return net


def child_games(job):
    import torch
    from xiangqi_alphazero_amd import selfplay
    p = PRESETS[job["preset"]]
    cfg = types.SimpleNamespace(num_simulations=p["sims"], c_puct=1.5, temperature_threshold=p["temperature_threshold"],
                                max_game_length=p["max_game_length"], random_opening_moves=p["random_opening_moves"],
                                enable_resign=True, resign_threshold=-0.9, resign_check_steps=5)
    cap = (p["full_prob"], p["fast_sims"]) if job["mode"].endswith("on") else None
    samples, results, st, elapsed = selfplay.run_games(_net(p["channels"], p["blocks"], GAINS[job["weights"]]), cfg, p["games"],
                                                       "cuda", n_slots=p["slots"], seed=11, poll_every=64 if p["slots"] < 64 else 256,
                                                       tree_reuse=job["mode"].startswith("reuse"), playout_cap=cap)
    torch.cuda.synchronize()
    moves = int(st["moves_played"])
    return {"preset": job["preset"], "weights": job["weights"], "mode": job["mode"], "path": st["path"], "launch": st["launch"],
            "games": int(len(results)), "samples": int(len(samples)), "wall_s": round(elapsed, 2),
            "games_per_hour": round(len(results) * 3600.0 / elapsed, 1), "samples_per_hour": round(len(samples) * 3600.0 / elapsed, 1),
            "steps": int(st["steps"]), "steps_per_game": round(st["steps"] / max(len(results), 1), 2),
            "rows_evaluated": int(st["rows_evaluated"]), "mean_plies": round(float(results["steps"].mean()), 2),
            "moves": moves, "fast_moves": int(st["fast_moves"]), "fast_share": round(st["fast_moves"] / moves, 4) if moves else 0.0,
            "sims": int(st["sims"]), "fast_sims": int(st["fast_sims"]), "reused_visits": int(st["reused_visits"]),
            "resigns": int(st["resigns"]), "samples_equal_full_moves": int(len(samples)) == moves - int(st["fast_moves"]),
            "overflow": int(st["overflow"])}


def trace():
    import torch
    from xiangqi_alphazero_amd import engine, evaluator
    c = TRACE
    ev = evaluator.make_evaluator(_net(c["channels"], c["blocks"], GAINS["peaked"]), "cuda", "hip")[0]
    cfg = engine.make_config(c["slots"], c["sims"], seed=5, start_stagger=True, max_out_samples=c["slots"] * 16)
    eng = engine.SelfPlayEngine(cfg, evaluator=ev, playout_cap=(c["full_prob"], c["fast_sims"]))
    assert eng.capture_step()
    t0 = time.time()
    for i in range(c["steps"]):
        eng.step()
        if i % 256 == 255:
            eng.drain_device()
    torch.cuda.synchronize()
    st = eng.stats()
    print(json.dumps({"steps": eng.steps, "launch": eng.launch_mode, "wall_s": round(time.time() - t0, 1),
                      "moves": st["moves_played"], "fast_moves": st["fast_moves"], "sims": st["sims"],
                      "fast_sims": st["fast_sims"], "overflow": st["overflow"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["games", "trace"])
    ap.add_argument("--preset", choices=sorted(PRESETS), default="cfg1")
    ap.add_argument("--weights", choices=sorted(GAINS), nargs="*", default=sorted(GAINS))
    ap.add_argument("--modes", choices=MODES, nargs="*", default=list(MODES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.part == "trace":
        trace()
        return
    if args.child:
        print("RESULT " + json.dumps(child_games(json.loads(args.child))), flush=True)
        return
    p = PRESETS[args.preset]
    jobs = [dict(preset=args.preset, weights=w, mode=m) for w in args.weights for m in args.modes]   # off / on alternate
    S, Sf, pf = p["sims"], p["fast_sims"], p["full_prob"]
    out = {"tool": "tools/measure_playout_cap.py", "preset": dict(p, name=args.preset),
           "steps_per_game_ratio_expected_without_reuse": round((pf * S + (1 - pf) * Sf + 1) / (S + 1), 4), "runs": []}
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
