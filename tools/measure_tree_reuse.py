#!/usr/bin/env python3
"""Tree reuse across moves (engine.SelfPlayEngine(tree_reuse=True)) against the engine without it: complete games through
run_games, alternated, each run in a fresh child process under `timeout -k`; the first failing run ends the measurement.

    python tools/measure_tree_reuse.py games --preset cfg1 --out profiles/r08_tree_reuse_cfg1_games.json
    python tools/measure_tree_reuse.py games --preset standard_train --out profiles/r08_tree_reuse_standard_train.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_tree_reuse.py trace --config 1

Presets: cfg1 = BASELINE configs[1] (1024 slots x 400 sims x 128x6, games_target 1024, the "full" game settings of
training/train.py:692-704); standard_train = the reference's standard_train preset (20 games x 200 sims x 128x6).  Weights:
random init, and peaked (make_state_dict(policy_gain=8)).  Modes: off, on, and at cfg1 on + the evaluation cache.  Per run:
games/hour, steps, rows evaluated, new simulations, reused visits and the reused share reused_visits / (sims + reused_visits).
`trace` runs replayed reuse-on steps at configs[1] (1024 x 400 x 128x6) or configs[2] (8192 x 800 x 256x10) from a staggered
start, long enough that slots end moves every step, for a kernel trace of k_reroot.
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
                 random_opening_moves=8, modes=("off", "on", "on+cache")),
    "standard_train": dict(slots=20, games=20, sims=200, channels=128, blocks=6, temperature_threshold=20, max_game_length=300,
                           random_opening_moves=6, modes=("off", "on")),
}
TRACE = {1: dict(slots=1024, sims=400, channels=128, blocks=6, steps=700),
         2: dict(slots=8192, sims=800, channels=256, blocks=10, steps=1000)}


def _net(channels, blocks, gain):
    from xiangqi_alphazero_amd import model, weights
    net = model.XiangqiNet(channels, blocks)
    net.load_state_dict(weights.make_state_dict(channels, blocks, policy_gain=gain))
    return net


def child_games(job):
    import hashlib
    import numpy as np
    import torch
    from xiangqi_alphazero_amd import engine, selfplay
    p = PRESETS[job["preset"]]
    cfg = types.SimpleNamespace(num_simulations=p["sims"], c_puct=1.5, temperature_threshold=p["temperature_threshold"],
                                max_game_length=p["max_game_length"], random_opening_moves=p["random_opening_moves"],
                                enable_resign=True, resign_threshold=-0.9, resign_check_steps=5)
    K = engine.recommended_cache_entries(p["sims"]) if job["mode"] == "on+cache" else 0
    samples, results, st, elapsed = selfplay.run_games(_net(p["channels"], p["blocks"], GAINS[job["weights"]]), cfg, p["games"],
                                                       "cuda", n_slots=p["slots"], seed=11, poll_every=64 if p["slots"] < 64 else 256,
                                                       eval_cache_entries=K, tree_reuse=job["mode"] != "off")
    torch.cuda.synchronize()
    digest = hashlib.sha256(np.sort(results, order=["slot", "game_seq"]).tobytes() +
                            np.sort(samples, order=["slot", "game_seq", "ply"]).tobytes()).hexdigest()[:16]
    visits = int(sum(int(s["visits"][:s["n_moves"]].sum()) for s in samples))
    total = st["sims"] + st["reused_visits"]
    return {"preset": job["preset"], "weights": job["weights"], "mode": job["mode"], "path": st["path"], "launch": st["launch"],
            "games": int(len(results)), "wall_s": round(elapsed, 2), "games_per_hour": round(len(results) * 3600.0 / elapsed, 1),
            "steps": int(st["steps"]), "rows_evaluated": int(st["rows_evaluated"]), "sims": int(st["sims"]),
            "reused_visits": int(st["reused_visits"]), "reroots": int(st["reroots"]),
            "reused_share": round(st["reused_visits"] / total, 4) if total else 0.0, "moves": int(st["moves_played"]),
            "sample_visits_equal_sims_plus_reused": visits == total, "eval_cache_hits": int(st["eval_cache_hits"]),
            "overflow": int(st["overflow"]), "records_sha256_16": digest}


def trace(config):
    import torch
    from xiangqi_alphazero_amd import engine, evaluator
    c = TRACE[config]
    ev = evaluator.make_evaluator(_net(c["channels"], c["blocks"], GAINS["peaked"]), "cuda", "hip")[0]
    cfg = engine.make_config(c["slots"], c["sims"], seed=5, start_stagger=True, max_out_samples=c["slots"] * 16)
    eng = engine.SelfPlayEngine(cfg, evaluator=ev, tree_reuse=True)
    assert eng.capture_step()
    t0 = time.time()
    for i in range(c["steps"]):
        eng.step()
        if i % 256 == 255:
            eng.drain_device()
    torch.cuda.synchronize()
    st = eng.stats()
    print(json.dumps({"config": config, "steps": eng.steps, "launch": eng.launch_mode, "wall_s": round(time.time() - t0, 1),
                      "moves": st["moves_played"], "reroots": st["reroots"], "reused_visits": st["reused_visits"],
                      "sims": st["sims"], "overflow": st["overflow"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["games", "trace"])
    ap.add_argument("--preset", choices=sorted(PRESETS), default="cfg1")
    ap.add_argument("--config", type=int, choices=(1, 2), default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.part == "trace":
        trace(args.config)
        return
    if args.child:
        print("RESULT " + json.dumps(child_games(json.loads(args.child))), flush=True)
        return
    p = PRESETS[args.preset]
    jobs = [dict(preset=args.preset, weights=w, mode=m) for w in GAINS for m in p["modes"]]   # alternated within each weight set
    out = {"tool": "tools/measure_tree_reuse.py", "preset": dict(p, name=args.preset), "runs": []}
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
