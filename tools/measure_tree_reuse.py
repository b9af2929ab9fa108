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
import sys

import measure_common as mc
from measure_common import GAINS

sys.path.insert(0, mc.ROOT)
# the common presets with the modes each is measured in
PRESETS = {"cfg1": dict(mc.PRESETS["cfg1"], modes=("off", "on", "on+cache")),
           "standard_train": dict(mc.PRESETS["standard_train"], modes=("off", "on"))}
TRACE = {1: dict(mc.PRESETS["cfg1"], steps=700),
         2: dict(slots=8192, sims=800, channels=256, blocks=10, steps=1000)}


def child_games(job):
    import torch
    from xiangqi_alphazero_amd import engine, selfplay
    p = PRESETS[job["preset"]]
    K = engine.recommended_cache_entries(p["sims"]) if job["mode"] == "on+cache" else 0
    samples, results, st, elapsed = selfplay.run_games(mc.make_net(p["channels"], p["blocks"], GAINS[job["weights"]]),
                                                       mc.selfplay_config(p), p["games"], "cuda", n_slots=p["slots"], seed=11,
                                                       poll_every=mc.poll_every(p), eval_cache_entries=K, tree_reuse=job["mode"] != "off")
    torch.cuda.synchronize()
    visits = int(sum(int(s["visits"][:s["n_moves"]].sum()) for s in samples))
    total = st["sims"] + st["reused_visits"]
    return {"preset": job["preset"], "weights": job["weights"], "mode": job["mode"], "path": st["path"], "launch": st["launch"],
            "games": int(len(results)), "wall_s": round(elapsed, 2), "games_per_hour": round(len(results) * 3600.0 / elapsed, 1),
            "steps": int(st["steps"]), "rows_evaluated": int(st["rows_evaluated"]), "sims": int(st["sims"]),
            "reused_visits": int(st["reused_visits"]), "reroots": int(st["reroots"]),
            "reused_share": round(st["reused_visits"] / total, 4) if total else 0.0, "moves": int(st["moves_played"]),
            "sample_visits_equal_sims_plus_reused": visits == total, "eval_cache_hits": int(st["eval_cache_hits"]),
            "overflow": int(st["overflow"]), "records_sha256_16": mc.record_hash(samples, results)}


def trace(config):
    mc.trace(TRACE[config], TRACE[config]["steps"], dict(tree_reuse=True),
             lambda eng, st: {"config": config, "reroots": st["reroots"], "reused_visits": st["reused_visits"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["games", "trace"])
    ap.add_argument("--preset", choices=sorted(PRESETS), default="cfg1")
    ap.add_argument("--config", type=int, choices=(1, 2), default=1)
    args = mc.parse_args(ap, 400, child_games)
    if args.part == "trace":
        trace(args.config)
        return
    p = PRESETS[args.preset]
    jobs = [dict(preset=args.preset, weights=w, mode=m) for w in GAINS for m in p["modes"]]   # alternated within each weight set
    out = {"tool": "tools/measure_tree_reuse.py", "preset": dict(p, name=args.preset), "runs": []}
    sys.exit(0 if mc.run_children(__file__, jobs, args.timeout, out, args.out, argv=lambda job: ["games"]) else 1)


if __name__ == "__main__":
    main()
