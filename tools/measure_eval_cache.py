#!/usr/bin/env python3
"""Evaluation cache (engine.SelfPlayEngine(eval_cache_entries=K)) against the packed step, alternated, each run in a fresh
child process under `timeout -k`; the first failing run ends the measurement.

    python tools/measure_eval_cache.py --config 1 --out profiles/r06_eval_cache_cfg1.json [--games]
    python tools/measure_eval_cache.py --config 2 --out profiles/r06_eval_cache_cfg2.json

configs[1] = 1024 slots x 400 sims x 128x6, configs[2] = 8192 x 800 x 256x10, K = recommended_cache_entries(S).
Per weight set (random init, and peaked: make_state_dict(policy_gain=8)) and mode (off / on) a refilling engine with
staggered starts is warmed for --warm-moves moves and then timed over --steps replayed steps (HIP events): hit rate, rows
evaluated per step, ms per step, simulations/s.  Mode "on-nohit" invalidates the table before every step: the cache's cost
at a hit rate of 0.  --games adds complete games through run_games (games/hour, the records' digest) -- configs[1] only.
"""
import argparse
import sys

import measure_common as mc
from measure_common import GAINS

sys.path.insert(0, mc.ROOT)
CONFIGS = {1: dict(slots=1024, sims=400, channels=128, blocks=6), 2: dict(slots=8192, sims=800, channels=256, blocks=10)}


def _cfg(c):                                    # cfg1's game settings ("full" preset of training/train.py:692-704) at c's simulations
    return mc.selfplay_config(dict(mc.PRESETS["cfg1"], sims=c["sims"]))


def _net(c, weights_name):
    return mc.make_net(c["channels"], c["blocks"], GAINS[weights_name])


def child_steps(job):
    import ctypes as C
    import torch
    from xiangqi_alphazero_amd import engine, evaluator, hip
    c = CONFIGS[job["config"]]
    ev, ev_name = evaluator.make_evaluator(_net(c, job["weights"]), "cuda", "hip")
    cfg = _cfg(c)
    ecfg = engine.make_config(c["slots"], c["sims"], c_puct=cfg.c_puct, temperature_threshold=cfg.temperature_threshold,
                              max_game_length=cfg.max_game_length, random_opening_moves=cfg.random_opening_moves,
                              enable_resign=cfg.enable_resign, resign_threshold=cfg.resign_threshold,
                              resign_check_steps=cfg.resign_check_steps, seed=11, start_stagger=True,
                              max_out_samples=c["slots"] * 201 * 2, max_out_results=c["slots"] * 8)
    K = engine.recommended_cache_entries(c["sims"]) if job["mode"] != "off" else 0
    eng = engine.SelfPlayEngine(ecfg, "cuda", evaluator=ev, eval_cache_entries=K)
    assert eng.capture_step()
    nohit = job["mode"] == "on-nohit"

    def one():
        if nohit:
            hip.check(eng.lib.xq_evcache_invalidate(C.byref(eng.cache), hip.stream_ptr()), "xq_evcache_invalidate")
        eng.step()

    for i in range(job["warm_moves"] * (c["sims"] + 1)):
        one()
        if i % 512 == 511:
            eng.drain_device()
    eng.drain_device()
    torch.cuda.synchronize()
    a = eng.stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(job["steps"]):
        one()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    b = eng.stats()
    d = lambda k: int(b.get(k, 0)) - int(a.get(k, 0))
    probes = d("eval_cache_probes")
    return {"config": job["config"], "weights": job["weights"], "mode": job["mode"], "evaluator": ev_name, "launch": eng.launch_mode,
            "path": eng.path, "entries_per_slot": K, "cache_bytes": engine.eval_cache_bytes(c["slots"], K) if K else 0,
            "steps": job["steps"], "ms_per_step": round(ms / job["steps"], 4), "simulations_per_s": round(d("sims") * 1000.0 / ms, 1),
            "rows_per_step": round(d("rows_evaluated") / job["steps"], 1),
            "hit_rate": round(d("eval_cache_hits") / probes, 4) if probes else 0.0,
            "waiting_per_step": round(probes / job["steps"], 1) if probes else None,
            "mismatches": int(b.get("eval_cache_mismatches", 0)), "evictions_in_window": d("eval_cache_evictions"),
            "overflow": int(b["overflow"])}


def child_games(job):
    import torch
    from xiangqi_alphazero_amd import engine, selfplay
    c = CONFIGS[job["config"]]
    cfg = _cfg(c)
    K = engine.recommended_cache_entries(c["sims"]) if job["mode"] == "on" else 0
    samples, results, st, elapsed = selfplay.run_games(_net(c, job["weights"]), cfg, c["slots"], "cuda", n_slots=c["slots"],
                                                       seed=11, poll_every=256, eval_cache_entries=K)
    torch.cuda.synchronize()
    return {"config": job["config"], "weights": job["weights"], "mode": job["mode"], "kind": "games", "path": st["path"],
            "launch": st["launch"], "games": int(len(results)), "wall_s": round(elapsed, 2),
            "games_per_hour": round(len(results) * 3600.0 / elapsed, 1), "simulations_per_s": round(st["sims"] / elapsed, 1),
            "steps": int(st["steps"]), "rows_evaluated": int(st["rows_evaluated"]), "eval_cache_hits": int(st["eval_cache_hits"]),
            "eval_cache_probes": int(st["eval_cache_probes"]), "mismatches": int(st.get("eval_cache_mismatches", 0)),
            "records_sha256_16": mc.record_hash(samples, results)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=(1, 2), default=1)
    ap.add_argument("--games", action="store_true", help="also complete games through run_games (configs[1])")
    ap.add_argument("--warm-moves", type=int, default=2)
    ap.add_argument("--steps", type=int, default=0, help="timed steps (default: 2000 at configs[1], 200 at configs[2])")
    ap.add_argument("--reps", type=int, default=1, help="off/on pairs per weight set")
    args = mc.parse_args(ap, 600, lambda job: child_games(job) if job.get("kind") == "games" else child_steps(job))
    steps = args.steps or (2000 if args.config == 1 else 200)
    jobs = []
    for w in GAINS:
        for _ in range(args.reps):
            for mode in ("off", "on"):
                jobs.append(dict(config=args.config, weights=w, mode=mode, warm_moves=args.warm_moves, steps=steps))
    jobs.append(dict(config=args.config, weights="random", mode="on-nohit", warm_moves=args.warm_moves, steps=steps))
    if args.games:
        for w in GAINS:
            for mode in ("off", "on"):
                jobs.append(dict(config=args.config, weights=w, mode=mode, kind="games"))
    options = dict(config=args.config, games=args.games, warm_moves=args.warm_moves, steps=steps, reps=args.reps)
    out = {"tool": "tools/measure_eval_cache.py", "options": options, "config": dict(CONFIGS[args.config], name=args.config),
           "runs": []}
    sys.exit(0 if mc.run_children(__file__, jobs, args.timeout, out, args.out) else 1)


if __name__ == "__main__":
    main()
