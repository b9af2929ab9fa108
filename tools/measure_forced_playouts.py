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
import sys

import measure_common as mc
from measure_common import GAINS, PRESETS

sys.path.insert(0, mc.ROOT)
MODES = ("off", "on", "cap", "cap+on")
K_FORCED, CAP_PROB = 2.0, 0.25


def child_games(job):
    import numpy as np
    import torch
    from xiangqi_alphazero_amd import selfplay
    p = PRESETS[job["preset"]]
    S = p["sims"]
    cap = (CAP_PROB, max(1, S // 4)) if job["mode"].startswith("cap") else None
    forced = K_FORCED if job["mode"].endswith("on") else None
    samples, results, st, elapsed = selfplay.run_games(mc.make_net(p["channels"], p["blocks"], GAINS[job["weights"]]),
                                                       mc.selfplay_config(p), p["games"], "cuda", n_slots=p["slots"], seed=11,
                                                       poll_every=mc.poll_every(p), playout_cap=cap, forced_playouts=forced)
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
    c = PRESETS[preset]
    kw = dict(forced_playouts=forced if forced > 0 else None, playout_cap=(CAP_PROB, max(1, c["sims"] // 4)) if with_cap else None)
    mc.trace(c, steps, kw, lambda eng, st: {"preset": preset, "k": eng.forced_playouts, "playout_cap": eng.playout_cap,
                                            "forced_sims": st["forced_sims"], "pruned_visits": st["pruned_visits"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["games", "trace"])
    ap.add_argument("--preset", choices=sorted(PRESETS), default="cfg1")
    ap.add_argument("--weights", choices=sorted(GAINS), nargs="*", default=sorted(GAINS))
    ap.add_argument("--modes", choices=MODES, nargs="*", default=list(MODES))
    ap.add_argument("--forced", type=float, default=K_FORCED, help="trace: k, 0 = the engine without the option")
    ap.add_argument("--steps", type=int, default=700, help="trace: replayed steps")
    ap.add_argument("--cap", action="store_true", help="trace: with the playout cap")
    args = mc.parse_args(ap, 400, child_games)
    if args.part == "trace":
        trace(args.preset, args.forced, args.steps, args.cap)
        return
    p = PRESETS[args.preset]
    jobs = [dict(preset=args.preset, weights=w, mode=m) for w in args.weights for m in args.modes]   # off / on alternate
    out = {"tool": "tools/measure_forced_playouts.py", "preset": dict(p, name=args.preset), "k": K_FORCED, "runs": []}
    sys.exit(0 if mc.run_children(__file__, jobs, args.timeout, out, args.out, argv=lambda job: ["games"]) else 1)


if __name__ == "__main__":
    main()
