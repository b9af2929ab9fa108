#!/usr/bin/env python3
"""The Gumbel root search with sequential halving (engine.SelfPlayEngine(gumbel=(m, c_visit, c_scale))) against the engine without
it: complete games through run_games, the modes alternated, each run in a fresh child process under `timeout -k`; the first
failing run ends the measurement.

    python tools/measure_gumbel.py games --preset cfg1 --modes off on off on --out profiles/r12_gumbel_cfg1_games.json
    python tools/measure_gumbel.py games --preset standard_train --modes off on on@32 on@64 off on on@32 on@64 --out ...
    python tools/measure_gumbel.py shape --preset standard_train --sims 32 --out profiles/r12_gumbel_search_shape.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_gumbel.py trace --preset cfg1 --gumbel 0
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_gumbel.py trace --preset cfg1 --gumbel 16

Presets: cfg1 = BASELINE configs[1] (1024 slots x 400 sims x 128x6, games_target 1024); standard_train = the reference's
standard_train preset (20 games x 200 sims x 128x6); small = 256 slots x 64 sims x 64x2 (a quick look).  m = 16, c_visit = 50,
c_scale = 1.  Weights: peaked (make_state_dict(policy_gain=8)) unless --weights says otherwise.  Modes: `off`, `on` (the preset's
S), `on@N` (Gumbel at N simulations: the few-simulation regime the rule is made for, against `off` at the preset's S).
Per run: games/hour, samples/hour, steps, rows evaluated, mean plies, considered moves per Gumbel move, the share of moves whose
played child is not the prior's first maximum.  Whether training gains from the option is not measured here.
`shape` searches positions drawn from a Gumbel self-play run again on a search-only engine (no history ring: repetition is not
seen) and rebuilds the improved policy on the host from the root's visits, W, priors and kept network value by the header's
formula: the share of the target's mass that lies on unvisited children.
`trace` runs replayed steps at a preset from a staggered start for a kernel trace of k_select / k_expand: once with --gumbel 0
(the instances the same engine launches without the option: the comparison figure) and once with --gumbel 16.
"""
import argparse
import sys

import measure_common as mc
from measure_common import GAINS, PRESETS

sys.path.insert(0, mc.ROOT)
M, C_VISIT, C_SCALE = 16, 50.0, 1.0


def _mode(mode, preset_sims):
    """'off' | 'on' | 'on@N' -> (gumbel or None, simulations)"""
    name, _, n = mode.partition("@")
    if name not in ("off", "on"):
        raise SystemExit(f"unknown mode {mode}")
    return ((M, C_VISIT, C_SCALE) if name == "on" else None), (int(n) if n else preset_sims)


def child_games(job):
    import torch
    from xiangqi_alphazero_amd import selfplay
    p = PRESETS[job["preset"]]
    gumbel, S = _mode(job["mode"], p["sims"])
    samples, results, st, elapsed = selfplay.run_games(mc.make_net(p["channels"], p["blocks"], GAINS[job["weights"]]),
                                                       mc.selfplay_config(p, num_simulations=S), p["games"], "cuda",
                                                       n_slots=p["slots"], seed=11, poll_every=mc.poll_every(p), gumbel=gumbel)
    torch.cuda.synchronize()
    moves, gm = int(st["moves_played"]), int(st["gumbel_moves"])
    return {"preset": job["preset"], "weights": job["weights"], "mode": job["mode"], "gumbel": st["gumbel"], "sims_per_move": S,
            "path": st["path"], "launch": st["launch"], "games": int(len(results)), "samples": int(len(samples)),
            "wall_s": round(elapsed, 2), "games_per_hour": round(len(results) * 3600.0 / elapsed, 1),
            "samples_per_hour": round(len(samples) * 3600.0 / elapsed, 1), "steps": int(st["steps"]),
            "steps_per_game": round(st["steps"] / max(len(results), 1), 2), "rows_evaluated": int(st["rows_evaluated"]),
            "mean_plies": round(float(results["steps"].mean()), 2), "moves": moves, "sims": int(st["sims"]),
            "gumbel_moves": gm, "gumbel_considered": int(st["gumbel_considered"]), "gumbel_offprior": int(st["gumbel_offprior"]),
            "considered_per_move": round(st["gumbel_considered"] / gm, 3) if gm else 0.0,
            "offprior_share": round(st["gumbel_offprior"] / gm, 5) if gm else 0.0,
            "improved_policy_samples": int((samples["reserved0"] == 1).sum()) if len(samples) else 0,
            "red_wins": int(st["red_wins"]), "black_wins": int(st["black_wins"]), "draws": int(st["draws"]),
            "resigns": int(st["resigns"]), "overflow": int(st["overflow"])}


def shape(preset, sims, weights, positions):
    """Search-shape figures that need the tree: positions of a Gumbel self-play run searched again, search only."""
    import numpy as np
    import torch
    from xiangqi_alphazero_amd import engine, evaluator, selfplay
    p = PRESETS[preset]
    net = mc.make_net(p["channels"], p["blocks"], GAINS[weights])
    gumbel = (M, C_VISIT, C_SCALE)
    samples, results, st, _ = selfplay.run_games(net, mc.selfplay_config(p, num_simulations=sims), p["games"], "cuda",
                                                 n_slots=p["slots"], seed=11, gumbel=gumbel)
    pick = samples[np.linspace(0, len(samples) - 1, min(positions, len(samples))).astype(np.int64)]
    ev = evaluator.make_evaluator(net, "cuda", "hip")[0]
    eng = engine.SelfPlayEngine(engine.make_config(len(pick), sims, seed=23, manual_moves=1), evaluator=ev, gumbel=gumbel)
    for slot, s in enumerate(pick):
        eng.set_position(slot, s["board"], int(s["side"]))
    for _ in range(2 * sims + 8):
        eng.step()
        if eng.held():
            break
    assert eng.held() and eng.stats()["overflow"] == 0
    v_hat = eng.gumbel_root_values().cpu().numpy()
    tp_all = eng.arena_views()["P"].cpu().numpy()
    cv, cs = float(np.float32(C_VISIT)), float(np.float32(C_SCALE))
    unvisited, visited_children, top1, kl = [], [], [], []
    for slot in range(len(pick)):
        r = eng.read_root(slot)
        n = len(r["actions"])
        N, W = r["visits"].astype(np.int64), r["total_value"]
        tp = tp_all[slot, 1:1 + n].astype(np.float64)
        l = np.log(np.maximum(tp, float(np.finfo(np.float32).tiny)))
        q = np.divide(W, N, out=np.zeros(n), where=N > 0)
        vis = N > 0
        v_mix = (v_hat[slot] + N.sum() * ((tp[vis] * q[vis]).sum() / tp[vis].sum())) / (1.0 + N.sum())
        x = l + ((cv + N.max()) * cs) * ((np.where(vis, q, v_mix) + 1.0) * 0.5)
        pi = np.exp(x - x.max())
        pi /= pi.sum()
        unvisited.append(float(pi[~vis].sum()))
        visited_children.append(int(vis.sum()))
        top1.append(float(pi.max()))
        kl.append(float((pi * (np.log(np.maximum(pi, 1e-300)) - np.log(tp / tp.sum()))).sum()))
    gm = int(st["gumbel_moves"])
    return {"preset": preset, "weights": weights, "sims_per_move": sims, "gumbel": list(gumbel), "self_play_moves": gm,
            "considered_per_move": round(st["gumbel_considered"] / gm, 3), "offprior_share": round(st["gumbel_offprior"] / gm, 5),
            "positions_searched_again": len(pick), "note": "search only, no history ring, fresh device Gumbel draws",
            "visited_children_mean": round(float(np.mean(visited_children)), 3),
            "target_mass_on_unvisited_children_mean": round(float(np.mean(unvisited)), 5),
            "target_mass_on_unvisited_children_median": round(float(np.median(unvisited)), 5),
            "target_largest_entry_mean": round(float(np.mean(top1)), 5),
            "kl_target_from_prior_mean_nats": round(float(np.mean(kl)), 4)}


def trace(preset, m, steps):
    mc.trace(PRESETS[preset], steps, dict(gumbel=(m, C_VISIT, C_SCALE) if m > 0 else None),
             lambda eng, st: {"preset": preset, "gumbel": eng.gumbel, "gumbel_moves": st["gumbel_moves"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["games", "shape", "trace"])
    ap.add_argument("--preset", choices=sorted(PRESETS), default="cfg1")
    ap.add_argument("--weights", choices=sorted(GAINS), default="peaked")
    ap.add_argument("--modes", nargs="*", default=["off", "on", "off", "on"], help="games: off | on | on@N, run in this order")
    ap.add_argument("--gumbel", type=int, default=M, help="trace: considered moves, 0 = the engine without the option")
    ap.add_argument("--steps", type=int, default=700, help="trace: replayed steps")
    ap.add_argument("--sims", type=int, default=32, help="shape: simulations per move")
    ap.add_argument("--positions", type=int, default=512, help="shape: positions searched again")
    args = mc.parse_args(ap, 400, lambda job: shape(job["preset"], job["sims"], job["weights"], job["positions"])
                         if job.get("shape") else child_games(job))
    if args.part == "trace":
        trace(args.preset, args.gumbel, args.steps)
        return
    p = PRESETS[args.preset]
    if args.part == "shape":
        jobs = [dict(shape=True, preset=args.preset, weights=args.weights, sims=args.sims, positions=args.positions)]
    else:
        jobs = [dict(preset=args.preset, weights=args.weights, mode=m) for m in args.modes]
    out = {"tool": "tools/measure_gumbel.py", "part": args.part, "preset": dict(p, name=args.preset),
           "gumbel": [M, C_VISIT, C_SCALE], "runs": []}
    sys.exit(0 if mc.run_children(__file__, jobs, args.timeout, out, args.out, argv=lambda job: [args.part]) else 1)


if __name__ == "__main__":
    main()
