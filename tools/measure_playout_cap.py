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
import sys

import measure_common as mc
from measure_common import GAINS

sys.path.insert(0, mc.ROOT)
# the common presets with the cap: p = 0.25, S_fast = S / 4
PRESETS = {k: dict(mc.PRESETS[k], fast_sims=mc.PRESETS[k]["sims"] // 4, full_prob=0.25)
           for k in ("cfg1", "standard_train")}
MODES = ("off", "on", "reuse", "reuse+on")
TRACE = dict(PRESETS["cfg1"], steps=700)


def child_games(job):
    import torch
    from xiangqi_alphazero_amd import selfplay
    p = PRESETS[job["preset"]]
    cap = (p["full_prob"], p["fast_sims"]) if job["mode"].endswith("on") else None
    samples, results, st, elapsed = selfplay.run_games(mc.make_net(p["channels"], p["blocks"], GAINS[job["weights"]]),
                                                       mc.selfplay_config(p), p["games"], "cuda", n_slots=p["slots"], seed=11,
                                                       poll_every=mc.poll_every(p), tree_reuse=job["mode"].startswith("reuse"), playout_cap=cap)
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
    mc.trace(TRACE, TRACE["steps"], dict(playout_cap=(TRACE["full_prob"], TRACE["fast_sims"])),
             lambda eng, st: {"fast_moves": st["fast_moves"], "fast_sims": st["fast_sims"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["games", "trace"])
    ap.add_argument("--preset", choices=sorted(PRESETS), default="cfg1")
    ap.add_argument("--weights", choices=sorted(GAINS), nargs="*", default=sorted(GAINS))
    ap.add_argument("--modes", choices=MODES, nargs="*", default=list(MODES))
    args = mc.parse_args(ap, 400, child_games)
    if args.part == "trace":
        trace()
        return
    p = PRESETS[args.preset]
    jobs = [dict(preset=args.preset, weights=w, mode=m) for w in args.weights for m in args.modes]   # off / on alternate
    S, Sf, pf = p["sims"], p["fast_sims"], p["full_prob"]
    out = {"tool": "tools/measure_playout_cap.py", "preset": dict(p, name=args.preset),
           "steps_per_game_ratio_expected_without_reuse": round((pf * S + (1 - pf) * Sf + 1) / (S + 1), 4), "runs": []}
    sys.exit(0 if mc.run_children(__file__, jobs, args.timeout, out, args.out, argv=lambda job: ["games"]) else 1)


if __name__ == "__main__":
    main()
