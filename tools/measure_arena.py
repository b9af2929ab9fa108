#!/usr/bin/env python3
"""The arena gate at scale (arena.play_arena with `opening_plies` and the per-model packed step) against the reference-shaped gate:
every run in a fresh child process under `timeout -k`; the first failing run ends the measurement.  Needs a GPU.

    python tools/measure_arena.py --out profiles/r13_arena_128x6.json
    python tools/measure_arena.py --parts a b --out profiles/r13_arena_gate_only.json

Nets: 128x6, both sides on peaked weights (weights.make_state_dict(policy_gain=8)) with different seeds.  Parts:
  a  the reference-shaped gate: 10 games, 100 simulations, options off (the default path, timed as it ships; a second run through
     an arena-options engine with opening_plies = 0 reports the steps, which the default path does not count)
  b  256 games, opening_plies = 4, packed
  c  1024 games, opening_plies = 4, packed
  d  1024 games, the masked step against the packed step on the same openings, alternated in ONE child (masked, packed, ...):
     wall seconds of each and whether the per-game (winner, steps) tables are equal
  e  1024 games packed, the settled-move cutoff (early_stop) off and on, three alternated pairs in ONE
     child: d's comparison, and per `early` run the settled moves and the simulations saved (--gain 1: random-init-like weights)
Per run: wall seconds (engine construction and graph recording included, after one tiny warm-up arena in the child), engine
steps, tower rows / (steps x slots) -- the masked step runs both towers over every slot, 2 x steps x G rows; the packed step runs
`rows_evaluated` -- games per second, distinct (winner, steps, opening) rows, and the verdict: win rate with its standard error
over the pairs and the 95 % interval (arena.pair_statistics; without openings the games are not pairs of distinct openings and
only the win rate is given).
"""
import argparse
import sys
import time

import measure_common as mc

sys.path.insert(0, mc.ROOT)
CHANNELS, BLOCKS, GAIN, OPENING = 128, 6, 8.0, 4
JOBS = {
    "a": [dict(part="a", games=10, opening_plies=0, modes=["default", "masked"])],
    "b": [dict(part="b", games=256, opening_plies=OPENING, modes=["packed"])],
    "c": [dict(part="c", games=1024, opening_plies=OPENING, modes=["packed"])],
    "d": [dict(part="d", games=1024, opening_plies=OPENING, modes=["masked", "packed", "masked", "packed"])],
}
EARLY = {"e": [dict(part="e", games=1024, opening_plies=OPENING, modes=["packed", "early"] * 3)]}


def _evaluators(gain=GAIN):
    from xiangqi_alphazero_amd import evaluator
    return [evaluator.make_evaluator(mc.make_net(CHANNELS, BLOCKS, gain, seed), "cuda", "hip")[0] for seed in (1, 2)]


def child(job):
    import numpy as np
    import torch
    from xiangqi_alphazero_amd import arena
    if not torch.cuda.is_available():
        raise SystemExit("tools/measure_arena.py needs a GPU")
    en, eo = _evaluators(job.get("gain", GAIN))
    arena.play_arena(en, eo, 2, 4, 4)                                       # warm-up: code objects, allocator
    torch.cuda.synchronize()
    G, R, S, L = job["games"], job["opening_plies"], job["sims"], job["max_game_length"]
    rows, tables = [], []
    for mode in job["modes"]:
        info = None if mode == "default" else {}
        kw = {} if mode == "default" else dict(opening_plies=R, seed=job["seed"], packed=(mode != "masked"), info=info,
                                               **({"early_stop": True} if mode == "early" else {}))
        torch.cuda.synchronize()
        t0 = time.time()
        res = arena.play_arena(en, eo, G, S, L, **kw)
        torch.cuda.synchronize()
        wall = time.time() - t0
        winners, steps = res["winner"].astype(np.int64), res["steps"].astype(np.int64)
        table = list(zip(winners.tolist(), steps.tolist()))
        tables.append((mode, table))
        row = {"part": job["part"], "mode": mode, "games": G, "simulations": S, "max_game_length": L, "opening_plies": R,
               "wall_s": round(wall, 3), "games_per_s": round(G / wall, 2), "mean_plies": round(float(steps.mean()), 2),
               "red_wins": int((winners == 1).sum()), "black_wins": int((winners == -1).sum()), "draws": int((winners == 0).sum())}
        if info is not None:
            st = info["stats"]
            tower_rows = int(st["rows_evaluated"]) if info["packed"] else 2 * info["steps"] * G
            row.update({"steps": info["steps"], "rows_evaluated": int(st["rows_evaluated"]), "tower_rows": tower_rows,
                        "tower_rows_per_step_slot": round(tower_rows / (info["steps"] * G), 4),
                        "requests": int(st["root_evals"] + st["leaf_evals"]), "overflow": int(st["overflow"]),
                        "sims": int(st["sims"]), "moves": int(st["moves_played"]), "settled_moves": st.get("settled_moves"),
                        "simulations_saved": st.get("simulations_saved"),
                        "distinct_games": len({(w, s, tuple(o)) for (w, s), o in zip(table, info["openings"].tolist())}),
                        "distinct_openings": len({tuple(o) for o in info["openings"].tolist()})})
        else:
            row["distinct_games"] = len(set(table))
        if R > 0:
            ps = arena.pair_statistics(winners)
            row.update({"pairs": ps["pairs"], "win_rate": round(ps["win_rate"], 5), "win_rate_se": round(ps["win_rate_se"], 5),
                        "win_rate_ci95": [round(x, 5) for x in ps["win_rate_ci95"]]})
        else:
            score = np.where(winners == 0, 0.5, np.where((winners == 1) == (np.arange(G) % 2 == 0), 1.0, 0.0))
            row["win_rate"] = round(float(score.mean()), 5)
        rows.append(row)
    if job["part"] in ("d", "e"):
        first = tables[0][1]
        rows.append({"part": job["part"], "mode": "comparison", "tables_equal": all(t == first for _, t in tables),
                     **{m + "_wall_s": [r["wall_s"] for r in rows if r["mode"] == m] for m in dict.fromkeys(job["modes"])}})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="*", choices=sorted({**JOBS, **EARLY}), default=sorted(JOBS))
    ap.add_argument("--gain", type=float, default=GAIN, help="policy gain of both networks' weights")
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--max-game-length", type=int, default=300)
    ap.add_argument("--seed", type=int, default=13)
    args = mc.parse_args(ap, 500, child)
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/measure_arena.py needs a GPU")
    out = {"tool": "tools/measure_arena.py", "net": f"{CHANNELS}x{BLOCKS}", "policy_gain": args.gain, "simulations": args.sims,
           "max_game_length": args.max_game_length, "seed": args.seed, "runs": []}
    jobs = [dict(job, sims=args.sims, max_game_length=args.max_game_length, seed=args.seed, gain=args.gain)
            for part in args.parts for job in {**JOBS, **EARLY}[part]]
    sys.exit(0 if mc.run_children(__file__, jobs, args.timeout, out, args.out) else 1)


if __name__ == "__main__":
    main()
