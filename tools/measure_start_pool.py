"""Start-position pool: complete games through run_games, off (--prob 0) and from a `from_table` pool ("R", won entries) at each
--prob; every run a fresh child under `timeout -k` (--timeout), the first failure ends it.  --out profiles/r27_start_pool_<preset>.json
--adjudicate N: table adjudication off and on, alternated N times, on a pool of won and drawn "Nb" entries at the largest --prob.  --resign N T: the per-side resign rule off and on at threshold T (K = 5, holdout 0.1), alternated N times, from the initial position."""
import argparse, sys  # noqa: E401
import measure_common as mc
def child(job):  # noqa: E302
    from xiangqi_alphazero_amd import endgame, resign, selfplay, start_pool
    p, prob = mc.PRESETS[job["preset"]], job["prob"]
    tb, kinds = (endgame.Tablebase.generate("Nb", "cuda"), ("win", "draw")) if "adjudicate" in job else (endgame.Tablebase.generate("R", "cuda"), ("win",))
    pool = (*start_pool.from_table(tb, 4096, kinds, seed=1, min_plies=5), prob) if prob else None
    smp, res, st, t = selfplay.run_games(mc.make_net(p["channels"], p["blocks"]), mc.selfplay_config(p), p["games"], "cuda",
                                         n_slots=p["slots"], seed=11, poll_every=mc.poll_every(p), start_pool=pool,
                                         **({"adjudicate": ((tb,), {})} if job.get("adjudicate") else {}),
                                         **({"resign": dict(threshold=job["resign"], check_steps=5, holdout_prob=0.1)} if job.get("resign") else {}))
    return dict(job, games=len(res), games_per_hour=round(len(res) * 3600.0 / t, 1), mean_plies=round(float(res["steps"].mean()), 2),
                samples_per_game=round(len(smp) / len(res), 2), pool_games=st["start_pool_games"], overflow=int(st["overflow"]),
                samples_per_hour=round(len(smp) * 3600.0 / t, 1), adjudicated_games=st["adjudicated_games"], wall_s=round(t, 2),
                resigned=st["resign_resigned"], holdout_games=st["resign_holdout_games"], fp_curve=None if st["resign_rows"] is None else {k: getattr(v, "tolist", lambda: v)() for k, v in resign.false_positive_curve(st["resign_rows"]).items()})
ap =argparse.ArgumentParser()
ap.add_argument("--preset", choices=sorted(mc.PRESETS), default="small")
ap.add_argument("--adjudicate", type=int, default=0, help="N > 0: N alternated off/on pairs of table adjudication instead")
ap.add_argument("--resign", type=float, nargs=2, default=[0, 0], help="N T: N alternated off/on pairs of the per-side resign rule at threshold T instead")
ap.add_argument("--prob", type=float, nargs="*", default=[0.0, 1.0, 0.25], help="0 = the option off")
args = mc.parse_args(ap, 400, child)
sys.exit(0 if mc.run_children(__file__, [dict(preset=args.preset, prob=0.0, resign=a) for _ in range(int(args.resign[0])) for a in (0, args.resign[1])] or [dict(preset=args.preset, prob=max(args.prob), adjudicate=a) for _ in range(args.adjudicate) for a in (0, 1)] or
                              [dict(preset=args.preset, prob=q) for q in args.prob], args.timeout,
                              {"tool": "tools/measure_start_pool.py", "runs": []}, args.out) else 1)
