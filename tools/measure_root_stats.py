#!/usr/bin/env python3
"""Root statistics per sample (engine.SelfPlayEngine(root_stats=True)): what recording them costs, and
how the recorded value relates to the game's result.

    python tools/measure_root_stats.py --parent-tree <dir> --out profiles/r16_root_stats_cfg1.json

`--parent-tree` is a built checkout of the PARENT commit (its libxq_hip.so in place).  The "off" runs are taken there, the "on"
runs on this tree, alternated parent, this, parent, this ... in one call, every run in a fresh child process under `timeout -k`;
the first failing run ends the measurement.  A child is this file run with the tree it measures first on sys.path; it uses only
what both trees have.

Per run (preset cfg1 = BASELINE configs[1]: 1024 slots x 400 simulations x 128x6, peaked weights, games_target 1024):
  (a) complete games through run_games: games/hour; and k_select's time per launch over `--select-steps` eager steps from a
      staggered start, device events around xq_engine_select alone (the evaluator and the expansion run full width between them).
      The margin of each figure is the spread (max - min) the PARENT's own repeated runs show in this call.
  (b) over the samples of the "on" games: the mean of |root_q - z| and the share with sign(root_q) != z per ply bucket.
      Descriptive only.

Two limits of what this reports.  The `k_select` figure is the time of the whole `eng.select()` call between two device events:
that is `k_select` alone only because the measured engine has neither tree reuse (which adds `k_reroot` to the call) nor leaf
batching (which launches `k_select_multi`), so xq_engine_select launches exactly one kernel; the figure includes the events'
own overhead, equally on both trees.  And the margin is the spread of the parent's runs in this one call: with the default
`--repeats 2` that is the distance of two runs, a weak margin -- use `--repeats 3` or more where the GPU time allows, and read
"within_margin" as "not distinguishable here", not as "no cost".

Whether a network trained on the mixed target is stronger is NOT measured here: that takes arena matches over trained networks.
"""
import argparse
import json
import sys

import measure_common as mc

PRESETS = {k: mc.PRESETS[k] for k in ("cfg1", "small")}
BUCKETS = ((0, 20), (20, 40), (40, 80), (80, 120), (120, 1 << 16))


def _ply_buckets(samples):
    import numpy as np
    pad = np.ascontiguousarray(samples["pad"])
    q = pad[:, 0:4].copy().view(np.float32).reshape(-1)
    mark = pad[:, 8] == 1
    z, ply = samples["z"].astype(np.float64), samples["ply"].astype(np.int64)
    out = []
    for lo, hi in BUCKETS:
        m = mark & (ply >= lo) & (ply < hi)
        n = int(m.sum())
        out.append({"plies": [lo, None if hi >= 1 << 16 else hi - 1], "samples": n,
                    "mean_abs_q_minus_z": round(float(np.abs(q[m] - z[m]).mean()), 4) if n else None,
                    "share_sign_differs": round(float((np.sign(q[m]) != z[m]).mean()), 4) if n else None})
    return {"marked": int(mark.sum()), "samples": int(len(samples)), "buckets": out}


def child(job):
    import torch
    from xiangqi_alphazero_amd import selfplay
    p = PRESETS[job["preset"]]
    on = job["root_stats"] == "on"
    net = mc.make_net(p["channels"], p["blocks"])
    cfg = mc.selfplay_config(p, **({"record_root_stats": True} if on else {}))    # the config key, as a training loop sets it
    samples, results, st, elapsed = selfplay.run_games(net, cfg, p["games"], "cuda", n_slots=p["slots"], seed=11, poll_every=256)
    torch.cuda.synchronize()
    assert bool(st.get("root_stats", False)) == on and int(st["overflow"]) == 0
    row = {"preset": job["preset"], "tree": job["tree"], "root_stats": on, "path": st["path"], "launch": st["launch"],
           "games": int(len(results)), "samples": int(len(samples)), "wall_s": round(elapsed, 2),
           "games_per_hour": round(len(results) * 3600.0 / elapsed, 1), "mean_plies": round(float(results["steps"].mean()), 2),
           "moves": int(st["moves_played"]), "sims": int(st["sims"])}
    if on:
        row["root_q_against_z"] = _ply_buckets(samples)
    # k_select alone: eager steps from a staggered start, the stages called one by one, events around the select launch
    eng = mc.staggered_engine(p, net, **({"root_stats": True} if on else {}))
    steps, warm = int(job["select_steps"]), 32
    pairs = []
    for i in range(warm + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        x = eng.select()
        b.record()
        eng.evaluate_and_expand(x)
        if i >= warm:
            pairs.append((a, b))
        if i % 256 == 255:
            eng.drain_device()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    est = eng.stats()
    assert int(est["overflow"]) == 0
    row.update(k_select_us_mean=round(1000.0 * sum(ms) / len(ms), 3), k_select_us_median=round(1000.0 * ms[len(ms) // 2], 3),
               select_steps=steps, select_moves=int(est["moves_played"]))
    return row


def summarise(out, job, row):
    mc.parent_this_summary(out, ("games_per_hour", "k_select_us_mean", "k_select_us_median"))
    if "summary" in out:
        out["summary"]["root_q_against_z"] = [r for r in out["runs"] if r["tree"] == "this"][-1].get("root_q_against_z")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=sorted(PRESETS), default="cfg1")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: the `off` runs are taken there")
    ap.add_argument("--repeats", type=int, default=2, help="parent/this pairs")
    ap.add_argument("--select-steps", type=int, default=600)
    args = mc.parse_args(ap, 400, child)
    out = {"tool": "tools/measure_root_stats.py", "preset": dict(PRESETS[args.preset], name=args.preset), "weights": "peaked",
           "order": [], "runs": []}
    jobs = mc.off_on_jobs(args.parent_tree, args.repeats, "root_stats", preset=args.preset, select_steps=args.select_steps)
    ok = mc.run_children(__file__, jobs, args.timeout, out, args.out, cwd=lambda job: job["tree_path"], after_each=summarise)
    if "summary" in out:
        print(json.dumps(out["summary"], indent=1))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
