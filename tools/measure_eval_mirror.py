#!/usr/bin/env python3
"""Evaluation mirror (engine.SelfPlayEngine(eval_mirror=True)): what the mirrored gather costs, and how
asymmetric a network is -- the quantity the option averages away.

    python tools/measure_eval_mirror.py a --parent-tree <dir> --out profiles/r17_eval_mirror_cfg1.json
    python tools/measure_eval_mirror.py b --out profiles/r17_eval_mirror_asymmetry.json
    python tools/measure_eval_mirror.py steps --mirror on|off          (a short eager run, for a kernel trace taken around it)

Every run is a fresh child process under `timeout -k`; the first failing run ends the measurement.

Mode a.  `--parent-tree` is a built checkout of the PARENT commit (its libxq_hip.so in place).  The "off" runs are taken there,
the "on" runs on this tree, alternated parent, this, parent, this ... in one call.  A child is this file run with the tree it
measures first on sys.path; on the parent's tree it uses only what both trees have.  Per run (preset cfg1 = BASELINE configs[1]:
1024 slots x 400 simulations x 128x6, peaked weights, games_target 1024):
  * complete games through run_games (packed step, replayed graph): games/hour;
  * the replayed step: `--step-steps` graph replays from a staggered start between two device events, microseconds per step.
The margin of each figure is the spread (max - min) of the PARENT's own runs in this call: with `--repeats 2` the distance of two
runs, a weak margin.  Read "within_margin" as "not distinguishable here", not as "no cost".  Games with the option on are other
games (the network's answers differ), so games/hour also moves with the games' lengths; the step time does not.

Mode b.  For two 128x6 networks (`random`: weights.make_state_dict's default gain; `peaked`: policy_gain 8), each over
`--positions` corpus positions (tests/golden/corpus.npz, positions that are not over): the request and its mirror image
(hip.mirror_requests) are both evaluated;
  * |v(x) - v(mirror x)|: mean and maximum;
  * the total-variation distance between the legal-move priors of the request and the un-mirrored priors of the mirrored request
    (the softmax over the legal logits of each; the mirrored request's list keeps the order, so index i is the same move): mean
    and maximum.
A network that is exactly symmetric shows zeros and the option changes nothing for it.

Mode steps.  `--steps` eager packed steps of a `--preset` engine from a staggered start with the option on or off and nothing
else: run the child under a kernel trace, in a run of its own, to read the per-launch time of k_gather_rows_mirror against
k_gather_rows (`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_eval_mirror.py steps --child '<job>'`, the job
being {"mode": "steps", "tree_path": "<this tree>", "preset": "cfg1", "mirror": "on" or "off", "steps": 400}).

Whether a network trained from such games is stronger is NOT measured here: that takes arena matches over trained networks.
"""
import argparse
import json
import os
import sys

import measure_common as mc
from measure_common import ROOT

PRESETS = {k: mc.PRESETS[k] for k in ("cfg1", "small")}


def child_a(job):
    import torch
    from xiangqi_alphazero_amd import selfplay
    p = PRESETS[job["preset"]]
    on = job["mirror"] == "on"
    net = mc.make_net(p["channels"], p["blocks"])
    cfg = mc.selfplay_config(p, **({"eval_random_mirror": True} if on else {}))   # the config key, as a training loop sets it
    samples, results, st, elapsed = selfplay.run_games(net, cfg, p["games"], "cuda", n_slots=p["slots"], seed=11, poll_every=256)
    torch.cuda.synchronize()
    assert bool(st.get("eval_mirror", False)) == on and int(st["overflow"]) == 0
    row = {"preset": job["preset"], "tree": job["tree"], "eval_mirror": on, "path": st["path"], "launch": st["launch"],
           "games": int(len(results)), "samples": int(len(samples)), "wall_s": round(elapsed, 2),
           "games_per_hour": round(len(results) * 3600.0 / elapsed, 1), "mean_plies": round(float(results["steps"].mean()), 2),
           "moves": int(st["moves_played"]), "sims": int(st["sims"]), "steps": int(st["steps"]),
           "rows_evaluated": int(st["rows_evaluated"])}
    # the replayed step from a staggered start: one graph launch per step between two device events
    eng = mc.staggered_engine(p, net, **({"eval_mirror": True} if on else {}))
    assert eng.capture_step() and eng.launch_mode == "graph"
    steps, warm, chunk = int(job["step_steps"]), 64, 100
    for _ in range(warm):
        eng.step()
    chunks = []
    for _ in range(steps // chunk):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(chunk):
            eng.step()
        b.record()
        chunks.append((a, b))
        eng.drain_device()
    torch.cuda.synchronize()
    us = sorted(1000.0 * a.elapsed_time(b) / chunk for a, b in chunks)
    est = eng.stats()
    assert int(est["overflow"]) == 0
    row.update(step_us_mean=round(sum(us) / len(us), 3), step_us_median=round(us[len(us) // 2], 3), step_us_min=round(us[0], 3),
               step_steps=len(us) * chunk, step_rows_evaluated=int(est["rows_evaluated"]))
    return row


def child_b(job):
    import numpy as np
    import torch
    from xiangqi_alphazero_amd import evaluator, hip
    z = np.load(os.path.join(ROOT, "tests", "golden", "corpus.npz"))
    picks = np.nonzero(z["done"] == 0)[0]
    picks = picks[::max(1, len(picks) // int(job["positions"]))][:int(job["positions"])]
    boards = torch.from_numpy(z["board"][picks].copy()).cuda()
    sides = torch.from_numpy(z["side"][picks].copy()).cuda()
    x = hip.encode(boards, sides)
    moves, counts, _, _ = hip.movegen(boards, sides)
    counts = counts.to(torch.int32)
    mx, mmoves = hip.mirror_requests(x, moves, counts, torch.ones(len(x), dtype=torch.uint8, device="cuda"))
    net = mc.make_net(job["channels"], job["blocks"], mc.GAINS[job["weights"]])
    ev = evaluator.make_evaluator(net, "cuda", "hip")[0]
    ll, v = (t.clone().double() for t in ev.evaluate_legal(x, moves, counts))
    mll, mv = (t.clone().double() for t in ev.evaluate_legal(mx, mmoves, counts))
    torch.cuda.synchronize()
    legal = torch.arange(hip.MAXM, device="cuda")[None, :] < counts[:, None]
    neg = torch.full_like(ll, -float("inf"))
    p, mp = torch.softmax(torch.where(legal, ll, neg), 1), torch.softmax(torch.where(legal, mll, neg), 1)
    tv = 0.5 * (p - mp).abs().sum(1)
    dv = (v - mv).abs()
    return {"weights": job["weights"], "channels": job["channels"], "blocks": job["blocks"], "positions": int(len(picks)),
            "abs_value_difference": {"mean": round(float(dv.mean()), 6), "max": round(float(dv.max()), 6)},
            "abs_value_mean": round(float(v.abs().mean()), 6),
            "prior_total_variation": {"mean": round(float(tv.mean()), 6), "max": round(float(tv.max()), 6)}}


def child_steps(job):
    p = PRESETS[job["preset"]]
    on = job["mirror"] == "on"
    eng = mc.staggered_engine(p, out_rows_per_slot=64, **({"eval_mirror": True} if on else {}))
    mc.replay_steps(eng, int(job["steps"]))                      # eager: no step is captured here
    st = eng.stats()
    assert int(st["overflow"]) == 0
    return {"eval_mirror": on, "steps": int(job["steps"]), "rows_evaluated": int(st["rows_evaluated"]), "slots": p["slots"],
            "preset": job["preset"]}


CHILDREN = {"a": child_a, "b": child_b, "steps": child_steps}


def summarise(out, job, row):
    mc.parent_this_summary(out, ("games_per_hour", "step_us_mean", "step_us_median"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=sorted(CHILDREN))
    ap.add_argument("--preset", choices=sorted(PRESETS), default="cfg1")
    ap.add_argument("--parent-tree", default=None, help="mode a: a built checkout of the parent commit, for the `off` runs")
    ap.add_argument("--repeats", type=int, default=2, help="mode a: parent/this pairs")
    ap.add_argument("--step-steps", type=int, default=2000, help="mode a: replayed steps timed per run")
    ap.add_argument("--positions", type=int, default=1024, help="mode b: corpus positions")
    ap.add_argument("--mirror", choices=("on", "off"), default="on", help="mode steps")
    ap.add_argument("--steps", type=int, default=400, help="mode steps")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        job = json.loads(args.child)
        sys.path.insert(0, job["tree_path"])
        mc.emit_result(CHILDREN[args.mode](job))
        return
    out = {"tool": "tools/measure_eval_mirror.py", "mode": args.mode, "runs": []}
    if args.mode == "a":
        if not args.parent_tree or not os.path.isdir(os.path.join(args.parent_tree, "xiangqi-alphazero_amd")):
            sys.exit("--parent-tree: a built checkout of the parent commit is required (the `off` runs are taken on it)")
        trees = {"parent": os.path.abspath(args.parent_tree), "this": ROOT}
        out.update(preset=dict(PRESETS[args.preset], name=args.preset), weights="peaked", order=[])
        jobs = [dict(mode="a", preset=args.preset, tree=tree, tree_path=trees[tree], mirror=m, step_steps=args.step_steps)
                for _ in range(args.repeats) for tree, m in (("parent", "off"), ("this", "on"))]
    elif args.mode == "b":
        jobs = [dict(mode="b", tree="this", tree_path=ROOT, weights=w, channels=128, blocks=6, positions=args.positions)
                for w in ("random", "peaked")]
    else:
        jobs = [dict(mode="steps", tree="this", tree_path=ROOT, preset=args.preset, mirror=args.mirror, steps=args.steps)]
    ok = mc.run_children(__file__, jobs, args.timeout, out, args.out, argv=lambda job: [job["mode"]],
                         cwd=lambda job: job["tree_path"], after_each=summarise if args.mode == "a" else None)
    if "summary" in out:
        print(json.dumps(out["summary"], indent=1))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
