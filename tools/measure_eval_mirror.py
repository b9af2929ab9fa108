#!/usr/bin/env python3
"""Evaluation mirror (engine.SelfPlayEngine(eval_mirror=True)): what the mirrored gather costs, and how
asymmetric a network is -- the quantity the option averages away.

    python tools/measure_eval_mirror.py a --parent-tree <dir> --out profiles/r17_eval_mirror_cfg1.json
    python tools/measure_eval_mirror.py b --out profiles/r17_eval_mirror_asymmetry.json
    python tools/measure_eval_mirror.py steps --mirror on|off          (a short eager run, for a kernel trace taken around it)

Every run is a fresh child process under `timeout -k`; the first failing run ends the measurement.

Mode a.  `--parent-tree` is a built checkout of the PARENT commit (its libxq_hip.so in place).  The "off" runs are taken there,
the "on" runs on this tree, alternated parent, this, parent, this ... in one call, each measure_common.off_on_child with the tree
it measures first on sys.path (preset cfg1 = BASELINE configs[1]: 1024 slots x 400 simulations x 128x6, peaked weights,
games_target 1024): games/hour of complete games, and microseconds per replayed step over `--step-steps` graph replays.
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
OPT = dict(job_key="mirror", config_key="eval_random_mirror", engine_kw="eval_mirror", extra=lambda st, steps: {})


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


CHILDREN = {"a": lambda job: mc.off_on_child(job, PRESETS[job["preset"]], OPT), "b": child_b,
            "steps": lambda job: mc.off_on_steps_child(job, PRESETS[job["preset"]], OPT)}


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
    args = mc.parse_args(ap, 400, lambda job: CHILDREN[job["mode"]](job))
    out = {"tool": "tools/measure_eval_mirror.py", "mode": args.mode, "runs": []}
    if args.mode == "a":
        out.update(preset=dict(PRESETS[args.preset], name=args.preset), weights="peaked", order=[])
        jobs = mc.off_on_jobs(args.parent_tree, args.repeats, "mirror", mode="a", preset=args.preset, step_steps=args.step_steps)
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
