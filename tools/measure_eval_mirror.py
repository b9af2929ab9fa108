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
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAKED_GAIN = 8.0
PRESETS = {
    "cfg1": dict(slots=1024, games=1024, sims=400, channels=128, blocks=6, temperature_threshold=20, max_game_length=400,
                 random_opening_moves=8),
    "small": dict(slots=256, games=256, sims=64, channels=64, blocks=2, temperature_threshold=20, max_game_length=120,
                  random_opening_moves=6),
}


def _net(channels, blocks, peaked=True, seed=0):
    from xiangqi_alphazero_amd import model, weights
    net = model.XiangqiNet(channels, blocks)
    kw = dict(policy_gain=PEAKED_GAIN) if peaked else {}
    net.load_state_dict(weights.make_state_dict(channels, blocks, seed=seed, **kw))
    return net


def child_a(job):
    import torch
    from xiangqi_alphazero_amd import engine, evaluator, selfplay
    p = PRESETS[job["preset"]]
    on = job["mirror"] == "on"
    net = _net(p["channels"], p["blocks"])
    cfg = types.SimpleNamespace(num_simulations=p["sims"], c_puct=1.5, temperature_threshold=p["temperature_threshold"],
                                max_game_length=p["max_game_length"], random_opening_moves=p["random_opening_moves"],
                                enable_resign=True, resign_threshold=-0.9, resign_check_steps=5)
    if on:
        cfg.eval_random_mirror = True                  # through the config key, as a training loop sets it
    samples, results, st, elapsed = selfplay.run_games(net, cfg, p["games"], "cuda", n_slots=p["slots"], seed=11, poll_every=256)
    torch.cuda.synchronize()
    assert bool(st.get("eval_mirror", False)) == on and int(st["overflow"]) == 0
    row = {"preset": job["preset"], "tree": job["tree"], "eval_mirror": on, "path": st["path"], "launch": st["launch"],
           "games": int(len(results)), "samples": int(len(samples)), "wall_s": round(elapsed, 2),
           "games_per_hour": round(len(results) * 3600.0 / elapsed, 1), "mean_plies": round(float(results["steps"].mean()), 2),
           "moves": int(st["moves_played"]), "sims": int(st["sims"]), "steps": int(st["steps"]),
           "rows_evaluated": int(st["rows_evaluated"])}
    # the replayed step from a staggered start: one graph launch per step between two device events
    ev = evaluator.make_evaluator(net, "cuda", "hip")[0]
    ecfg = engine.make_config(p["slots"], p["sims"], seed=5, start_stagger=True, max_out_samples=p["slots"] * 16)
    eng = engine.SelfPlayEngine(ecfg, evaluator=ev, **({"eval_mirror": True} if on else {}))
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
    net = _net(job["channels"], job["blocks"], peaked=job["weights"] == "peaked")
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
    import torch
    from xiangqi_alphazero_amd import engine, evaluator
    p = PRESETS[job["preset"]]
    on = job["mirror"] == "on"
    ev = evaluator.make_evaluator(_net(p["channels"], p["blocks"]), "cuda", "hip")[0]
    cfg = engine.make_config(p["slots"], p["sims"], seed=5, start_stagger=True, max_out_samples=p["slots"] * 64)
    eng = engine.SelfPlayEngine(cfg, evaluator=ev, **({"eval_mirror": True} if on else {}))
    for i in range(int(job["steps"])):
        eng.step()
        if i % 256 == 255:
            eng.drain_device()
    torch.cuda.synchronize()
    st = eng.stats()
    assert int(st["overflow"]) == 0
    return {"eval_mirror": on, "steps": int(job["steps"]), "rows_evaluated": int(st["rows_evaluated"]), "slots": p["slots"],
            "preset": job["preset"]}


CHILDREN = {"a": child_a, "b": child_b, "steps": child_steps}


def _group(rows, key):
    v = [r[key] for r in rows]
    return {"runs": v, "min": min(v), "max": max(v), "mean": round(sum(v) / len(v), 3), "spread": round(max(v) - min(v), 3)}


def _run_child(job, cwd, timeout):
    t0 = time.time()
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__), job["mode"], "--child", json.dumps(job)]
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    line = next((l for l in r.stdout.splitlines() if l.startswith("RESULT ")), None)
    if r.returncode != 0 or line is None:
        print(r.stdout[-3000:], file=sys.stderr)
        print(f"child failed (exit {r.returncode}) on {job}: stopping", file=sys.stderr)
        return None, r.returncode
    row = json.loads(line[7:])
    row["child_wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(row), flush=True)
    return row, 0


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
        print("RESULT " + json.dumps(CHILDREN[args.mode](job)), flush=True)
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
    for job in jobs:
        row, rc = _run_child(job, job["tree_path"], args.timeout)
        if row is None:
            out["failed"] = dict(job=job, exit=rc)
            break
        out["runs"].append(row)
        if args.mode == "a":
            out["order"].append(job["tree"])
    if args.mode == "a":
        par, this = [r for r in out["runs"] if r["tree"] == "parent"], [r for r in out["runs"] if r["tree"] == "this"]
        if par and this:
            out["summary"] = {}
            for key in ("games_per_hour", "step_us_mean", "step_us_median"):
                p, t = _group(par, key), _group(this, key)
                out["summary"][key] = {"parent_off": p, "this_on": t, "delta_of_means": round(t["mean"] - p["mean"], 3),
                                       "margin_parent_spread": p["spread"],
                                       "within_margin": abs(t["mean"] - p["mean"]) <= p["spread"]}
            print(json.dumps(out["summary"], indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    sys.exit(1 if "failed" in out else 0)


if __name__ == "__main__":
    main()
