#!/usr/bin/env python3
"""Game records (engine.SelfPlayEngine(record_games=True)) against the engine without them and against the parent commit: what
the option costs.  Complete games through run_games on peaked weights with one seed, the kinds of run alternated, each run in a
fresh child process under `timeout -k`; the first failing run ends the measurement.

    python tools/measure_game_records.py games --preset cfg1 --parent-tree <checkout of the parent commit, library built> \\
        --out profiles/r18_game_records_cfg1.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_game_records.py trace --records 0
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_game_records.py trace --records 1
    python tools/measure_game_records.py spread --stats off=<csv>,<csv>,<csv> on=<csv>,... parent=<csv>,... --out <json>

Presets: cfg1 = BASELINE configs[1] (1024 slots x 400 sims x 128x6, games_target 1024); small = 256 slots x 64 sims x 64x2 (a
quick look).  Kinds of run: `parent` (the parent commit's tree, given by --parent-tree: its own Python and its own library; it
has no option), `off` (this tree, the option off) and `on`.  Per run: games/hour, samples/hour, steps, mean game length, and for
`on` the records' own counts, the share of games each reason ended and the mean opening length -- the first figures the records
make available.  The summary gives every kind's runs with its own run-to-run spread and says whether `off` lies within the
parent's spread and `on` within it as well.
`trace` runs replayed steps at a preset from a staggered start for a kernel trace; `spread` reads the `*_kernel_stats.csv` files of
several such traces and writes the mean time per launch of k_select (and of k_flush_records, which only `on` launches) for every
run with each group's own spread.
"""
import argparse
import csv
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


def _net(channels, blocks, seed=0):
    from xiangqi_alphazero_amd import model, weights
    net = model.XiangqiNet(channels, blocks)
    net.load_state_dict(weights.make_state_dict(channels, blocks, seed=seed, policy_gain=PEAKED_GAIN))
    return net


def child_games(job):
    import numpy as np
    import torch
    from xiangqi_alphazero_amd import selfplay
    p = PRESETS[job["preset"]]
    cfg = types.SimpleNamespace(num_simulations=p["sims"], c_puct=1.5, temperature_threshold=p["temperature_threshold"],
                                max_game_length=p["max_game_length"], random_opening_moves=p["random_opening_moves"],
                                enable_resign=True, resign_threshold=-0.9, resign_check_steps=5)
    if job["kind"] == "on":
        cfg.record_games = True                          # through the config key, as a training loop sets it
    samples, results, st, elapsed = selfplay.run_games(_net(p["channels"], p["blocks"]), cfg, p["games"], "cuda", n_slots=p["slots"],
                                                       seed=11, poll_every=64 if p["slots"] < 64 else 256)
    torch.cuda.synchronize()
    row = {"preset": job["preset"], "kind": job["kind"], "path": st["path"], "launch": st["launch"], "games": int(len(results)),
           "samples": int(len(samples)), "wall_s": round(elapsed, 2), "games_per_hour": round(len(results) * 3600.0 / elapsed, 1),
           "samples_per_hour": round(len(samples) * 3600.0 / elapsed, 1), "steps": int(st["steps"]),
           "mean_plies": round(float(results["steps"].mean()), 2), "moves": int(st["moves_played"]), "sims": int(st["sims"]),
           "overflow": int(st["overflow"])}
    if job["kind"] == "on":
        rec = st["game_records"]
        row.update(records=int(len(rec)), recorded=int(st["game_records_recorded"]), dropped=int(st["game_records_dropped"]),
                   mean_opening_plies=round(float(rec["opening_plies"].mean()), 3),
                   reasons={str(r): int((rec["reason"] == r).sum()) for r in (1, 2, 3, 4)},
                   moves_in_records=int(rec["n_moves"].astype(np.int64).sum()))
    return row


def trace(preset, records, steps):
    import torch
    from xiangqi_alphazero_amd import engine, evaluator
    c = PRESETS[preset]
    ev = evaluator.make_evaluator(_net(c["channels"], c["blocks"]), "cuda", "hip")[0]
    cfg = engine.make_config(c["slots"], c["sims"], seed=5, start_stagger=True, max_out_samples=c["slots"] * 16)
    kw = {"record_games": True} if records else {}     # records 0 also runs on a tree without the option (the parent commit's)
    eng = engine.SelfPlayEngine(cfg, evaluator=ev, **kw)
    assert eng.capture_step()
    t0 = time.time()
    for i in range(steps):
        eng.step()
        if i % 256 == 255:
            eng.drain_device()
            if records:
                eng.drain_games_device()
    torch.cuda.synchronize()
    st = eng.stats()
    print(json.dumps({"preset": preset, "records": bool(records), "steps": eng.steps, "launch": eng.launch_mode,
                      "wall_s": round(time.time() - t0, 1), "moves": st["moves_played"], "sims": st["sims"],
                      "games_finished": st["games_finished"], "overflow": st["overflow"]}), flush=True)


def _mean_us(path, want, without=()):
    """Mean time per launch of the kernels whose name holds `want` in a rocprofv3 `*_kernel_stats.csv` (calls-weighted), in
    microseconds; None when there is no such launch."""
    calls = total = 0
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if want in row["Name"] and not any(w in row["Name"] for w in without):
                calls += int(row["Calls"])
                total += float(row["TotalDurationNs"])
    return round(total / calls / 1000.0, 3) if calls else None


def _group(runs):
    runs = [r for r in runs if r is not None]
    if not runs:
        return None
    return {"runs": runs, "min": min(runs), "max": max(runs), "spread": round(max(runs) - min(runs), 3),
            "mean": round(sum(runs) / len(runs), 3)}


def spread(groups, out_path):
    out = {"tool": "tools/measure_game_records.py spread", "unit": "microseconds per launch, mean of a run", "k_select": {},
           "k_flush_records": {}}
    for spec in groups:
        name, files = spec.split("=", 1)
        out["k_select"][name] = _group([_mean_us(p, "k_select", ("k_select_multi",)) for p in files.split(",")])
        out["k_flush_records"][name] = _group([_mean_us(p, "k_flush_records") for p in files.split(",")])
    g = out["k_select"]
    for kind in ("off", "on"):
        if g.get(kind) and g.get("parent"):
            out[f"{kind}_within_parent_spread"] = g["parent"]["min"] <= g[kind]["mean"] <= g["parent"]["max"]
    print(json.dumps(out, indent=1))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


def summarise(rows):
    out = {}
    for kind in ("parent", "off", "on"):
        out[kind] = _group([r["games_per_hour"] for r in rows if r["kind"] == kind])
    p = out.get("parent")
    for kind in ("off", "on"):
        if p and out.get(kind):
            out[f"{kind}_within_parent_spread"] = p["min"] <= out[kind]["mean"] <= p["max"]
            out[f"{kind}_over_parent_mean"] = round(out[kind]["mean"] / p["mean"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["games", "trace", "spread"])
    ap.add_argument("--preset", choices=sorted(PRESETS), default="cfg1")
    ap.add_argument("--runs", choices=("parent", "off", "on"), nargs="*", default=["parent", "off", "on"] * 3)
    ap.add_argument("--parent-tree", default=None, help="games: a checkout of the parent commit with its library built")
    ap.add_argument("--records", type=int, default=1, help="trace: 1 = game records on, 0 = the engine without the option")
    ap.add_argument("--steps", type=int, default=700, help="trace: replayed steps")
    ap.add_argument("--stats", nargs="*", default=[], help="spread: name=<kernel_stats.csv>,<kernel_stats.csv>,... per group")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.part == "spread":
        spread(args.stats, args.out)
        return
    # a child of a `parent` run imports the parent commit's package: its Python goes with its library
    tree = json.loads(args.child).get("tree") if args.child else None
    sys.path.insert(0, tree or ROOT)
    if args.part == "trace":
        trace(args.preset, args.records, args.steps)
        return
    if args.child:
        print("RESULT " + json.dumps(child_games(json.loads(args.child))), flush=True)
        return
    if "parent" in args.runs and not args.parent_tree:
        sys.exit("runs of kind `parent` need --parent-tree")
    out = {"tool": "tools/measure_game_records.py games", "preset": dict(PRESETS[args.preset], name=args.preset), "weights": "peaked",
           "runs": []}
    for kind in args.runs:
        job = dict(preset=args.preset, kind=kind, tree=os.path.abspath(args.parent_tree) if kind == "parent" else None)
        t0 = time.time()
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "games", "--child", json.dumps(job)]
        r = subprocess.run(cmd, cwd=job["tree"] or ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = next((x for x in r.stdout.splitlines() if x.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(r.stdout[-3000:], file=sys.stderr)
            print(f"child failed (exit {r.returncode}) on {job}: stopping", file=sys.stderr)
            out["failed"] = dict(job=job, exit=r.returncode)
            break
        row = json.loads(line[7:])
        row["child_wall_s"] = round(time.time() - t0, 1)
        print(json.dumps(row), flush=True)
        out["runs"].append(row)
        out["summary"] = summarise(out["runs"])
        if args.out:                                     # after every run: a measurement cut short keeps what it has
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
    print(json.dumps(out.get("summary", {}), indent=1))
    sys.exit(1 if "failed" in out else 0)


if __name__ == "__main__":
    main()
