#!/usr/bin/env python3
"""The fixed alpha-beta opponent (hip.alphabeta_batch, baseline.play_vs_baseline): what a search costs and what a match says.

    python tools/measure_baseline.py kernel --out profiles/r21_baseline_kernel.json
    python tools/measure_baseline.py match --net random --depth 2 --out profiles/r21_baseline_match_random_d2.json
    python tools/measure_baseline.py ladder --out profiles/r21_baseline_ladder.json

kernel  xq_alphabeta_batch at depths 1 to 4 over 1024 corpus positions (tests/golden/corpus.npz, finished games left out): the
        time of one call by device events (the three launches of the call; warmed, the median of --repeats calls), the nodes the
        call reports and nodes per second.
match   one match of --games games (256) at --sims simulations (100) between a 128x6 network and the baseline of --depth:
        --net random (random initialisation) or peaked (weights.make_state_dict(policy_gain=8)); wall time and the result.
ladder  the baselines of depth 1, 2 and 3 against the random player (depth 0), --games games each.
Every part is one process; run the parts one after another, each under its own time limit.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _positions(n):
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", "corpus.npz"))
    live = np.nonzero(z["done"] == 0)[0]
    idx = live[np.linspace(0, len(live) - 1, n).astype(int)]
    return z["board"][idx], z["side"][idx]


def kernel(args):
    import numpy as np
    import torch
    from xiangqi_alphazero_amd import hip
    boards, sides = _positions(args.positions)
    b, s = torch.from_numpy(boards.astype(np.int8)).cuda(), torch.from_numpy(sides.astype(np.int8)).cuda()
    rows = []
    for depth in range(1, hip.AB_MAX_DEPTH + 1):
        out = hip.alphabeta_batch(b, s, depth)              # warm-up: code objects loaded, the allocator holds the buffers
        torch.cuda.synchronize()
        times = []
        for _ in range(args.repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = hip.alphabeta_batch(b, s, depth)
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1))
        nodes = int(out["nodes"].to(torch.int64).sum().item())
        moves = int(out["counts"].to(torch.int64).sum().item())
        ms = float(np.median(times))
        rows.append({"depth": depth, "positions": int(len(boards)), "root_moves": moves, "nodes": nodes,
                     "call_ms_median": round(ms, 3), "call_ms_min": round(min(times), 3), "call_ms_max": round(max(times), 3),
                     "repeats": args.repeats, "nodes_per_second": round(nodes / (ms * 1e-3), 1),
                     "status_nonzero": int((out["status"] != 0).sum().item())})
        print(json.dumps(rows[-1]), flush=True)
    return {"tool": "tools/measure_baseline.py kernel", "timing": "device events around one hip.alphabeta_batch call", "rows": rows}


def _summary(res):
    return {k: res[k] for k in ("depth", "games", "wins", "losses", "draws", "win_rate", "pairs", "win_rate_se", "baseline_nodes")} | {
        "win_rate_ci95": list(res["win_rate_ci95"]), "seconds": round(res["seconds"], 2),
        "mean_plies": round(float(res["game_records"]["n_moves"].mean()), 2),
        "reasons": {str(r): int((res["game_records"]["reason"] == r).sum()) for r in (1, 2, 4)}}


def match(args):
    import torch
    from xiangqi_alphazero_amd import baseline, model, weights
    net = model.XiangqiNet(128, 6)
    if args.net == "peaked":
        net.load_state_dict(weights.make_state_dict(128, 6, seed=0, policy_gain=8.0))
    else:
        torch.manual_seed(0)
        net = model.XiangqiNet(128, 6)
    res = baseline.play_vs_baseline(net.cuda().eval(), args.games, args.depth, args.sims, opening_plies=4, seed=args.seed)
    torch.cuda.synchronize()
    return {"tool": "tools/measure_baseline.py match", "net": "128x6 " + args.net, "simulations": args.sims, "seed": args.seed,
            "result": _summary(res)}


def ladder(args):
    import torch
    from xiangqi_alphazero_amd import baseline
    rows = []
    for depth in (1, 2, 3):
        res = baseline.play_vs_baseline(depth, args.games, 0, 0, opening_plies=4, seed=args.seed)
        torch.cuda.synchronize()
        rows.append({"seat": f"depth {depth}", "against": "depth 0 (uniformly random)", **_summary(res)})
        print(json.dumps(rows[-1]), flush=True)
    return {"tool": "tools/measure_baseline.py ladder", "seed": args.seed, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kernel", "match", "ladder"])
    ap.add_argument("--positions", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--net", choices=("random", "peaked"), default="random")
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    t0 = time.time()
    out = {"kernel": kernel, "match": match, "ladder": ladder}[args.part](args)
    out["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
