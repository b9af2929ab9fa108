#!/usr/bin/env python3
"""The forced-mate search (hip.mate_search_batch) and the tactics yardstick (tactics.solve_rate): what a call costs, what the node
limit cuts, and how many puzzles a network plus S simulations solves.

    python tools/measure_tactics.py kernel --out profiles/r24_tactics_kernel.json
    python tools/measure_tactics.py solve --puzzles puzzles/ladder_d3_n3.txt --out profiles/r24_tactics_solve.json

kernel  one call over 1024 unfinished corpus positions (tests/golden/corpus.npz, measure_baseline.py's choice): checks only at
        N = 1..5 and all moves at N = 1..--all-moves-max, without a node limit; the time by device events (warmed, the median of
        --repeats calls with the range), the visits and visits per second; hip.alphabeta_batch at depth 2 and 4 on the same
        positions in the same process (they prove the mates of all moves at N = 1 and 2); and how many root moves --limits cut.
solve   the solve rate of a random-init and a peaked 128x6 network on a puzzle file at --sims simulations, with the proven-result
        search off and on, per mate-in, with the binomial standard error.  One child process per (network, simulations, solver)
        under measure_common's runner.  No trained network is measured here.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import measure_common  # noqa: E402


def _positions(n):
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", "corpus.npz"))
    live = np.nonzero(z["done"] == 0)[0]
    idx = live[np.linspace(0, len(live) - 1, n).astype(int)]
    return z["board"][idx], z["side"][idx]


def _timed(call, repeats):
    """-> (the last call's outputs, median / min / max milliseconds by device events) after one warming call."""
    import numpy as np
    import torch
    out = call()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = call()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return out, {"call_ms_median": round(float(np.median(times)), 3), "call_ms_min": round(min(times), 3),
                 "call_ms_max": round(max(times), 3), "repeats": repeats}


def kernel(args):
    import numpy as np
    import torch
    from xiangqi_alphazero_amd import hip
    boards, sides = _positions(args.positions)
    b, s = torch.from_numpy(boards.astype(np.int8)).cuda(), torch.from_numpy(sides.astype(np.int8)).cuda()
    free = 2 ** 32 - 1
    rows, visits = [], {}
    for checks, top in ((True, hip.MATE_MAX_MOVES), (False, args.all_moves_max)):
        for n in range(1, top + 1):
            out, t = _timed(lambda: hip.mate_search_batch(b, s, n, checks, free), args.repeats)
            nodes = out["nodes"].cpu().numpy().view(np.uint32).astype(np.int64)
            visits[(checks, n)] = nodes
            mate = out["mate_in"].cpu().numpy()
            rows.append({"search": "checks only" if checks else "all moves", "max_moves": n, "positions": int(len(boards)),
                         "root_moves": int(out["counts"].to(torch.int64).sum().item()), "visits": int(nodes.sum()),
                         "largest_visits_of_a_root_move": int(nodes.max()), **t,
                         "visits_per_second": round(float(nodes.sum()) / (t["call_ms_median"] * 1e-3), 1),
                         "positions_with_a_mate": int((out["best_mate_in"] > 0).sum().item()),
                         "root_moves_that_mate": int(((mate >= 1) & (mate <= n)).sum()),
                         "status_nonzero": int((out["status"] != 0).sum().item())})
            print(json.dumps(rows[-1]), flush=True)
    for depth in (2, 4):
        out, t = _timed(lambda: hip.alphabeta_batch(b, s, depth), args.repeats)
        nodes = int(out["nodes"].to(torch.int64).sum().item())
        rows.append({"search": "alphabeta_batch", "depth": depth, "positions": int(len(boards)), "nodes": nodes, **t,
                     "nodes_per_second": round(nodes / (t["call_ms_median"] * 1e-3), 1)})
        print(json.dumps(rows[-1]), flush=True)
    cuts = []
    for limit in args.limits:
        for key in ((True, hip.MATE_MAX_MOVES), (False, args.all_moves_max)):
            searched = visits[key] > 0
            cuts.append({"node_limit": limit, "search": "checks only" if key[0] else "all moves", "max_moves": key[1],
                         "root_moves_searched": int(searched.sum()), "root_moves_cut": int((visits[key] > limit).sum())})
    return {"tool": "tools/measure_tactics.py kernel", "timing": "device events around one call", "default_node_limit":
            hip.MATE_DEFAULT_NODE_LIMIT, "rows": rows, "node_limit_cuts": cuts}


def solve_child(job):
    import torch
    from xiangqi_alphazero_amd import model, tactics
    with open(os.path.join(ROOT, job["puzzles"])) as f:
        positions = tactics.puzzles_from_text(f.read())
    labelled = tactics.label(positions["board"], positions["side"], job["max_moves"], job["checks_only"])
    puzzles = tactics.select(labelled, job["max_moves"], 1, unique=False)
    if job["net"] == "peaked":
        net = measure_common.make_net(128, 6)
    else:
        torch.manual_seed(0)
        net = model.XiangqiNet(128, 6)
    res = tactics.solve_rate(net.cuda().eval(), puzzles, job["sims"], solver=job["solver"], seed=job["seed"])
    by = {}
    for m, (count, solved) in res["by_mate_in"].items():
        p = solved / count
        by[str(m)] = {"puzzles": count, "solved": solved, "solve_rate": round(p, 4), "se": round(math.sqrt(p * (1 - p) / count), 4)}
    p = res["solve_rate"]
    measure_common.emit_result({**job, "net": "128x6 " + job["net"], "puzzles": res["puzzles"], "dropped": len(labelled) - len(puzzles),
                                "solved": res["solved"], "optimal": res["optimal"], "solve_rate": round(p, 4),
                                "se": round(math.sqrt(p * (1 - p) / max(res["puzzles"], 1)), 4), "by_mate_in": by,
                                "seconds": round(res["seconds"], 2)})


def solve(args):
    jobs = [dict(puzzles=os.path.relpath(os.path.abspath(args.puzzles), ROOT), net=net, sims=sims, solver=solver, max_moves=args.max_moves,
                 checks_only=not args.all_moves, seed=args.seed)
            for net in args.nets for sims in args.sims for solver in (False, True)]
    out = {"tool": "tools/measure_tactics.py solve", "note": "random-init and peaked synthetic weights only: no trained network"}
    measure_common.run_children(__file__, jobs, args.timeout, out, args.out, argv=lambda job: ["solve"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kernel", "solve"])
    ap.add_argument("--positions", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--all-moves-max", type=int, default=3)
    ap.add_argument("--limits", type=int, nargs="+", default=[1000, 10000, 100000])
    ap.add_argument("--puzzles", default=None)
    ap.add_argument("--nets", nargs="+", default=["random", "peaked"])
    ap.add_argument("--sims", type=int, nargs="+", default=[100, 400])
    ap.add_argument("--max-moves", type=int, default=3)
    ap.add_argument("--all-moves", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    args = measure_common.parse_args(ap, 300)
    if args.child:
        return solve_child(json.loads(args.child))
    t0 = time.time()
    out = {"kernel": kernel, "solve": solve}[args.part](args)
    out["wall_s"] = round(time.time() - t0, 1)
    measure_common.save_json(out, args.out)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
