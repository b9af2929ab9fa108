"""Leaf batching (leaves_per_step = K) on one GPU: search latency, small / medium self-play throughput, search quality.

    python tools/measure_leaf_batch.py a|b|c|d|trace [--out FILE]

  a  search latency: one position per search (the opening + 8 corpus positions), 128x6, S = 800, random and peaked
     weights (make_state_dict(policy_gain=8)), wall ms per search for K in {1, 4, 8, 16, 32}; steps replayed from a graph
  b  small self-play: the reference's standard_train preset (20 games, 200 sims, 128x6), complete games, K in {1, 4, 8}:
     games/hour, mean leaves per slot-step, collisions
  c  medium self-play: 1024 slots, 400 sims, 128x6 (BASELINE configs[1]), K in {1, 2, 4}: steady-state simulations/s over a
     fixed window of replayed steps after a staggered start (not complete games)
  d  search quality (reported, not gated): 256 corpus positions, peaked weights, S = 200: how often the most-visited root
     move at K = 8 and K = 16 equals the one at K = 1
  trace  a few replayed K = 8 steps of (b)'s configuration, for rocprofv3 --kernel-trace --stats
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from xiangqi_alphazero_amd import engine, evaluator, model, selfplay, weights  # noqa: E402


def _ev(channels, blocks, gain=None):
    net = model.XiangqiNet(channels, blocks)
    kw = {} if gain is None else {"policy_gain": gain}
    net.load_state_dict(weights.make_state_dict(channels, blocks, **kw))
    return evaluator.make_evaluator(net, "cuda", "hip")[0]


def _positions(n):
    import golden_io as G
    from oracle import xq_oracle as O
    d = G.corpus()
    picks = [i for i in range(3, len(d["board"]), max(1, len(d["board"]) // (2 * n))) if not d["done"][i]][:n]
    out = []
    for i in picks:
        g = O.Game()
        for a in d["taken"][i - d["ply"][i]:i]:
            g.make_action(int(a))
        out.append(g)
    return out


def _set(eng, slot, g):
    eng.set_position(slot, g.board, g.current_player, g.move_count, g.no_capture_count, g.history()[-12:])


def _search(eng, games, S, K):
    for s, g in enumerate(games):
        _set(eng, s, g)
    for _ in range(-(-S // K) + 1):
        eng.step()
    while not eng.held():
        for _ in range(4):
            eng.step()


def part_a():
    from oracle import xq_oracle as O
    games = [O.Game()] + _positions(8)
    out = {"what": "MCTS search of ONE position, 128x6, S=800, steps replayed from a HIP graph; wall ms per search "
                   "(set_position .. finished search, synchronised)", "rows": []}
    for wname, gain in (("random", None), ("peaked", 8.0)):
        ev = _ev(128, 6, gain)
        for K in (1, 4, 8, 16, 32):
            eng = engine.SelfPlayEngine(engine.make_config(1, 800, add_noise=False, manual_moves=True), evaluator=ev,
                                        leaves_per_step=K)
            _set(eng, 0, games[0])
            eng.capture_step(warmup=1)
            ms, steps, coll = [], [], []
            for g in games:
                c0, s0 = eng.stats()["collisions"], eng.steps
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _search(eng, [g], 800, K)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
                steps.append(eng.steps - s0)
                coll.append(eng.stats()["collisions"] - c0)
            row = {"weights": wname, "K": K, "ms_per_search": [round(x, 2) for x in ms], "ms_mean": round(float(np.mean(ms)), 2),
                   "steps_mean": float(np.mean(steps)), "collisions_mean": float(np.mean(coll)), "launch": eng.launch_mode}
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
    return out


def _cfg(S, games):
    return types.SimpleNamespace(num_simulations=S, c_puct=1.5, temperature_threshold=20, max_game_length=300,
                                 random_opening_moves=6, enable_resign=True, resign_threshold=-0.9, resign_check_steps=5,
                                 num_games_per_iter=games)


def _derived(st, elapsed, K):
    leaves, lsteps, coll = st["leaves_per_step_sum"], st["leaf_steps"], st["collisions"]
    return {"K": K, "seconds": round(elapsed, 3), "games": st["games_finished"],
            "games_per_hour": round(st["games_finished"] * 3600.0 / elapsed, 1), "steps": st["steps"],
            "sims": st["sims"], "mean_leaves_per_slot_step": round(leaves / lsteps, 3) if lsteps else 1.0,
            "collisions": coll, "collisions_per_leaf_step": round(coll / lsteps, 4) if lsteps else 0.0,
            "collision_rate_per_descent": round(coll / (coll + st["sims"]), 4) if st["sims"] else 0.0,
            "launch": st["launch"], "path": st["path"], "overflow": st["overflow"]}


def part_b():
    net = model.XiangqiNet(128, 6)
    net.load_state_dict(weights.make_state_dict(128, 6))
    out = {"what": "run_games at the reference's standard_train preset: 20 games, 200 sims, 128x6 random weights, complete "
                   "games, steps replayed", "rows": []}
    for K in (1, 4, 8):
        _, _, st, el = selfplay.run_games(net, _cfg(200, 20), 20, "cuda", seed=11, leaves_per_step=K, poll_every=32)
        row = _derived(st, el, K)
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    return out


def part_c(window=300, warm=100):
    ev = _ev(128, 6)
    out = {"what": f"1024 slots, 400 sims, 128x6 (configs[1]), staggered start, {warm} warm-up then {window} timed replayed steps: "
                   "simulations/s (steady state, not complete games)", "rows": []}
    for K in (1, 2, 4):
        cfg = engine.make_config(1024, 400, seed=5, start_stagger=True)
        eng = engine.SelfPlayEngine(cfg, evaluator=ev, leaves_per_step=K)
        eng.capture_step()
        for _ in range(warm):
            eng.step()
        s0 = eng.stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(window):
            eng.step()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        s1 = eng.stats()
        d = {k: s1[k] - s0[k] for k in ("sims", "moves_played", "collisions", "leaves_per_step_sum", "leaf_steps", "rows_evaluated")}
        row = {"K": K, "ms_per_step": round(el * 1e3 / window, 3), "sims_per_s": round(d["sims"] / el, 1),
               "moves_per_s": round(d["moves_played"] / el, 1),
               "mean_leaves_per_slot_step": round(d["leaves_per_step_sum"] / d["leaf_steps"], 3) if d["leaf_steps"] else 1.0,
               "collisions_per_leaf_step": round(d["collisions"] / d["leaf_steps"], 4) if d["leaf_steps"] else 0.0,
               "rows_per_step": round(d["rows_evaluated"] / window, 1), "launch": eng.launch_mode, "overflow": s1["overflow"]}
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    return out


def part_d():
    ev = _ev(128, 6, 8.0)
    games = _positions(256)
    best = {}
    for K in (1, 8, 16):
        eng = engine.SelfPlayEngine(engine.make_config(len(games), 200, add_noise=False, manual_moves=True), evaluator=ev,
                                    leaves_per_step=K)
        eng.capture_step(warmup=0)
        _search(eng, games, 200, K)
        best[K] = [int(np.argmax(eng.read_root(s)["visits"])) for s in range(len(games))]
    n = len(games)
    out = {"what": f"{n} corpus positions, peaked weights (policy_gain=8), 128x6, S=200: share of positions whose most-visited "
                   "root move (first maximum) at K equals K = 1's", "positions": n,
           "agree_k8": round(sum(a == b for a, b in zip(best[1], best[8])) / n, 4),
           "agree_k16": round(sum(a == b for a, b in zip(best[1], best[16])) / n, 4)}
    print(json.dumps(out), flush=True)
    return out


def part_trace():
    net = model.XiangqiNet(128, 6)
    net.load_state_dict(weights.make_state_dict(128, 6))
    ev = evaluator.make_evaluator(net, "cuda", "hip")[0]
    cfg = engine.make_config(20, 200, seed=11, games_target=20, random_opening_moves=6)
    eng = engine.SelfPlayEngine(cfg, evaluator=ev, leaves_per_step=8)
    eng.capture_step()
    for _ in range(40):
        eng.step()
    torch.cuda.synchronize()
    print(json.dumps({"steps": eng.steps, "launch": eng.launch_mode}))
    return {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["a", "b", "c", "d", "trace"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"a": part_a, "b": part_b, "c": part_c, "d": part_d, "trace": part_trace}[a.part]()
    res["device"] = torch.cuda.get_device_name(0)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
