#!/usr/bin/env python3
"""The table as opponent and teacher (hip.tb_play_batch, hip.tb_samples, endgame.play_out): what a call costs beside the probe,
how many won endings a network plus S simulations converts against the table's best defence, and what a few epochs on table
samples change.

    python tools/measure_endgame_playout.py time --out profiles/r26_tb_play_time.json
    python tools/measure_endgame_playout.py playout --out profiles/r26_tb_play_playout.json
    python tools/measure_endgame_playout.py teach --out profiles/r26_tb_play_teach.json

time     per --signatures table: tb_probe_batch with every output, tb_play_batch (the table choosing) and tb_samples over the
         same --positions random valid entries in one process, by device events (warmed, the median of --repeats calls; every
         call allocates its outputs inside the span, as the probe's figure of make_tablebase.py --time does).
playout  endgame.play_out of a random-init and a peaked 128x6 network on --positions won entries (seed 0, the entries of
         make_tablebase.py --hold) of every --signatures table at every --sims; one child per row under measure_common's runner.
teach    a random-init 128x6 network scored by endgame.play_out before and after --epochs epochs over --samples table samples of
         the signature (training.train_network on a ReplayBuffer of Tablebase.samples rows); one child.
Synthetic and freshly taught weights only: no trained network is measured here."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import measure_common  # noqa: E402
from measure_tactics import _timed  # noqa: E402


def time_part(args):
    import numpy as np
    import torch
    from xiangqi_alphazero_amd import endgame, hip
    rows = []
    for sig in args.signatures:
        table = hip.tb_generate(sig, "cuda")[0]
        pool = np.nonzero(table.cpu().numpy() != hip.TB_INVALID)[0]
        pick = np.sort(np.random.default_rng(args.seed).choice(pool, size=min(args.positions, len(pool)), replace=False))
        boards, sides = endgame.index_to_board(sig, pick)
        b, s, idx = torch.from_numpy(boards).cuda(), torch.from_numpy(sides).cuda(), torch.from_numpy(pick.astype(np.int32)).cuda()
        row = {"signature": sig, "entries": int(len(table)), "positions": int(len(pick))}
        for name, call in (("probe", lambda: hip.tb_probe_batch(sig, table, b, s)), ("play", lambda: hip.tb_play_batch(sig, table, b, s)),
                           ("samples", lambda: hip.tb_samples(sig, table, idx))):
            row[name] = _timed(call, args.repeats)[1]
        for name in ("play", "samples"):
            row[name + "_over_probe"] = round(row[name]["call_ms_median"] / row["probe"]["call_ms_median"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return {"tool": "tools/measure_endgame_playout.py time", "timing": "device events around one call, outputs allocated inside",
            "rows": rows}


def _net(name):
    import torch
    from xiangqi_alphazero_amd import model
    if name == "peaked":
        return measure_common.make_net(128, 6).cuda().eval()
    torch.manual_seed(0)
    return model.XiangqiNet(128, 6).cuda().eval()


def _row(res):
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items() if k != "games"}


def child(job):
    from xiangqi_alphazero_amd import endgame
    tb = endgame.Tablebase.generate(job["signature"], "cuda")
    boards, sides, _ = tb.entries_of(("win",), min(job["positions"], int((tb.table > 0).sum())), seed=job["seed"])
    net = _net(job["net"])
    if job["part"] == "playout":
        res = endgame.play_out(net, tb, boards, sides, job["sims"], max_plies=job["max_plies"], seed=job["seed"])
        return measure_common.emit_result({**job, "net": "128x6 " + job["net"], **_row(res)})
    import types
    import torch
    from xiangqi_alphazero_amd import training
    before = endgame.play_out(net, tb, boards, sides, job["sims"], max_plies=job["max_plies"], seed=job["seed"])
    cfg = types.SimpleNamespace(num_epochs=job["epochs"], batch_size=256, min_buffer_size=0, learning_rate=0.002, weight_decay=1e-4)
    have = int(((tb.table != -1) & (tb.table != endgame.INVALID)).sum())
    buf = training.ReplayBuffer(2 * job["samples"], "cuda")
    buf.extend(tb.samples(tb.entries_of(n=min(job["samples"], have), seed=job["seed"] + 1)[2], as_tensor=True))
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=cfg.learning_rate, weight_decay=cfg.weight_decay)
    t0 = time.time()
    tr = training.train_network(net, opt, training._ConstantRate(), buf, cfg)
    after = endgame.play_out(net.eval(), tb, boards, sides, job["sims"], max_plies=job["max_plies"], seed=job["seed"])
    measure_common.emit_result({**job, "net": "128x6 random", "records": buf.count, "train_seconds": round(time.time() - t0, 1),
                                "training": tr, "before": _row(before), "after": _row(after)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["time", "playout", "teach"])
    ap.add_argument("--signatures", nargs="+", default=None)
    ap.add_argument("--positions", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nets", nargs="+", default=["random", "peaked"])
    ap.add_argument("--sims", type=int, nargs="+", default=[100, 400])
    ap.add_argument("--max-plies", type=int, default=100)
    ap.add_argument("--samples", type=int, default=8192)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    args = measure_common.parse_args(ap, 500)
    if args.child:
        return child(json.loads(args.child))
    t0 = time.time()
    sigs = args.signatures or {"time": ["Ra", "RNa", "Raabb"], "playout": ["R", "CA"], "teach": ["R"]}[args.part]
    n = args.positions or (1 << 16 if args.part == "time" else 1024)
    if args.part == "time":
        args.signatures, args.positions = sigs, n
        out = time_part(args)
    else:
        common = dict(part=args.part, positions=n, max_plies=args.max_plies, seed=args.seed)
        if args.part == "playout":
            jobs = [dict(common, signature=g, net=net, sims=s) for g in sigs for net in args.nets for s in args.sims]
        else:
            jobs = [dict(common, signature=g, net="random", sims=args.sims[0], samples=args.samples, epochs=args.epochs) for g in sigs]
        out = {"tool": "tools/measure_endgame_playout.py " + args.part,
               "note": "random-init, peaked synthetic and freshly taught weights only: no trained network"}
        measure_common.run_children(__file__, jobs, args.timeout, out, args.out, argv=lambda job: [job["part"]])
    out["wall_s"] = round(time.time() - t0, 1)
    measure_common.save_json(out, args.out)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
