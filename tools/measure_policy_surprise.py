#!/usr/bin/env python3
"""What the scoring pass (selfplay.score_samples) and policy-surprise weighted epochs cost, measured on the GPU.  Every part runs
in fresh child processes, each under `timeout -k` with a limit of its own; the first failing child ends the measurement.

    python tools/measure_policy_surprise.py pass --preset cfg1 --out profiles/r19_policy_surprise_pass_cfg1.json
    python tools/measure_policy_surprise.py pass --preset standard_train --out profiles/r19_policy_surprise_pass_standard_train.json
    python tools/measure_policy_surprise.py kernels --out profiles/r19_policy_surprise_kernels.json
    python tools/measure_policy_surprise.py train --parent-tree <checkout of the parent commit, library built> \\
        --out profiles/r19_policy_surprise_train_step.json

`pass`: complete games through run_games on peaked weights (make_state_dict(policy_gain=8)) at a preset -- cfg1 = BASELINE
configs[1] (1024 slots x 400 sims x 128x6), standard_train = the reference's preset (20 games x 200 sims x 128x6), small = a quick
look -- then the scoring pass over the samples those games produced with the evaluator of the same network, for chunks of 256,
1024 and 4096: samples/s (a host clock around work that ends in a device synchronise, after one warm-up pass per chunk size; the
samples are repeated up to at least 16384 rows so that the window is not a toy) and the pass's share of the self-play time of the
same games.  From the same scores: the KL quantiles, the largest weight w_i at alpha = 0.5 and 1, and the share of an epoch's
draws that go to the tenth of the records with the largest KL.
`kernels`: the gather and the score kernel alone, 131072 rows per launch (past the Infinity Cache), device events around 20
back-to-back launches after 3 warm-up launches: time per launch, the bytes the kernel must move (computed from the shapes: 640 B
read and 5660 B written per row for the gather; 6 m + 6 read and 16 or 24 written for the score, whose launches rotate over
four sets of buffers, 600 MB in all, so that the cache does not serve them), the rate, and its share of the HBM peak (8 TB/s).  The counts call at the same size rides along with its time alone.
`train`: the train step (128x6, batch 256, 4096 logical samples, --epochs epochs timed after a warm-up epoch) at policy_surprise_weight = 0
on this tree and on the parent commit's tree (which has no option), alternated; the summary says whether this tree's mean lies
inside the parent's own spread -- the two are meant to be the same code.
Whether a network trained with alpha > 0 is stronger is not measured here: that takes arena matches over trained networks
(tools/measure_arena.py).
"""
import argparse
import json
import os
import sys
import time
import types

import measure_common as mc
from measure_common import ROOT

PEAKED_GAIN = mc.GAINS["peaked"]
HBM_PEAK_TBS = 8.0
PRESETS = dict(mc.PRESETS, small=dict(mc.PRESETS["small"], slots=64, games=64, sims=32, max_game_length=60))
CHUNKS = (256, 1024, 4096)


def _play(p, seed=11):
    from xiangqi_alphazero_amd import selfplay
    net = mc.make_net(p["channels"], p["blocks"])
    samples, results, st, elapsed = selfplay.run_games(net, mc.selfplay_config(p), p["games"], "cuda", n_slots=p["slots"],
                                                       seed=seed, poll_every=mc.poll_every(p), device_records=True)
    return net, samples, results, st, elapsed


def child_pass(job):
    import numpy as np
    import torch
    from xiangqi_alphazero_amd import evaluator, selfplay
    from xiangqi_alphazero_amd import sample_format as F
    p = PRESETS[job["preset"]]
    net, samples, results, st, elapsed = _play(p)
    torch.cuda.synchronize()
    n = int(samples.shape[0])
    ev = evaluator.make_evaluator(net, "cuda", "hip")[0]
    rows = samples.repeat((16384 + n - 1) // n, 1) if n < 16384 else samples
    out = {"preset": job["preset"], "games": int(results.shape[0]), "samples": n, "selfplay_wall_s": round(elapsed, 2),
           "path": st["path"], "launch": st["launch"], "rows_timed": int(rows.shape[0]), "chunks": {}}
    for chunk in CHUNKS:
        selfplay.score_samples(ev, rows, write_back=False, chunk=chunk)      # warm-up: buffers, code objects
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        selfplay.score_samples(ev, rows, write_back=False, chunk=chunk)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rate = rows.shape[0] / dt
        out["chunks"][str(chunk)] = {"samples_per_s": round(rate, 1), "window_s": round(dt, 3),
                                     "pass_s_for_these_games": round(n / rate, 4),
                                     "share_of_selfplay_time": round(n / rate / elapsed, 6)}
    scores = selfplay.score_samples(ev, samples, write_back=True)
    torch.cuda.synchronize()
    out["summary"] = selfplay.score_summary(scores, samples)
    rec = samples.cpu().numpy().reshape(-1).view(F.SAMPLE_DTYPE)
    kl = F.policy_stats(rec)["policy_kl"].astype(np.float64)
    out["kl_quantiles"] = {str(q): round(float(np.quantile(kl, q)), 6) for q in (0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0)}
    top = kl >= np.quantile(kl, 0.9)
    out["weights"] = {}
    for alpha in (0.5, 1.0):
        w, marked, M, S = F.surprise_weights(rec, alpha)
        c = F.surprise_counts(rec, alpha, 12345, 0)
        out["weights"][str(alpha)] = {"largest_w": round(float(w.max()), 4), "marked": int(M), "epoch_draws": int(c.sum()),
                                      "records_never_drawn": int((c == 0).sum()),
                                      "share_of_draws_to_top_kl_decile": round(float(c[top].sum() / max(c.sum(), 1)), 4)}
    return out


def child_kernels(job):
    import torch
    from xiangqi_alphazero_amd import hip
    n = int(job.get("rows", 131072))
    net, samples, _, _, _ = _play(PRESETS["small"])
    rows = samples.repeat((n + samples.shape[0] - 1) // samples.shape[0], 1)[:n].contiguous()
    x = torch.empty((n, 15, 10, 9), dtype=torch.float32, device="cuda")
    moves = torch.empty((n, 128), dtype=torch.int16, device="cuda")
    counts = torch.empty(n, dtype=torch.int32, device="cuda")
    logits = torch.randn((n, 128), device="cuda")
    value = torch.zeros(n, device="cuda")
    scores = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
    mean_m = float(rows[:, 92].float().mean().item())                       # byte 92: n_moves

    def timed(fn, launches=20):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches * 1e-3

    def row(seconds, bytes_per_row):
        rate = n * bytes_per_row / seconds / 1e12
        return {"us_per_launch": round(seconds * 1e6, 2), "bytes_per_row": round(bytes_per_row, 1), "tb_per_s": round(rate, 3),
                "share_of_hbm_peak": round(rate / HBM_PEAK_TBS, 4)}

    out = {"rows_per_launch": n, "mean_moves_per_row": round(mean_m, 2), "hbm_peak_tb_per_s": HBM_PEAK_TBS,
           "timing": "device events around 20 back-to-back launches after 3 warm-up launches"}
    out["k_samples_to_requests"] = row(timed(lambda: hip.samples_to_requests(rows, None, out=(x, moves, counts))), 640 + 5400 + 256 + 4)
    # the score kernel's inputs of one launch (84 MB of records, 67 MB of logits) fit the 256 MB Infinity Cache: the launches rotate
    # over four sets, 600 MB in all, so that no launch finds its inputs there.  Bytes asked for per row: n_moves and late_temp, 2 m
    # of visits, 4 m of logits, the value; 16 written (24 with write-back).  Board and actions are never read.
    sets = [(rows.clone(), torch.randn((n, 128), device="cuda"), value.clone(), scores.clone()) for _ in range(4)]
    turn = [0]

    def score(write_back):
        r, lg, v, sc = sets[turn[0] % len(sets)]
        turn[0] += 1
        hip.score_samples(r, None, lg, v, 0.3, write_back, out=sc)

    out["score_kernel_buffers"] = "20 launches rotate over 4 sets of records, logits, value and scores (600 MB in all)"
    out["k_score_samples"] = row(timed(lambda: score(False)), 2 + 6 * mean_m + 4 + 16)
    out["k_score_samples_write_back"] = row(timed(lambda: score(True)), 2 + 6 * mean_m + 4 + 24)
    # the counts read 8 + 18 bytes of every 640-byte record and write 4: a time, and no bandwidth figure (the fetched sectors are
    # a multiple of the bytes asked for)
    out["xq_surprise_counts (memset + two kernels)"] = {"us_per_call": round(timed(lambda: hip.surprise_counts(rows, 0.5, 1, 0)) * 1e6, 2)}
    return out


def child_train(job):
    import torch
    from xiangqi_alphazero_amd import selfplay, training
    cfg = mc.selfplay_config(dict(sims=16, temperature_threshold=20, max_game_length=120, random_opening_moves=8),
                             enable_resign=False)
    samples, _, _, _ = selfplay.run_games(mc.make_net(64, 3, mc.GAINS["random"]), cfg, 64, "cuda", seed=5)
    buf = training.ReplayBuffer(10 ** 6, "cuda")
    buf.extend(samples[:2048])
    net = mc.make_net(128, 6, mc.GAINS["random"]).cuda()
    net.use_native_conv(True)
    opt = torch.optim.Adam(net.parameters(), lr=2e-3, weight_decay=1e-4, fused=True)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[50, 80], gamma=0.1)
    tcfg = types.SimpleNamespace(min_buffer_size=1, num_epochs=1, batch_size=256)
    kw = {} if job["kind"] == "parent" else {"surprise_weight": 0.0}
    g = torch.Generator().manual_seed(3)
    training.train_network(net, opt, sch, buf, tcfg, generator=g, **kw)     # warm-up epoch (allocator, library algorithm search)
    torch.cuda.synchronize()
    tcfg.num_epochs = epochs = int(job.get("epochs", 12))
    t0 = time.perf_counter()
    stats = training.train_network(net, opt, sch, buf, tcfg, generator=g, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"kind": job["kind"], "buffer_samples": len(buf), "epochs_timed": epochs, "samples_per_s": round(epochs * len(buf) / dt, 1), "window_s": round(dt, 3),
            "policy_loss": stats["policy_loss"], "value_loss": stats["value_loss"]}


CHILDREN = {"pass": child_pass, "kernels": child_kernels, "train": child_train}


def summarise(out, job, row):
    g = out["summary"] = {k: mc.group([x["samples_per_s"] for x in out["runs"] if x["kind"] == k]) for k in ("parent", "this")}
    if g["parent"] and g["this"]:
        g["this_within_parent_spread"] = mc.within_spread(g["parent"], g["this"])
        g["this_over_parent_mean"] = round(g["this"]["mean"] / g["parent"]["mean"], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=sorted(CHILDREN))
    ap.add_argument("--preset", choices=sorted(PRESETS), default="cfg1")
    ap.add_argument("--rows", type=int, default=131072, help="kernels: rows per launch")
    ap.add_argument("--runs", choices=("parent", "this"), nargs="*", default=["parent", "this"] * 3, help="train: the alternation")
    ap.add_argument("--epochs", type=int, default=12, help="train: epochs in the timed window")
    ap.add_argument("--parent-tree", default=None, help="train: a checkout of the parent commit with its library built")
    args = mc.parse_args(ap, 300)
    if args.child:                                       # a child of a `parent` run imports the parent commit's package
        job = json.loads(args.child)
        sys.path.insert(0, job.get("tree") or ROOT)
        import torch
        if not torch.cuda.is_available():
            sys.exit("no GPU: nothing here is measured without one")
        mc.emit_result(CHILDREN[args.part](job))
        return
    if args.part == "train":
        if "parent" in args.runs and not args.parent_tree:
            sys.exit("runs of kind `parent` need --parent-tree")
        jobs = [dict(kind=k, epochs=args.epochs, tree=os.path.abspath(args.parent_tree) if k == "parent" else None) for k in args.runs]
    else:
        jobs = [dict(preset=args.preset, rows=args.rows)]
    out = {"tool": "tools/measure_policy_surprise.py " + args.part, "weights": "peaked (policy_gain %g)" % PEAKED_GAIN, "runs": []}
    ok = mc.run_children(__file__, jobs, args.timeout, out, args.out, argv=lambda job: [args.part],
                         cwd=lambda job: job.get("tree") or ROOT, after_each=summarise if args.part == "train" else None)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
