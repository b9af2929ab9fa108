#!/usr/bin/env python3
"""Game records as training samples (hip.records_to_samples, training.pretrain_from_records): what the conversion costs and what
a supervised warm start on baseline games buys against the baseline.

    python tools/measure_pretrain.py kernel --out profiles/r23_supervise_kernel.json
    python tools/measure_pretrain.py strength --out profiles/r23_supervise_strength.json

kernel    --records ladder games (1024), depth 3 against depth 3: device events around xq_records_sample_counts, the prefix sum
          and xq_records_to_samples (every ply selected; buffers allocated beforehand, no host synchronisation inside), and around
          xq_replay_games_batch with every output on the same records, the two calls alternated; warmed, the median of --repeats
          calls with minimum and maximum; samples per second and bytes written per second against the HBM peak.
strength  a corpus of ladder games (tools/make_baseline_games.py: --depths, --games per match, --opening-plies, --seed), a 128x6
          network of random initialisation (--net-seed), `play_vs_baseline` at --match-games games, --sims simulations and 4 opening
          plies against depths 1, 2 and 3 before and after `pretrain_from_records` (--epochs, --batch, --lr), in this one run.
Every part is one process; run the parts one after another, each under its own time limit.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK_BYTES_PER_S = 8.0e12        # MI355X: 8 TB/s


def _events(fn, repeats):
    import torch
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return times


def _ms(times):
    import numpy as np
    return {"ms_median": round(float(np.median(times)), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4)}


def kernel(args):
    import numpy as np
    import torch
    import make_baseline_games
    from xiangqi_alphazero_amd import hip
    records, matches = make_baseline_games.play([(3, 3)], args.records, 4, args.seed)
    n = len(records)
    rec = torch.from_numpy(records.view(np.uint8).reshape(n, hip.RECORD_BYTES).copy()).cuda()
    first = hip.records_to_samples(rec, 0, None, False, False)              # every ply; also the warm-up
    total = int(first["samples"].shape[0])
    assert total == int(records["n_moves"].sum()) and not first["status"].any().item()
    opts = hip.SuperviseOpts(0, 0, 0, 0)
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    offsets = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    rows = torch.empty((total, hip.SAMPLE_BYTES), dtype=torch.uint8, device="cuda")
    lib, stream = hip.lib(), hip.stream_ptr("cuda")

    def convert():
        hip.check(lib.xq_records_sample_counts(rec.data_ptr(), None, n, C.byref(opts), counts.data_ptr(), stream), "counts")
        offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int32)
        hip.check(lib.xq_records_to_samples(rec.data_ptr(), None, offsets.data_ptr(), n, C.byref(opts), rows.data_ptr(),
                                            status.data_ptr(), stream), "convert")

    o = hip.replay_games(rec)                                               # its outputs, allocated once

    def replay():
        hip.check(lib.xq_replay_games_batch(rec.data_ptr(), None, n, 0, o["board"].data_ptr(), o["side"].data_ptr(),
                                            o["move_count"].data_ptr(), o["no_capture"].data_ptr(), o["hist12"].data_ptr(),
                                            o["status"].data_ptr(), o["over_kind"].data_ptr(), o["winner"].data_ptr(), stream), "replay")

    convert(), replay()
    torch.cuda.synchronize()
    t_convert, t_replay = [], []
    for _ in range(args.repeats):                                            # alternated: both see the same clocks
        t_convert += _events(convert, 1)
        t_replay += _events(replay, 1)
    assert rows.cpu().numpy().tobytes() == first["samples"].cpu().numpy().tobytes()
    ms = float(np.median(t_convert))
    written = total * hip.SAMPLE_BYTES
    return {"tool": "tools/measure_pretrain.py kernel", "timing": "device events; the conversion = counts + cumsum + conversion; "
            "the replay = xq_replay_games_batch with every output; both into buffers allocated beforehand",
            "records": n, "depths": "3:3", "opening_plies": 4, "seed": args.seed, "plies": total, "samples": total,
            "mean_plies": round(total / n, 2), "repeats": args.repeats, "conversion": _ms(t_convert), "replay": _ms(t_replay),
            "conversion_over_replay": round(ms / float(np.median(t_replay)), 3),
            "samples_per_second": round(total / (ms * 1e-3), 1), "bytes_written": written,
            "bytes_written_per_second": round(written / (ms * 1e-3), 1),
            "share_of_hbm_peak": round(written / (ms * 1e-3) / HBM_PEAK_BYTES_PER_S, 5), "corpus": matches}


def _matches(net, args):
    import torch
    from xiangqi_alphazero_amd import baseline
    rows = []
    for depth in (1, 2, 3):
        res = baseline.play_vs_baseline(net.eval(), args.match_games, depth, args.sims, opening_plies=4, seed=args.match_seed)
        torch.cuda.synchronize()
        rows.append({k: res[k] for k in ("depth", "games", "wins", "losses", "draws", "win_rate", "pairs", "win_rate_se")} |
                    {"win_rate_ci95": list(res["win_rate_ci95"]), "seconds": round(res["seconds"], 2)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def strength(args):
    import types
    import torch
    import make_baseline_games
    from xiangqi_alphazero_amd import model, native_conv, training
    depths = make_baseline_games.parse_depths(args.depths)
    records, corpus = make_baseline_games.play(depths, args.games, args.opening_plies, args.seed)
    torch.manual_seed(args.net_seed)
    net = model.XiangqiNet(128, 6).cuda()
    before = _matches(net, args)
    if native_conv.supported(128):
        net.use_native_conv(True)
    opt = torch.optim.Adam(net.parameters(), lr=args.lr, weight_decay=1e-4, fused=True)
    cfg = types.SimpleNamespace(batch_size=args.batch, num_epochs=1, min_buffer_size=0)
    info = {}
    t0 = time.time()
    epochs = training.pretrain_from_records(net, opt, records, cfg, args.epochs, generator=torch.Generator().manual_seed(args.net_seed),
                                            merge_duplicates=args.merge_duplicates, info=info, movers=args.movers,
                                            skip_opening=True, skip_draws=False)
    torch.cuda.synchronize()
    train_s = time.time() - t0
    after = _matches(net, args)
    return {"tool": "tools/measure_pretrain.py strength", "corpus": {"depths": args.depths, "games_per_match": args.games,
            "games": int(len(records)), "opening_plies": args.opening_plies, "seed": args.seed, "matches": corpus},
            "network": "128x6, random initialisation", "net_seed": args.net_seed, "pretrain": {**info, "epochs": args.epochs,
            "batch_size": args.batch, "learning_rate": args.lr, "movers": args.movers, "merge_duplicates": args.merge_duplicates,
            "policy_loss": [e["policy_loss"] for e in epochs], "value_loss": [e["value_loss"] for e in epochs],
            "distinct_positions": epochs[-1]["distinct_positions"], "seconds": round(train_s, 1)},
            "match": {"games": args.match_games, "simulations": args.sims, "opening_plies": 4, "seed": args.match_seed},
            "before": before, "after": after}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kernel", "strength"])
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--depths", default="3:3")
    ap.add_argument("--games", type=int, default=2048, help="games per match of the corpus")
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--net-seed", type=int, default=0)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--lr", type=float, default=0.001)
    ap.add_argument("--movers", type=int, default=0)
    ap.add_argument("--merge-duplicates", action="store_true")
    ap.add_argument("--match-games", type=int, default=256)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--match-seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    t0 = time.time()
    out = {"kernel": kernel, "strength": strength}[args.part](args)
    out["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
