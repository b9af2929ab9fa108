#!/usr/bin/env python3
"""How many records of a real replay buffer are duplicates of one position, and what merging them costs, measured on the GPU.
Everything runs in one fresh child process under `timeout -k` (the games are played once and every figure is taken over the same
samples); the child rewrites the output file after every stage, so a measurement cut short keeps what it has.

    python tools/measure_merge_duplicates.py --preset cfg1 --parent-lib <libxq_hip.so built from the parent commit> \\
        --out profiles/r20_merge_duplicates_cfg1.json

Stages, on the samples of complete games through run_games on peaked weights (make_state_dict(policy_gain=8)) at a preset -- cfg1 =
BASELINE configs[1] (1024 slots x 400 sims x 128x6), small = a quick look:
`duplicates`: records, distinct positions with and without the mirror, the largest group, the group-size histogram, and per ply
    bucket the share of merged records (records that are not the oldest member of their group).
`grouping`: the time of keys + stable sort + heads over the buffer (device events around --reps repeats after a warm-up), the
    three parts alone, and ReplayBuffer.position_groups as a whole (a host clock around work that ends in a synchronise).
`batch`: microseconds per row of xq_groups_to_batch at the batch size (256, the train step's), device events around --launches
    back-to-back launches whose rows are a fresh random draw per launch from a pool of 64 index sets:
      * over a buffer of singleton groups (every record its own group), against xq_samples_to_batch_ex of the PARENT commit's
        library (--parent-lib, loaded beside this tree's in the same process) on the same records and the same draws, alternated
        --runs times each; the ratio of the means is reported with both spreads (`batch_4096`: the same two arms at 4096 rows
        per launch, where the host's enqueue rate does not bound the window);
      * over the real groups (logical samples drawn uniformly from 2 * n_groups, so large groups are drawn as rarely as in an
        epoch), and over the largest group alone.
`train`: the wall time of one train_network call (128x6, batch 256, one epoch over the whole buffer) with the option on and off,
    alternated --runs times each after a warm-up call of each kind.
Whether a network trained on merged samples is stronger is not measured here: that takes arena matches over trained networks
(tools/measure_arena.py).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import types

import measure_common as mc

PEAKED_GAIN = mc.GAINS["peaked"]
BATCH = 256
PRESETS = {"cfg1": mc.PRESETS["cfg1"], "small": dict(mc.PRESETS["small"], slots=64, games=64, sims=32, max_game_length=60)}
PLY_BUCKETS = [(i, i + 1) for i in range(10)] + [(10, 20), (20, 40), (40, 80), (80, 1 << 16)]


def _play(p, seed=11):
    from xiangqi_alphazero_amd import selfplay
    samples, results, st, elapsed = selfplay.run_games(mc.make_net(p["channels"], p["blocks"]), mc.selfplay_config(p), p["games"],
                                                       "cuda", n_slots=p["slots"], seed=seed, poll_every=mc.poll_every(p),
                                                       device_records=True)
    return samples, results, elapsed


def _group(runs):
    return mc.group(runs, digits=4, round_values=True)


def _events(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def stage_duplicates(buf, rec):
    import numpy as np
    out = {}
    for name, mirror in (("with_mirror", True), ("without_mirror", False)):
        g = buf.position_groups(mirror)
        sizes = g.sizes.cpu().numpy()
        hist = {str(k): int((sizes == k).sum()) for k in (1, 2, 3, 4)}
        hist["5-16"], hist["17-128"], hist[">128"] = int(((sizes >= 5) & (sizes <= 16)).sum()), \
            int(((sizes >= 17) & (sizes <= 128)).sum()), int((sizes > 128).sum())
        out[name] = {"distinct_positions": g.n_groups, "merged_records": g.n_records - g.n_groups,
                     "share_merged": round((g.n_records - g.n_groups) / g.n_records, 6), "largest_group": int(sizes.max()),
                     "groups_by_size": hist, "records_in_groups_of_two_or_more": int(sizes[sizes > 1].sum())}
        if mirror:
            # records oldest first are the buffer's own order here (the ring has not wrapped): the first member of a group stays
            first = np.zeros(g.n_records, dtype=bool)
            first[g.members.cpu().numpy()[g.offsets.cpu().numpy()[:-1]]] = True
            ply = rec["ply"].astype(np.int64)
            by_ply = {}
            for lo, hi in PLY_BUCKETS:
                at = (ply >= lo) & (ply < hi)
                if at.any():
                    key = str(lo) if hi == lo + 1 else ("%d-%d" % (lo, hi - 1) if hi < 1 << 16 else "%d+" % lo)
                    by_ply[key] = {"records": int(at.sum()), "share_merged": round(float((~first[at]).mean()), 6)}
            out["share_merged_by_ply"] = by_ply
    return out


def stage_grouping(buf, reps):
    import torch
    from xiangqi_alphazero_amd import hip
    n = buf.count
    ring = torch.arange(n, dtype=torch.int32, device="cuda")
    keys, mir = hip.position_keys(buf.store, ring, True)
    order = torch.sort(keys, stable=True)[1].to(torch.int32)
    parts = {"xq_position_keys": lambda: hip.position_keys(buf.store, ring, True),
             "torch.sort (stable, int64 keys) + int32 cast": lambda: torch.sort(keys, stable=True)[1].to(torch.int32),
             "xq_position_group_heads": lambda: hip.position_group_heads(buf.store, ring, order, keys, mir)}

    def three():
        k, m = hip.position_keys(buf.store, ring, True)
        o = torch.sort(k, stable=True)[1].to(torch.int32)
        hip.position_group_heads(buf.store, ring, o, k, m)

    out = {"records": n, "reps": reps, "keys_sort_heads_ms": round(_events(three, reps) * 1e3, 4),
           "parts_ms": {k: round(_events(f, reps) * 1e3, 4) for k, f in parts.items()}}
    buf.position_groups(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        buf.position_groups(True)
    torch.cuda.synchronize()
    out["ReplayBuffer.position_groups_ms (host clock, with its relabelling and one .item())"] = \
        round((time.perf_counter() - t0) / reps * 1e3, 4)
    return out


def stage_batch(buf, parent_lib, launches, runs, BATCH=BATCH, singletons_only=False):
    import torch
    from xiangqi_alphazero_amd import hip
    n = buf.count
    dev = buf.store.device
    gen = torch.Generator().manual_seed(7)
    states = torch.empty((BATCH, 15, 10, 9), dtype=torch.float32, device=dev)
    pi = torch.empty((BATCH, hip.ACTION_SPACE), dtype=torch.float32, device=dev)
    z = torch.empty((BATCH, 1), dtype=torch.float32, device=dev)
    stream = hip.stream_ptr(dev)
    opts = hip.BatchOpts(0.0)
    T = float(buf.late_temperature)

    def draws(high):
        logical = [torch.randint(0, high, (BATCH,), generator=gen).to(dev) for _ in range(64)]
        return [((l // 2).to(torch.int32).contiguous(), (l % 2).to(torch.uint8).contiguous()) for l in logical]

    def grouped(groups, sets):
        turn = [0]

        def fn():
            g, f = sets[turn[0] % len(sets)]
            turn[0] += 1
            hip.check(hip.lib().xq_groups_to_batch(buf.store.data_ptr(), groups.offsets.data_ptr(), groups.members.data_ptr(),
                                                   groups.member_mirrored.data_ptr(), groups.n_groups, g.data_ptr(), f.data_ptr(),
                                                   BATCH, T, C.byref(opts), states.data_ptr(), pi.data_ptr(), z.data_ptr(), stream),
                      "xq_groups_to_batch")
        return fn

    out = {"batch": BATCH, "launches_per_run": launches, "bytes_written_per_row": 4 * (1350 + 8100 + 1),
           "timing": "device events around back-to-back launches after a warm-up launch; rows drawn afresh per launch"}
    # singleton groups: every record its own group, un-mirrored -- the plain kernel's work plus three index words per row
    from xiangqi_alphazero_amd.training import PositionGroups
    single = PositionGroups(torch.arange(n + 1, dtype=torch.int32, device=dev), torch.arange(n, dtype=torch.int32, device=dev),
                            torch.zeros(n, dtype=torch.uint8, device=dev), n, torch.ones(n, dtype=torch.int64, device=dev), n)
    sets = draws(2 * n)
    this_fn = grouped(single, sets)
    arms = {"this_groups_to_batch_singletons": this_fn}
    if parent_lib:
        parent = C.CDLL(parent_lib)
        vp = C.c_void_p
        parent.xq_samples_to_batch_ex.argtypes = [vp, vp, vp, C.c_int32, C.c_double, C.POINTER(hip.BatchOpts), vp, vp, vp, vp]
        turn = [0]

        def parent_fn():
            g, f = sets[turn[0] % len(sets)]                     # a singleton group's id IS its record index
            turn[0] += 1
            hip.check(parent.xq_samples_to_batch_ex(buf.store.data_ptr(), g.data_ptr(), f.data_ptr(), BATCH, T, C.byref(opts),
                                                    states.data_ptr(), pi.data_ptr(), z.data_ptr(), stream), "parent xq_samples_to_batch_ex")
        arms["parent_samples_to_batch_ex"] = parent_fn
        # the two produce the same bytes on the same draw
        parent_fn()
        a = (states.clone(), pi.clone(), z.clone())
        turn[0] = 0
        single_turn = grouped(single, sets)
        single_turn()
        torch.cuda.synchronize()
        out["singleton_rows_equal_parent_bytes"] = all(torch.equal(x, y) for x, y in zip(a, (states, pi, z)))
    times = {k: [] for k in arms}
    for _ in range(runs):                                        # alternated
        for k, fn in arms.items():
            times[k].append(_events(fn, launches) / BATCH * 1e6)
    out["us_per_row"] = {k: _group(v) for k, v in times.items()}
    if parent_lib:
        t, p = out["us_per_row"]["this_groups_to_batch_singletons"], out["us_per_row"]["parent_samples_to_batch_ex"]
        out["singletons_over_parent_mean"] = round(t["mean"] / p["mean"], 4)
        out["this_mean_within_parent_spread"] = mc.within_spread(p, t)
    if singletons_only:
        return out
    real = buf.position_groups(True)
    real_fn = grouped(real, draws(2 * real.n_groups))
    out["us_per_row"]["this_groups_to_batch_real_groups"] = _group([_events(real_fn, launches) / BATCH * 1e6 for _ in range(runs)])
    big = int(torch.argmax(real.sizes).item())
    big_sets = [(torch.full((BATCH,), big, dtype=torch.int32, device=dev), (torch.arange(BATCH, device=dev) % 2).to(torch.uint8))]
    big_fn = grouped(real, big_sets)
    out["largest_group_size"] = int(real.sizes.max().item())
    out["us_per_row"]["this_groups_to_batch_largest_group_only"] = _group([_events(big_fn, max(1, launches // 50)) / BATCH * 1e6
                                                                            for _ in range(runs)])
    return out


def stage_train(buf, runs):
    import torch
    from xiangqi_alphazero_amd import training
    net = mc.make_net(128, 6, mc.GAINS["random"]).cuda()
    net.use_native_conv(True)
    opt = torch.optim.Adam(net.parameters(), lr=2e-3, weight_decay=1e-4, fused=True)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[5000], gamma=0.1)
    tcfg = types.SimpleNamespace(min_buffer_size=1, num_epochs=1, batch_size=BATCH)
    g = torch.Generator().manual_seed(3)
    walls = {"off": [], "on": []}
    stats = {}
    for r in range(runs + 1):                                    # the first call of each kind is the warm-up
        for kind in ("off", "on"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats[kind] = training.train_network(net, opt, sch, buf, tcfg, generator=g, merge_duplicates=kind == "on")
            torch.cuda.synchronize()
            if r:
                walls[kind].append(time.perf_counter() - t0)
    out = {"model": "128x6, native conv", "batch": BATCH, "epochs_per_call": 1,
           "train_network_wall_s": {k: _group(v) for k, v in walls.items()},
           "epoch_samples": {k: stats[k]["epoch_samples"] for k in stats},
           "stats_on": {k: stats["on"][k] for k in ("distinct_positions", "merged_records", "largest_group")}}
    out["on_over_off_mean"] = round(out["train_network_wall_s"]["on"]["mean"] / out["train_network_wall_s"]["off"]["mean"], 4)
    return out


def child(job):
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing here is measured without one")
    from xiangqi_alphazero_amd import training
    from xiangqi_alphazero_amd import sample_format as F
    p = PRESETS[job["preset"]]
    out = {"tool": "tools/measure_merge_duplicates.py", "preset": job["preset"], "weights": "peaked (policy_gain %g)" % PEAKED_GAIN}

    samples, results, elapsed = _play(p)
    torch.cuda.synchronize()
    out.update(games=int(results.shape[0]), records=int(samples.shape[0]), selfplay_wall_s=round(elapsed, 2),
               random_opening_moves=p["random_opening_moves"])
    buf = training.ReplayBuffer(2 * int(samples.shape[0]) + 2, "cuda")
    buf.extend(samples)
    rec = samples.cpu().numpy().reshape(-1).view(F.SAMPLE_DTYPE)
    for name, fn in (("duplicates", lambda: stage_duplicates(buf, rec)), ("grouping", lambda: stage_grouping(buf, job["reps"])),
                     ("batch", lambda: stage_batch(buf, job.get("parent_lib"), job["launches"], job["runs"])),
                     # the same two arms at 4096 rows per launch, where a launch is long enough that the host's enqueue rate
                     # does not bound the window
                     ("batch_4096", lambda: stage_batch(buf, job.get("parent_lib"), max(1, job["launches"] // 4), job["runs"], 4096, True)),
                     ("train", lambda: stage_train(buf, job["runs"]))):
        if name in job["stages"]:
            out[name] = fn()
            print(name, json.dumps(out[name]), flush=True)
            mc.save_json(out, job.get("out"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=sorted(PRESETS), default="cfg1")
    ap.add_argument("--parent-lib", default=None, help="libxq_hip.so built from the parent commit (the singleton comparison)")
    ap.add_argument("--stages", nargs="*", default=["duplicates", "grouping", "batch", "batch_4096", "train"])
    ap.add_argument("--reps", type=int, default=20, help="grouping: repeats in the timed window")
    ap.add_argument("--launches", type=int, default=2000, help="batch: launches per run")
    ap.add_argument("--runs", type=int, default=3, help="batch and train: alternated runs per arm")
    args = mc.parse_args(ap, 540, child)
    job = dict(preset=args.preset, parent_lib=os.path.abspath(args.parent_lib) if args.parent_lib else None, stages=args.stages,
               reps=args.reps, launches=args.launches, runs=args.runs, out=os.path.abspath(args.out) if args.out else None)
    sys.exit(0 if mc.run_children(__file__, [job], args.timeout, {}) else 1)       # the child writes --out itself, stage by stage


if __name__ == "__main__":
    main()
