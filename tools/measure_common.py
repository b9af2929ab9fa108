"""What the tools/measure_<option>.py tools share: the presets, the networks and the self-play config they measure with, the one
runner of child processes, the replayed-steps loop behind every `trace` part, and the reading of a profiler's kernel statistics.

A tool imports this as `import measure_common` (it sits beside the script; there is no package).  Importing it loads neither
torch nor the project's package: a child that measures another checkout puts that checkout on sys.path first, and only then do
make_net, staggered_engine and replay_steps import what they need.

The runner is the rule of the shared GPU machines in one place: every child runs under `timeout -k` with a limit of its own, and
after a child that failed, aborted or ran into its limit no further child is started.
"""
import csv
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAINS = {"random": 1.0, "peaked": 8.0}           # weights.make_state_dict(policy_gain=...)
# cfg1 = BASELINE configs[1] with the "full" game settings; standard_train = the reference's preset; small = a quick look
PRESETS = {
    "cfg1": dict(slots=1024, games=1024, sims=400, channels=128, blocks=6, temperature_threshold=20, max_game_length=400,
                 random_opening_moves=8),
    "standard_train": dict(slots=20, games=20, sims=200, channels=128, blocks=6, temperature_threshold=20, max_game_length=300,
                           random_opening_moves=6),
    "small": dict(slots=256, games=256, sims=64, channels=64, blocks=2, temperature_threshold=20, max_game_length=120,
                  random_opening_moves=6),
}


def make_net(channels, blocks, gain=GAINS["peaked"], seed=0):
    from xiangqi_alphazero_amd import model, weights
    net = model.XiangqiNet(channels, blocks)
    net.load_state_dict(weights.make_state_dict(channels, blocks, seed=seed, policy_gain=gain))
    return net


def selfplay_config(preset, **extra_keys):
    """The config selfplay.run_games reads: the reference's eight keys from a preset, plus the keys a tool adds or overrides."""
    keys = dict(num_simulations=preset["sims"], c_puct=1.5, temperature_threshold=preset["temperature_threshold"],
                max_game_length=preset["max_game_length"], random_opening_moves=preset["random_opening_moves"],
                enable_resign=True, resign_threshold=-0.9, resign_check_steps=5)
    keys.update(extra_keys)
    return types.SimpleNamespace(**keys)


def poll_every(preset):
    return 64 if preset["slots"] < 64 else 256


def save_json(out, path):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


def emit_result(row):
    """The child's side of the runner's protocol: one line the parent finds in the child's output."""
    print("RESULT " + json.dumps(row), flush=True)


def parse_args(ap, timeout, child=None):
    """The three arguments of every tool on the runner (`--out`, `--timeout` per child, `--child`), then the parse.  With `child`,
    a child process (`--child <job>`) puts the job's `tree_path` (default: this tree) first on sys.path, emits `child(job)` and ends."""
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=timeout, help="seconds per child")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if child and args.child:
        job = json.loads(args.child)
        sys.path.insert(0, job.get("tree_path", ROOT))
        emit_result(child(job))
        sys.exit(0)
    return args


def record_hash(samples, results):
    """16 hex digits over the sorted results and samples of a run: equal for equal games, whatever order they finished in."""
    import hashlib
    import numpy as np
    return hashlib.sha256(np.sort(results, order=["slot", "game_seq"]).tobytes() +
                          np.sort(samples, order=["slot", "game_seq", "ply"]).tobytes()).hexdigest()[:16]


def run_children(script, jobs, timeout, out, out_path=None, argv=lambda job: [], cwd=lambda job: ROOT, after_each=None):
    """Run `script <argv(job)> --child <json of job>` once per job, each in a fresh process under `timeout -k 10 <timeout>` in
    `cwd(job)`.  A child fails by a non-zero exit status or by printing no result line: the tail of its output is shown,
    out["failed"] says which job and how, and no further child is started.  A passing child's row (or rows, when it emits a list)
    goes to out["runs"], the last with `child_wall_s`; then `after_each(out, job, row)` runs.  With `out_path`, `out` is written
    there before the first child and after every child, so a measurement cut short keeps what it has.  True when all passed."""
    out.setdefault("runs", [])
    save_json(out, out_path)
    for job in jobs:
        t0 = time.time()
        cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(script), *argv(job), "--child",
               json.dumps(job)]
        r = subprocess.run(cmd, cwd=cwd(job), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = next((l for l in r.stdout.splitlines() if l.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(r.stdout[-3000:], file=sys.stderr)
            print(f"child failed (exit {r.returncode}) on {job}: stopping", file=sys.stderr)
            out["failed"] = dict(job=job, exit=r.returncode)
            save_json(out, out_path)
            return False
        row = json.loads(line[len("RESULT "):])
        rows = row if isinstance(row, list) else [row]
        rows[-1]["child_wall_s"] = round(time.time() - t0, 1)
        for x in rows:
            print(json.dumps(x), flush=True)
        out["runs"].extend(rows)
        if after_each:
            after_each(out, job, row)
        save_json(out, out_path)
    return True


def staggered_engine(preset, net=None, out_rows_per_slot=16, **engine_kw):
    """An engine at a preset's slots x sims from a staggered start (seed 5), on the evaluator of `net` (default: the preset's
    network on peaked weights).  `engine_kw` are the options under measurement."""
    from xiangqi_alphazero_amd import engine, evaluator
    ev = evaluator.make_evaluator(make_net(preset["channels"], preset["blocks"]) if net is None else net, "cuda", "hip")[0]
    cfg = engine.make_config(preset["slots"], preset["sims"], seed=5, start_stagger=True,
                             max_out_samples=preset["slots"] * out_rows_per_slot)
    return engine.SelfPlayEngine(cfg, evaluator=ev, **engine_kw)


def replay_steps(eng, steps, drain_every=256, drain=None):
    """`steps` steps with a drain of the samples (and `drain()`, if given) every `drain_every`; synchronised; the wall seconds."""
    import torch
    t0 = time.time()
    for i in range(steps):
        eng.step()
        if i % drain_every == drain_every - 1:
            eng.drain_device()
            if drain:
                drain()
    torch.cuda.synchronize()
    return round(time.time() - t0, 1)


def trace(preset, steps, engine_kw, keys, drain=None):
    """The `trace` part of a tool: replayed (captured) steps of staggered_engine(preset, **engine_kw) for a kernel trace taken
    around this process, then one JSON line: the common counters plus `keys(eng, stats)`.  `drain(eng)` is an extra drain."""
    eng = staggered_engine(preset, **engine_kw)
    assert eng.capture_step()
    wall = replay_steps(eng, steps, drain=(lambda: drain(eng)) if drain else None)
    st = eng.stats()
    print(json.dumps({**keys(eng, st), "steps": eng.steps, "launch": eng.launch_mode, "wall_s": wall, "moves": st["moves_played"],
                      "sims": st["sims"], "overflow": st["overflow"]}), flush=True)


def off_on_child(job, p, opt):
    """One run of an off/on measurement of an engine option on the tree the child was started for (with the option off it uses
    only what the parent commit's tree has too).  `opt`: the job's key that says "on" or "off", `config_key` (as a training loop
    sets it), `engine_kw` (the engine's keyword and its key in the stats) and `extra(stats, steps)`, the option's own figures.
    Complete games through run_games at preset `p` (packed step, replayed graph, weights job["weights"], default peaked):
    games/hour and a hash of the sorted records; then `step_steps` graph replays from a staggered start in chunks of 100 between
    two device events: microseconds per step, and `extra` again as step_*."""
    import torch
    from xiangqi_alphazero_amd import selfplay
    on = job[opt["job_key"]] == "on"
    net = make_net(p["channels"], p["blocks"], GAINS[job.get("weights", "peaked")])
    cfg = selfplay_config(p, **({opt["config_key"]: True} if on else {}))
    samples, results, st, elapsed = selfplay.run_games(net, cfg, p["games"], "cuda", n_slots=p["slots"], seed=11,
                                                       poll_every=poll_every(p))
    torch.cuda.synchronize()
    assert bool(st.get(opt["engine_kw"], False)) == on and int(st["overflow"]) == 0
    row = {"preset": job["preset"], "weights": job.get("weights", "peaked"), "tree": job["tree"], opt["engine_kw"]: on,
           "path": st["path"], "launch": st["launch"], "games": int(len(results)), "samples": int(len(samples)),
           "wall_s": round(elapsed, 2), "games_per_hour": round(len(results) * 3600.0 / elapsed, 1),
           "mean_plies": round(float(results["steps"].mean()), 2), "moves": int(st["moves_played"]), "sims": int(st["sims"]),
           "steps": int(st["steps"]), "rows_evaluated": int(st["rows_evaluated"]), "record_hash": record_hash(samples, results),
           **opt["extra"](st, int(st["steps"]))}
    eng = staggered_engine(p, net, **({opt["engine_kw"]: True} if on else {}))
    assert eng.capture_step() and eng.launch_mode == "graph"
    chunk = 100
    for _ in range(64):
        eng.step()
    before, chunks = eng.stats(), []
    for _ in range(int(job["step_steps"]) // chunk):
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
    timed = {k: v - before[k] for k, v in est.items() if isinstance(v, int) and not isinstance(v, bool) and k in before}
    row.update(step_us_mean=round(sum(us) / len(us), 3), step_us_median=round(us[len(us) // 2], 3), step_us_min=round(us[0], 3),
               step_steps=len(us) * chunk, step_rows_evaluated=int(est["rows_evaluated"]),
               **{"step_" + k: v for k, v in opt["extra"](timed, len(us) * chunk).items()})
    return row


def off_on_steps_child(job, p, opt):
    """`steps` eager steps (packed, or the option's own) of a staggered engine at preset `p` with the option on or off and nothing else: the child to
    take a kernel trace around, in a run of its own."""
    on = job[opt["job_key"]] == "on"
    eng = staggered_engine(p, out_rows_per_slot=64, **({opt["engine_kw"]: True} if on else {}))
    replay_steps(eng, int(job["steps"]))                         # eager: no step is captured here
    st = eng.stats()
    assert int(st["overflow"]) == 0
    return {opt["engine_kw"]: on, "steps": int(job["steps"]), "rows_evaluated": int(st["rows_evaluated"]), "slots": p["slots"],
            "preset": job["preset"], **opt["extra"](st, int(job["steps"]))}


def off_on_jobs(parent_tree, repeats, job_key, **job):
    """The jobs of `repeats` alternated pairs: `off` on `parent_tree`, a built checkout of the parent commit, `on` on this tree."""
    if not parent_tree or not os.path.isdir(os.path.join(parent_tree, "xiangqi-alphazero_amd")):
        sys.exit("--parent-tree: a built checkout of the parent commit is required (the `off` runs are taken on it)")
    trees = {"parent": os.path.abspath(parent_tree), "this": ROOT}
    return [dict(job, tree=tree, tree_path=trees[tree], **{job_key: m})
            for _ in range(repeats) for tree, m in (("parent", "off"), ("this", "on"))]


def kernel_mean_us(csv_path, want, without=()):
    """Mean time per launch of the kernels whose name holds `want` (and none of `without`) in a rocprofv3 `*_kernel_stats.csv`
    (calls-weighted), in microseconds; None when there is no such launch."""
    calls = total = 0
    with open(csv_path, newline="") as f:
        for row in csv.DictReader(f):
            if want in row["Name"] and not any(w in row["Name"] for w in without):
                calls += int(row["Calls"])
                total += float(row["TotalDurationNs"])
    return round(total / calls / 1000.0, 3) if calls else None


def group(values, digits=3, round_values=False):
    """The runs of one kind with their own run-to-run spread; None entries are dropped, and no entry at all gives None."""
    raw = [x for x in values if x is not None]
    if not raw:
        return None
    v = [round(x, digits) for x in raw] if round_values else raw
    return {"runs": v, "min": min(v), "max": max(v), "spread": round(max(raw) - min(raw), digits),
            "mean": round(sum(raw) / len(raw), digits)}


def within_spread(parent, other):
    """Does the mean of `other` lie between the smallest and the largest of the parent's own runs?"""
    return parent["min"] <= other["mean"] <= parent["max"]


def parent_this_summary(out, keys):
    """For runs alternated between the parent's tree (the option off) and this tree (on), told apart by their `tree`: `order`,
    and once both have a run, per key both groups, the distance of their means and whether the spread of the parent's own runs
    covers it."""
    out["order"] = [r["tree"] for r in out["runs"]]
    par, this = ([r for r in out["runs"] if r["tree"] == tree] for tree in ("parent", "this"))
    if par and this:
        out["summary"] = {}
        for key in keys:
            p, t = group([r[key] for r in par]), group([r[key] for r in this])
            out["summary"][key] = {"parent_off": p, "this_on": t, "delta_of_means": round(t["mean"] - p["mean"], 3),
                                   "margin_parent_spread": p["spread"],
                                   "within_margin": abs(t["mean"] - p["mean"]) <= p["spread"]}


def spread_groups(specs, kernels, kinds=("on",)):
    """`specs`: `name=<kernel_stats.csv>,<kernel_stats.csv>,...` per group of runs; `kernels`: {table: (want, without)}.  One
    table of groups per kernel, and from the first table `<kind>_within_parent_spread` where `kind` and `parent` both have runs."""
    out = {table: {} for table in kernels}
    for spec in specs:
        name, files = spec.split("=", 1)
        for table, (want, without) in kernels.items():
            out[table][name] = group([kernel_mean_us(p, want, without) for p in files.split(",")])
    g = next(iter(out.values()))
    for kind in kinds:
        if g.get(kind) and g.get("parent"):
            out[f"{kind}_within_parent_spread"] = within_spread(g["parent"], g[kind])
    return out
