"""Per-launch A/B of the wide convolution's epilogue builds, with and without residual, in ONE process (not a test):
    tests/microbench/build_ref.sh HEAD~1 parent                      # the parent commit's kernel
    tests/microbench/build_tree.sh rounds2                            # this tree as shipped (two exchange rounds)
    tests/microbench/build_tree.sh rounds4 -DXQ_EPI_ROUNDS=4          # this tree, four rounds over two plane sets
    python tests/microbench/conv_epilogue_ab.py [--b 8192] [--c 256] [--rounds 7] [--iters 20] [--json out.json] \
        parent=tests/microbench/lab/libxq_parent.so rounds2=... rounds4=...
The first library is the baseline; rounds2 against it prices the residual template argument alone, rounds4 against rounds2 the
four-round exchange.  Every library is loaded side by side with ctypes; a round times `iters` back-to-back launches of every
build in turn (HIP events on the current stream), first all builds with the residual, then all without, so clock drift and the
box hit all builds alike; one further round in front of each setting is run and not recorded.  Activations are post-ReLU like
the tower's.  Every build's first output must equal the baseline's bit for bit, in both settings.  Prints and writes, per
setting and build: median, minimum, every round, and for the baseline its own max - min, the yardstick a gain has to exceed."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from xiangqi_alphazero_amd import hip  # noqa: E402  (weight transform + stream pointer only)

ap = argparse.ArgumentParser()
ap.add_argument("--b", type=int, default=8192)
ap.add_argument("--c", type=int, default=256)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--json", default=None)
ap.add_argument("libs", nargs="+")
a = ap.parse_args()
if a.rounds < 5:
    sys.exit("at least 5 rounds")

B, Cn = a.b, a.c
g = torch.Generator(device="cpu").manual_seed(1)
x = torch.relu(torch.randn(B, 90, Cn, generator=g)).cuda()
w = (torch.randn(Cn, Cn, 3, 3, generator=g) * (2.0 / (9 * Cn)) ** 0.5).cuda()
u = hip.wino_transform_weights(w, 128)
bias = (torch.randn(Cn, generator=g) * 0.1).cuda()
res = torch.randn(B, 90, Cn, generator=g).cuda()
flags = 1 | 4                                           # ReLU, wide
stream = hip.stream_ptr(x.device)

libs = []
for spec in a.libs:
    name, path = spec.split("=", 1)
    L = C.CDLL(os.path.abspath(path))
    vp, i32 = C.c_void_p, C.c_int
    L.xq_wino_conv3x3.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.xq_wino_conv3x3.restype = i32
    libs.append((name, L, torch.empty_like(x)))


def run(L, y, with_res):
    rc = L.xq_wino_conv3x3(x.data_ptr(), u.data_ptr(), bias.data_ptr(), res.data_ptr() if with_res else None, y.data_ptr(), B, Cn, flags,
                           stream)
    if rc != 0:
        raise RuntimeError("xq_wino_conv3x3 -> %d" % rc)


result = {"shape": {"B": B, "C": Cn, "activations": "post-ReLU", "relu": True, "wide": True}, "rounds": a.rounds,
          "launches_per_round": a.iters, "baseline": libs[0][0], "unit": "ms per launch", "settings": {}}
for with_res in (True, False):
    key = "residual" if with_res else "no_residual"
    identical = {}
    for name, L, y in libs:
        y.fill_(float("nan"))
        for _ in range(3):
            run(L, y, with_res)
    torch.cuda.synchronize()
    for name, L, y in libs[1:]:
        identical[name] = bool(torch.equal(libs[0][2], y))
        print("%-12s bitwise %s == %s: %s" % (key, libs[0][0], name, identical[name]))
    times = {name: [] for name, _, _ in libs}
    for r in range(-1, a.rounds):                       # round -1 is not recorded: the clock settles under load during it
        for name, L, y in libs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                run(L, y, with_res)
            e1.record()
            torch.cuda.synchronize()
            if r >= 0:
                times[name].append(e0.elapsed_time(e1) / a.iters)
    base = times[libs[0][0]]
    base_med, base_spread = statistics.median(base), max(base) - min(base)
    builds = {}
    for name, _, _ in libs:
        t = times[name]
        med = statistics.median(t)
        builds[name] = {"median": round(med, 5), "min": round(min(t), 5), "max": round(max(t), 5), "all": [round(v, 5) for v in t],
                        "median_vs_baseline": round(med - base_med, 5), "median_vs_baseline_percent": round(100 * (med / base_med - 1), 3)}
        print("%-12s %-10s median %.4f  min %.4f  max %.4f  (%+.4f ms, %+.2f %% against %s)  all: %s"
              % (key, name, med, min(t), max(t), med - base_med, 100 * (med / base_med - 1), libs[0][0], " ".join("%.4f" % v for v in t)))
    result["settings"][key] = {"baseline_spread_max_minus_min": round(base_spread, 5), "bit_identical_to_baseline": identical, "builds": builds}
    print("%-12s %s's own max - min: %.4f ms" % (key, libs[0][0], base_spread))
    if not all(identical.values()):
        print("OUTPUTS DIFFER")
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
sys.exit(0 if all(all(s["bit_identical_to_baseline"].values()) for s in result["settings"].values()) else 1)
