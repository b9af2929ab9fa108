"""Synchronised BatchNorm on the hand-written kernels (native_conv.SyncBnAct, xq_bn_sync_* of csrc/xq_train.hip) and the data-parallel
train step that uses it (`training.train_network(ddp=True, native_bn=True)`, `config.native_sync_bn`).

  1. one rank (RCCL and gloo): bit-identical to the single-device fused BatchNorm (native_conv.BnAct);
  2. two ranks on one GPU (gloo), an uneven split of one batch: the whole batch's statistics -- against BnAct on all rows and against
     float64 entry by entry (tests/numerics.py bounds);
  3. the DDP step: the tower's SyncBatchNorm layers never go through torch, and the step agrees with the torch SyncBatchNorm step;
  4. AlphaZeroLoop with `native_sync_bn = True`, two ranks: finishes with identical replicas.
Multi-process cases run in fresh processes (subprocess or mp.spawn), at most two on the GPU at a time."""
import hashlib
import json
import os
import socket
import subprocess
import sys
import types

import pytest
import torch

import golden_io as G
import numerics as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init_gloo(rank, world, port):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def _spawn(fn, *args):
    import torch.multiprocessing as mp
    mp.spawn(fn, args=(2, _free_port()) + args, nprocs=2, join=True)


# ------------------------------------------------------------------------------------------------------------- 1. one rank

def test_world1_sync_bn_is_bit_identical_to_the_fused_path():
    """SyncBnAct over a one-rank RCCL group and a one-rank gloo group against BnAct on the same operands: y, the running statistics,
    num_batches_tracked, dx, d_residual, dgamma and dbeta equal under torch.equal (C = 64 / 256, with and without residual and ReLU,
    rows not a multiple of 512, non-default momentum and eps)."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sync_bn_world1_worker.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("SYNC_BN_WORLD1 ")]
    assert line, r.stdout[-2000:]
    o = json.loads(line[-1][len("SYNC_BN_WORLD1 "):])
    assert o["backend"] == "nccl" and o["world"] == 1
    assert len(o["cases"]) == 16 and {c["backend"] for c in o["cases"]} == {"nccl", "gloo"}
    assert {c["case"][0] for c in o["cases"]} == {64, 256}
    assert {(c["case"][2], c["case"][3]) for c in o["cases"]} == {(False, False), (False, True), (True, False), (True, True)}
    for c in o["cases"]:
        assert c["differ"] == [], c
        assert c["num_batches_tracked"] == 1, c
        assert len(c["outputs"]) == (8 if c["case"][2] else 7), c


# --------------------------------------------------------------------------------------------------- 2. two ranks, one batch

B2 = 37                    # split 19 + 18
CASES2 = [(64, False, False, 0.1, 1e-5), (256, True, True, 0.3, 1e-3)]


def _batch2(channels, with_res, momentum, eps, seed):
    """The same whole batch and module state on every rank (CPU generator)."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    std = 10.0 ** ((torch.rand(channels, generator=gen) * 2 - 1) * 1.5) * 0.3
    x = rn(B2, channels, 10, 9) * std.view(1, -1, 1, 1) + (0.5 * std * rn(channels)).view(1, -1, 1, 1)
    r = rn(B2, channels, 10, 9) if with_res else None
    gy = rn(B2, channels, 10, 9) * (10.0 ** ((torch.rand(channels, generator=gen) * 2 - 1) * 2)).view(1, -1, 1, 1)
    params = {"weight": torch.where(torch.rand(channels, generator=gen) < 0.2, -1.0, 1.0) * (torch.rand(channels, generator=gen) + 0.5),
              "bias": rn(channels) * 0.2, "running_mean": rn(channels) * 0.1, "running_var": torch.rand(channels, generator=gen) + 0.5}
    return x, r, gy, params


def _bn_run(bn, params, x, r, gy, relu, fn):
    cl = torch.channels_last
    with torch.no_grad():
        for k, v in params.items():
            getattr(bn, k).copy_(v)
    xg = x.cuda().contiguous(memory_format=cl).requires_grad_(True)
    rg = r.cuda().contiguous(memory_format=cl).requires_grad_(True) if r is not None else None
    y = fn(xg, bn, rg, relu)
    y.backward(gy.cuda())
    out = {"y": y.detach(), "dx": xg.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "running_mean": bn.running_mean,
           "running_var": bn.running_var, "nbt": bn.num_batches_tracked}
    if rg is not None:
        out["dres"] = rg.grad
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def _two_rank_bn(rank, world, port, tmp):
    dist = _init_gloo(rank, world, port)
    from xiangqi_alphazero_amd import native_conv
    out = []
    for k, (c, with_res, relu, momentum, eps) in enumerate(CASES2):
        x, r, gy, params = _batch2(c, with_res, momentum, eps, 500 + k)
        lo, hi = [(0, 19), (19, B2)][rank]
        sbn = torch.nn.SyncBatchNorm(c, eps=eps, momentum=momentum).cuda().train()
        assert native_conv.sync_bn_supported(sbn)
        got = _bn_run(sbn, params, x[lo:hi], None if r is None else r[lo:hi], gy[lo:hi], relu, native_conv.sync_bn_act)
        if rank == 0:                                           # the single-device fused BatchNorm on the whole batch
            bn = torch.nn.BatchNorm2d(c, eps=eps, momentum=momentum).cuda().train()
            got["whole"] = _bn_run(bn, params, x, r, gy, relu, native_conv.bn_act)
        out.append(got)
    torch.save(out, os.path.join(tmp, "bn2_%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_compute_the_whole_batch_statistics(tmp_path):
    """Two ranks over gloo on the one GPU hold 19 and 18 samples of one 37-sample batch.  Each rank's y and dx match the rows of BnAct
    on all 37 within 2 KAPPA_BN roundings of their float64 scale (the float64 sums add in another order), and both match float64
    BatchNorm within KAPPA_BN; running statistics are equal on both ranks and within KAPPA_BN_RUNNING (unbiased with n = 37 * 90);
    the ranks' local dgamma / dbeta add up to the whole batch's within KAPPA_BN."""
    from test_train_kernels import _bn_reference_forward, _check_bn_backward, _check_bn_forward, _per_channel
    _spawn(_two_rank_bn, str(tmp_path))
    ranks = [torch.load(tmp_path / ("bn2_%d.pt" % r)) for r in range(2)]
    for k, (c, with_res, relu, momentum, eps) in enumerate(CASES2):
        x, r, gy, params = _batch2(c, with_res, momentum, eps, 500 + k)
        a, b, whole = ranks[0][k], ranks[1][k], ranks[0][k]["whole"]
        case = "2 ranks C=%d res=%d relu=%d" % (c, with_res, relu)
        assert a["running_mean"].shape == (c,)
        for name in ("running_mean", "running_var", "nbt"):
            assert torch.equal(a[name], b[name]), name
        assert int(a["nbt"]) == 1
        y = torch.cat([a["y"], b["y"]])
        dx = torch.cat([a["dx"], b["dx"]])
        dres = torch.cat([a["dres"], b["dres"]]) if with_res else None
        dgamma, dbeta = a["dgamma"] + b["dgamma"], a["dbeta"] + b["dbeta"]
        rm0, rv0 = params["running_mean"].double(), params["running_var"].double()
        ref = _bn_reference_forward(x, r, params["weight"], params["bias"], rm0, rv0, momentum, eps, relu)
        assert ref["n"] == B2 * 90
        # against float64, entry by entry
        _check_bn_forward(case, ref, x, r, params["weight"], params["bias"], rm0, rv0, momentum, y, a["running_mean"], a["running_var"])
        _check_bn_backward(case, ref, params["weight"], relu, y, gy, dx, dres, dgamma, dbeta)
        # against the single-device fused kernels on the whole batch, same per-entry scales (either is within KAPPA_BN of float64)
        ga = params["weight"].double().abs()
        ysc = ga * ref["xhat"].abs().amax(dim=(0, 2, 3)) + params["bias"].double().abs()
        if with_res:
            ysc = ysc + r.double().abs().amax(dim=(0, 2, 3))
        N.check_componentwise(y, whole["y"].double(), _per_channel(ysc, y), 2 * N.KAPPA_BN, "y vs BnAct " + case)
        g = gy.double() * (y > 0).double() if relu else gy.double()
        n = ref["n"]
        sg, sgx = g.abs().sum(dim=(0, 2, 3)), (g * ref["xhat"]).abs().sum(dim=(0, 2, 3))
        dxsc = ga * ref["invstd"] * (g.abs().amax(dim=(0, 2, 3)) + sg / n + ref["xhat"].abs().amax(dim=(0, 2, 3)) * sgx / n)
        N.check_componentwise(dx, whole["dx"].double(), _per_channel(dxsc, dx), 2 * N.KAPPA_BN, "dx vs BnAct " + case)
        N.check_componentwise(dbeta, whole["dbeta"].double(), sg, 2 * N.KAPPA_BN, "dbeta vs BnAct " + case)
        N.check_componentwise(dgamma, whole["dgamma"].double(), sgx, 2 * N.KAPPA_BN, "dgamma vs BnAct " + case)
        # each rank's dgamma / dbeta are the LOCAL sums over its own rows (SyncBatchNorm's backward; DDP then combines them)
        for rk, (lo, hi) in ((a, (0, 19)), (b, (19, B2))):
            gl, xl = g[lo:hi], ref["xhat"][lo:hi]
            N.check_componentwise(rk["dbeta"], gl.sum(dim=(0, 2, 3)), gl.abs().sum(dim=(0, 2, 3)), N.KAPPA_BN, "local dbeta " + case)
            N.check_componentwise(rk["dgamma"], (gl * xl).sum(dim=(0, 2, 3)), (gl * xl).abs().sum(dim=(0, 2, 3)), N.KAPPA_BN,
                                  "local dgamma " + case)


# -------------------------------------------------------------------------------------------------------- 3. the DDP step

def _tower_bns(net):
    bns = [net.input_conv[1]]
    for blk in net.res_blocks:
        bns += [blk.bn1, blk.bn2]
    return bns


def _ddp_step_rank(rank, world, port, tmp):
    dist = _init_gloo(rank, world, port)
    from test_host_logic import _oracle_game_as_compact
    from xiangqi_alphazero_amd import model, training, weights
    t = json.load(open(os.path.join(G.GOLDEN, "train_trace_64x2.json")))
    game = [x for x in G.game_traces() if x["name"] == t["game"]][0]
    arr, _ = _oracle_game_as_compact(game)
    out = {}
    for mode in ("torch", "native"):
        buf = training.ReplayBuffer(50000)
        buf.extend(arr)
        net = model.XiangqiNet(*t["net"])
        net.load_state_dict(weights.make_state_dict(*t["net"], seed=t["seed"]))
        net = net.cuda().use_native_conv(True)
        opt = torch.optim.Adam(net.parameters(), lr=t["lr"], weight_decay=t["weight_decay"])
        sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=t["milestones"], gamma=t["gamma"])
        cfg = types.SimpleNamespace(min_buffer_size=10, num_epochs=1, batch_size=len(buf))          # ONE batch, split across the ranks
        training.prepare_ddp(net, "cuda", native_bn=(mode == "native"))
        calls = [0]
        hooks = [bn.register_forward_hook(lambda *_: calls.__setitem__(0, calls[0] + 1)) for bn in _tower_bns(net)]
        stats = training.train_network(net, opt, sch, buf, cfg, shuffle=False, ddp=True, native_bn=(mode == "native"))
        for h in hooks:
            h.remove()
        sd = net.state_dict()
        out[mode] = {"stats": stats, "hook_calls": calls[0], "n_tower_bn": len(_tower_bns(net)),
                     "all_sync": all(isinstance(bn, torch.nn.SyncBatchNorm) for bn in _tower_bns(net)),
                     "marks": sorted({bool(getattr(m, "native_bn", False)) for m in net.modules() if isinstance(m, torch.nn.SyncBatchNorm)}),
                     "grads": {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters()},
                     "state": {k: v.detach().cpu().clone() for k, v in sd.items()}, "keys": list(sd.keys())}
    torch.save(out, os.path.join(tmp, "step_%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_ddp_step_runs_the_tower_batchnorm_natively(tmp_path):
    """64x2, two ranks over gloo, one batch of the 64x2 trace's buffer split 24 + 24: `train_network(ddp=True, native_bn=True)` against
    `native_bn=False` from the same weights.  Forward hooks on the stem's and the tower's SyncBatchNorm fire once per layer with torch's
    SyncBatchNorm and never in native mode.  Losses agree to 1e-5 relative.  The parameter gradients (after clipping) agree entry by
    entry within 1e-4 of their tensor's largest entry: the two steps differ only in how the BatchNorm statistics are rounded (torch:
    float32 per-rank Welford statistics merged by count; here: float64 sums), about 2^-24 relative per layer, grown by the five
    normalised layers, the heads and the loss (worst measured on an MI355X: 1.4e-6), while a wrong count, or local instead of global
    statistics, moves the gradients by percents.  Both ranks end with identical weights and buffers; the state_dict keeps the reference's keys, and
    num_batches_tracked counts the batch in every layer in both modes (weights.make_state_dict starts it at 1)."""
    from xiangqi_alphazero_amd import weights
    _spawn(_ddp_step_rank, str(tmp_path))
    ranks = [torch.load(tmp_path / ("step_%d.pt" % r)) for r in range(2)]
    want_keys = list(weights.state_dict_shapes(64, 2).keys())
    for o in ranks:
        t, n = o["torch"], o["native"]
        assert t["all_sync"] and n["all_sync"] and t["n_tower_bn"] == n["n_tower_bn"] == 5
        assert t["hook_calls"] == 5, t["hook_calls"]                 # torch mode: every tower layer through SyncBatchNorm.forward
        assert n["hook_calls"] == 0, n["hook_calls"]                 # native mode: none of them
        assert t["marks"] == [False] and n["marks"] == [True]
        for k in ("policy_loss", "value_loss", "total_loss"):
            assert abs(n["stats"][k] - t["stats"][k]) <= 1e-5 * abs(t["stats"][k]), (k, n["stats"][k], t["stats"][k])
        worst = 0.0
        for name, gt in t["grads"].items():
            gn = n["grads"][name]
            tol = 1e-4 * gt.abs().max().item()
            err = (gn - gt).abs().max().item()
            assert err <= tol, (name, err, tol)
            worst = max(worst, err / max(tol, 1e-30))
        print("DDP-STEP grad error / tolerance, worst: %.3g" % worst)
        assert n["keys"] == t["keys"] == want_keys
        for k in want_keys:
            if k.endswith("num_batches_tracked"):
                assert int(n["state"][k]) == int(t["state"][k]) == 2, k
    for k in want_keys:                                              # both replicas identical, in both modes
        for mode in ("torch", "native"):
            assert torch.equal(ranks[0][mode]["state"][k], ranks[1][mode]["state"][k]), (mode, k)


# -------------------------------------------------------------------------------------------------------------- 4. the loop

def _loop_rank(rank, world, port, tmp):
    dist = _init_gloo(rank, world, port)
    from xiangqi_alphazero_amd import train_loop
    cfg = types.SimpleNamespace(
        num_channels=64, num_res_blocks=1, num_simulations=8, c_puct=1.5, temperature_threshold=10, num_games_per_iter=12,
        max_game_length=30, resign_threshold=-0.9, resign_check_steps=5, enable_resign=True, random_opening_moves=4,
        num_iterations=2, batch_size=64, num_epochs=1, learning_rate=0.002, weight_decay=1e-4, lr_milestones=[50, 80],
        lr_gamma=0.1, max_buffer_size=50000, min_buffer_size=100, eval_games=5, eval_win_rate=0.55, eval_simulations=8,
        checkpoint_dir=os.path.join(tmp, "ck%d" % rank), save_interval=2, native_sync_bn=True)
    loop = train_loop.AlphaZeroLoop(cfg, "cuda", seed=3)
    stats = loop.train()
    m = loop.current_model
    sync = [x for x in m.modules() if isinstance(x, torch.nn.SyncBatchNorm)]
    flat = torch.cat([t.reshape(-1).double() for t in list(m.state_dict().values()) + list(loop.best_model.state_dict().values())])
    digest = hashlib.sha256(flat.cpu().numpy().tobytes() + loop.buffer.store.cpu().numpy().tobytes()).hexdigest()
    ok = (len(sync) == 5 and all(getattr(x, "native_bn", False) for x in sync) and bool(stats[0]["training"])
          and bool(stats[1]["training"]) and stats[1]["training"]["policy_loss"] > 0 and len(stats) == 2)
    open(os.path.join(tmp, "loop%d" % rank), "w").write("%d %s" % (int(ok), digest))
    dist.barrier()
    dist.destroy_process_group()


def test_loop_with_native_sync_bn_two_ranks_share_one_gpu(tmp_path):
    """AlphaZeroLoop with config.native_sync_bn = True, two iterations, two ranks over gloo on the one GPU: the data-parallel step runs
    the synchronised BatchNorm of the stem and the tower on the hand-written kernels; both ranks end with bit-identical weights and
    buffers (current and best model, replay buffer)."""
    _spawn(_loop_rank, str(tmp_path))
    out = [open(tmp_path / ("loop%d" % r)).read().split() for r in range(2)]
    assert out[0][0] == "1" and out[1][0] == "1", out
    assert out[0][1] == out[1][1]
