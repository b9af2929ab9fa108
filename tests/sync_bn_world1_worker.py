"""Worker of tests/test_sync_bn_gpu.py (a fresh process: the one-rank RCCL group is initialised before any other GPU work).

Runs native_conv.SyncBnAct beside native_conv.BnAct on the same operands, over the one-rank `nccl` group (RCCL) and over a one-rank
`gloo` group on device tensors.  With one rank the all-reduce leaves the float64 sums as they are, so every output must be
bit-identical.  Prints one JSON line: per case and backend, the names of the outputs that differ (none expected)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# (channels, batch, residual, relu, momentum, eps); rows = batch * 90, none of them a multiple of NSEG = 512
CASES = [(64, 7, False, True, 0.1, 1e-5), (64, 37, True, True, 0.3, 1e-3), (64, 3, True, False, 0.1, 1e-5),
         (64, 19, False, False, 0.25, 1e-4), (256, 7, True, True, 0.3, 1e-3), (256, 37, False, False, 0.1, 1e-5),
         (256, 11, False, True, 0.1, 1e-5), (256, 5, True, False, 0.05, 2e-3)]


def _run(channels, batch, with_res, relu, momentum, eps, group, seed, sync):
    import torch
    from xiangqi_alphazero_amd import native_conv
    gen = torch.Generator().manual_seed(seed)
    cl = torch.channels_last
    rn = lambda *s: torch.randn(*s, generator=gen)
    x = (rn(batch, channels, 10, 9) * (rn(channels).abs() + 0.1).view(1, -1, 1, 1) + rn(channels).view(1, -1, 1, 1))
    x = x.cuda().contiguous(memory_format=cl).requires_grad_(True)
    r = rn(batch, channels, 10, 9).cuda().contiguous(memory_format=cl).requires_grad_(True) if with_res else None
    gy = rn(batch, channels, 10, 9).cuda()
    if sync:
        bn = torch.nn.SyncBatchNorm(channels, eps=eps, momentum=momentum, process_group=group).cuda().train()
        assert native_conv.sync_bn_supported(bn)
    else:
        bn = torch.nn.BatchNorm2d(channels, eps=eps, momentum=momentum).cuda().train()
        assert native_conv.bn_supported(bn)
    with torch.no_grad():
        bn.weight.copy_(rn(channels) + 0.2)
        bn.bias.copy_(rn(channels) * 0.3)
        bn.running_mean.copy_(rn(channels) * 0.1)
        bn.running_var.copy_(rn(channels).abs() + 0.5)
    y = (native_conv.sync_bn_act if sync else native_conv.bn_act)(x, bn, r, relu)
    y.backward(gy)
    torch.cuda.synchronize()
    out = {"y": y.detach(), "dx": x.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "running_mean": bn.running_mean,
           "running_var": bn.running_var, "num_batches_tracked": bn.num_batches_tracked}
    if with_res:
        out["dresidual"] = r.grad
    return out


def main():
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    gloo = dist.new_group(backend="gloo")
    res = {"backend": dist.get_backend(), "world": dist.get_world_size(), "cases": []}
    for k, case in enumerate(CASES):
        want = _run(*case, group=None, seed=100 + k, sync=False)
        for name, group in (("nccl", None), ("gloo", gloo)):
            got = _run(*case, group=group, seed=100 + k, sync=True)
            diff = sorted(n for n in want if not torch.equal(want[n], got[n]))
            res["cases"].append({"case": list(case), "backend": name, "outputs": sorted(want), "differ": diff,
                                 "num_batches_tracked": int(got["num_batches_tracked"])})
    dist.barrier()
    dist.destroy_process_group()
    print("SYNC_BN_WORLD1 " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
