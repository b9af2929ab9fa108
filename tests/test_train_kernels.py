"""The train-step kernels of csrc/xq_train.hip and the training direction of k_wino_conv, entry by entry against float64.

Every check is componentwise (tests/numerics.py): an entry's error is bounded by the scale an error analysis gives that entry, so a
channel 1e-4 of the largest is checked as hard as the largest.  The tensor-wide 1e-5 bounds of tests/test_training.py are kept
beside it.  Inputs: unit Gaussian, post-ReLU, sparse 0/1 planes, per-channel scales log-uniform over 10^-4 .. 10^4; shapes on both
sides of every switch of the host code (split count, empty splits, odd tile counts, the 64 / 128-channel conv variants).
Each test prints "RATIO <kernel> <case> <worst |err| / (2^-24 scale)>" (run with -s to see them)."""
import pytest
import torch
import torch.nn.functional as F

import numerics as N

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _report(kernel, case, worst):
    print("RATIO %-6s %-34s %8.2f" % (kernel, case, worst))


def _log_scales(c, decades, gen):
    return 10.0 ** ((torch.rand(c, generator=gen, device="cuda") * 2 - 1) * decades)


def _operands(family, b, c, gen):
    """(x, dy) float32 [B, 90, C] (NHWC, what the kernels read)."""
    shape = (b, 90, c)
    rn = lambda: torch.randn(shape, generator=gen, device="cuda")
    if family == "gauss":
        return rn(), rn()
    if family == "relu":                                                # post-ReLU activations, signed gradient
        return torch.relu(rn() + 0.3), rn()
    if family == "sparse":                                              # 0/1 planes, like the network's input
        return (torch.rand(shape, generator=gen, device="cuda") < 0.1).float(), rn()
    if family == "scaled":                                              # channel scales over 10^-4 .. 10^4 on both operands
        return torch.relu(rn() + 0.3) * _log_scales(c, 4, gen), rn() * _log_scales(c, 4, gen)
    if family == "scaled_pos":                                          # ... non-negative: ref = scale, the bound is relative
        return torch.relu(rn() + 0.3) * _log_scales(c, 4, gen), torch.relu(rn() + 0.3) * _log_scales(c, 4, gen)
    raise ValueError(family)


def _nchw(t):
    b, _, c = t.shape
    return t.view(b, 10, 9, c).permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------- weight gradient

_SHAPES = [(c, b) for c in (64, 128, 256, 512) for b in (1, 2, 3, 17, 35, 255, 256, 257)] + [(256, 1024), (256, 2048), (512, 1024)]
_FAMILY_SHAPES = {"relu": [(64, 3), (128, 35), (256, 257), (512, 255), (256, 2048)],
                  "sparse": [(64, 17), (128, 256), (256, 3), (512, 1024)],
                  "scaled": [(64, 35), (64, 1), (128, 3), (256, 256), (512, 257), (512, 1024)],
                  "scaled_pos": [(64, 3), (128, 255), (256, 35), (512, 2)]}
_WGRAD_CASES = [(c, b, "gauss") for c, b in _SHAPES] + [(c, b, f) for f, s in _FAMILY_SHAPES.items() for c, b in s]


@pytest.mark.parametrize("channels,batch,family", _WGRAD_CASES)
def test_wino_wgrad_componentwise(channels, batch, family):
    """hip.wino_wgrad against the float64 im2col GEMM: every entry within KAPPA_WGRAD * 2^-24 * sum over taps of wgrad64(|x|, |dy|);
    the tensor-wide 1e-5 bound too; the scratch size gives the split count of the rule in tests/numerics.py."""
    from xiangqi_alphazero_amd import hip
    x, dy = _operands(family, batch, channels, _gen(1000 * channels + batch))
    nbytes = hip.lib().xq_wino_wgrad_scratch_bytes(batch, channels)
    assert nbytes == N.wgrad_splits(batch, channels) * 9 * channels * channels * 4
    dw = hip.wino_wgrad(x, dy)
    ref, scale = N.wgrad_ref_and_scale(_nchw(x), _nchw(dy))
    case = "C=%d B=%d %s splits=%d empty=%d" % (channels, batch, family, N.wgrad_splits(batch, channels),
                                               N.wgrad_empty_splits(batch, channels))
    worst = N.check_componentwise(dw, ref, scale, N.KAPPA_WGRAD, "wgrad " + case)
    _report("wgrad", "C=%d B=%d %s" % (channels, batch, family), worst)
    assert (dw.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


# ---------------------------------------------------------------------------------------------------- forward and data gradient

def _conv_case(channels, batch, seed):
    gen = _gen(seed)
    x = (torch.relu(torch.randn(batch, channels, 10, 9, generator=gen, device="cuda") + 0.3) * _log_scales(channels, 2, gen).view(1, -1, 1, 1))
    w = torch.randn(channels, channels, 3, 3, generator=gen, device="cuda") * (2.0 / (9 * channels)) ** 0.5
    gy = torch.randn(batch, channels, 10, 9, generator=gen, device="cuda") * _log_scales(channels, 2, gen).view(1, -1, 1, 1)
    return x.contiguous(memory_format=torch.channels_last), w, gy


def _run_conv(x, w, gy):
    from xiangqi_alphazero_amd import native_conv
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = native_conv.conv3x3(xg, wg)
    y.backward(gy)
    return y.detach(), xg.grad, wg.grad


@pytest.mark.parametrize("channels,batch,block", [(512, 544, None), (512, 545, None), (128, 37, "64"), (128, 37, "128"),
                                                  (256, 37, "64"), (256, 37, "128")])
def test_native_conv_train_direction_componentwise(channels, batch, block, monkeypatch):
    """native_conv.conv3x3 forward, data gradient and weight gradient on both conv variants (chosen by batch size at C = 512, forced
    by XQ_TRAIN_CONV_BLOCK otherwise), post-ReLU inputs and gradients with channel scales over 10^-2 .. 10^2."""
    from xiangqi_alphazero_amd import native_conv
    if block is None:
        monkeypatch.delenv("XQ_TRAIN_CONV_BLOCK", raising=False)
        assert native_conv._co_block(batch, channels) == (64 if batch == 544 else 128)
    else:
        monkeypatch.setenv("XQ_TRAIN_CONV_BLOCK", block)
        assert native_conv._co_block(batch, channels) == int(block)
    x, w, gy = _conv_case(channels, batch, channels + batch)
    y, gx, gw = _run_conv(x, w, gy)
    case = "C=%d B=%d block=%d" % (channels, batch, native_conv._co_block(batch, channels))
    yref, yscale = N.conv3x3_ref_and_scale(x, w)
    gref, gscale = N.conv3x3_ref_and_scale(gy, N.dgrad_filters(w))
    wref, wscale = N.wgrad_ref_and_scale(x, gy)
    for kernel, kappa, got, ref, scale in (("fwd", N.KAPPA_CONV, y, yref, yscale), ("dgrad", N.KAPPA_CONV, gx, gref, gscale),
                                           ("wgrad", N.KAPPA_WGRAD, gw, wref, wscale)):
        _report(kernel, case, N.check_componentwise(got, ref, scale, kappa, "%s %s" % (kernel, case)))
        assert (got.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item(), kernel


@pytest.mark.parametrize("channels,batch", [(128, 37), (256, 37), (512, 545)])
def test_conv_variants_are_identical_in_the_training_direction(channels, batch, monkeypatch):
    """The 64- and 128-output-channel kernels sum in the same order: the same forward output, data gradient and weight gradient."""
    x, w, gy = _conv_case(channels, batch, 7 * channels + batch)
    outs = []
    for block in ("64", "128"):
        monkeypatch.setenv("XQ_TRAIN_CONV_BLOCK", block)
        outs.append(_run_conv(x, w, gy))
    for a, b, what in zip(outs[0], outs[1], ("y", "dx", "dw")):
        assert torch.equal(a, b), what


# ---------------------------------------------------------------------------------------------------------------- BatchNorm

def _bn_reference_forward(x, r, gamma, beta, rm0, rv0, momentum, eps, relu):
    """float64 training-mode BatchNorm2d (+ residual, ReLU) of the float32 operands; per-channel statistics."""
    x64 = x.double()
    n = x.numel() // x.shape[1]
    mean = x64.mean(dim=(0, 2, 3))
    var = x64.var(dim=(0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x64 - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
    pre = gamma.double().view(1, -1, 1, 1) * xhat + beta.double().view(1, -1, 1, 1)
    if r is not None:
        pre = pre + r.double()
    y = torch.relu(pre) if relu else pre
    rm = (1 - momentum) * rm0 + momentum * mean
    rv = (1 - momentum) * rv0 + momentum * var * n / max(n - 1, 1)
    return dict(mean=mean, var=var, invstd=invstd, xhat=xhat, y=y, rm=rm, rv=rv, n=n)


def _per_channel(v, like):
    return v.view(1, -1, 1, 1).expand_as(like)


def _check_bn_forward(case, ref, x, r, gamma, beta, rm0, rv0, momentum, y, rm, rv):
    """y within KAPPA_BN * 2^-24 * (|gamma| max|xhat| + |beta| + max|r|) of its channel; running statistics within KAPPA_BN_RUNNING
    roundings of their two terms."""
    sc = gamma.double().abs() * ref["xhat"].abs().amax(dim=(0, 2, 3)) + beta.double().abs()
    if r is not None:
        sc = sc + r.double().abs().amax(dim=(0, 2, 3))
    worst = N.check_componentwise(y, ref["y"], _per_channel(sc, ref["y"]), N.KAPPA_BN, "bn y " + case)
    rm_scale = (1 - momentum) * rm0.abs() + momentum * ref["mean"].abs()
    rv_scale = (1 - momentum) * rv0.abs() + momentum * ref["var"] * ref["n"] / max(ref["n"] - 1, 1)
    worst_run = max(N.check_componentwise(rm, ref["rm"], rm_scale, N.KAPPA_BN_RUNNING, "bn running_mean " + case),
                    N.check_componentwise(rv, ref["rv"], rv_scale, N.KAPPA_BN_RUNNING, "bn running_var " + case))
    _report("bnrun", case, worst_run)
    return worst


def _check_bn_backward(case, ref, gamma, relu, y_kernel, gy, dx, dres, dgamma, dbeta):
    """Gradients against float64 with the ReLU mask of the kernel's own output (the operand of the backward kernels): dbeta within
    KAPPA_BN * 2^-24 * sum|g|, dgamma * sum|g xhat|, dx * |gamma| invstd (max|g| + sum|g| / n + max|xhat| sum|g xhat| / n) of its
    channel; the residual's gradient is g exactly."""
    g = gy.double() * (y_kernel > 0).double() if relu else gy.double()
    xhat, n = ref["xhat"], ref["n"]
    db, dg = g.sum(dim=(0, 2, 3)), (g * xhat).sum(dim=(0, 2, 3))
    sg, sgx = g.abs().sum(dim=(0, 2, 3)), (g * xhat).abs().sum(dim=(0, 2, 3))
    ga, inv = gamma.double(), ref["invstd"]
    dx_ref = _per_channel(ga * inv, g) * (g - _per_channel(db / n, g) - xhat * _per_channel(dg / n, g))
    dx_sc = ga.abs() * inv * (g.abs().amax(dim=(0, 2, 3)) + sg / n + xhat.abs().amax(dim=(0, 2, 3)) * sgx / n)
    worst = max(N.check_componentwise(dbeta, db, sg, N.KAPPA_BN, "bn dbeta " + case),
                N.check_componentwise(dgamma, dg, sgx, N.KAPPA_BN, "bn dgamma " + case),
                N.check_componentwise(dx, dx_ref, _per_channel(dx_sc, dx_ref), N.KAPPA_BN, "bn dx " + case))
    if dres is not None:
        assert torch.equal(dres, g.float()), "bn d_residual " + case
    return worst


def _bn_module(channels, momentum, eps, gen):
    bn = torch.nn.BatchNorm2d(channels, eps=eps, momentum=momentum).cuda().train()
    with torch.no_grad():
        sign = torch.where(torch.rand(channels, generator=gen, device="cuda") < 0.2, -1.0, 1.0)
        bn.weight.copy_(sign * (torch.rand(channels, generator=gen, device="cuda") + 0.5))
        bn.bias.copy_(torch.randn(channels, generator=gen, device="cuda") * 0.2)
        bn.running_mean.copy_(torch.randn(channels, generator=gen, device="cuda") * 0.1)
        bn.running_var.copy_(torch.rand(channels, generator=gen, device="cuda") + 0.5)
    return bn


def _bn_inputs(channels, batch, with_res, gen, shift=0.5):
    """x with channel standard deviations log-uniform over 10^-2 .. 10 and means shift * std * N(0, 1); residual and dL/dy with channel
    scales over 10^-2 .. 10^2."""
    std = _log_scales(channels, 1.5, gen) * 0.3
    mean = std * shift * torch.randn(channels, generator=gen, device="cuda")
    cl = torch.channels_last
    rn = lambda: torch.randn(batch, channels, 10, 9, generator=gen, device="cuda")
    x = (rn() * std.view(1, -1, 1, 1) + mean.view(1, -1, 1, 1)).contiguous(memory_format=cl)
    r = (rn() * _log_scales(channels, 2, gen).view(1, -1, 1, 1)).contiguous(memory_format=cl) if with_res else None
    gy = rn() * _log_scales(channels, 2, gen).view(1, -1, 1, 1)
    return x, r, gy


def _run_bn(bn, x, r, gy, relu):
    from xiangqi_alphazero_amd import native_conv
    xg = x.clone().requires_grad_(True)
    rg = r.clone().requires_grad_(True) if r is not None else None
    for p in bn.parameters():
        p.grad = None
    y = native_conv.bn_act(xg, bn, rg, relu)
    y.backward(gy)
    return y.detach(), xg.grad, None if rg is None else rg.grad, bn.weight.grad.clone(), bn.bias.grad.clone()


@pytest.mark.parametrize("batch", [1, 3, 600])
@pytest.mark.parametrize("channels", [64, 128, 256, 512])
def test_bn_act_componentwise(channels, batch):
    """native_conv.bn_act (k_bn_partial, k_bn_fwd_finalize, k_bn_apply, k_bn_dx) with momentum 0.3 and eps 1e-3 -- not torch's defaults,
    so both must reach the kernels -- with and without residual and ReLU; rows = 90 (B = 1: unbiased factor 90 / 89), 270 and
    54 000 (> NSEG * 100).  num_batches_tracked counts both steps."""
    from xiangqi_alphazero_amd import native_conv
    momentum, eps = 0.3, 1e-3
    for k, (with_res, relu) in enumerate(((False, False), (False, True), (True, False), (True, True))):
        gen = _gen(channels * 10 + batch * 100 + k)
        bn = _bn_module(channels, momentum, eps, gen)
        assert native_conv.bn_supported(bn) and bn.momentum == momentum and bn.eps == eps
        x, r, gy = _bn_inputs(channels, batch, with_res, gen)
        case = "C=%d B=%d res=%d relu=%d" % (channels, batch, with_res, relu)
        rm0, rv0 = bn.running_mean.double().clone(), bn.running_var.double().clone()
        y, dx, dres, dgamma, dbeta = _run_bn(bn, x, r, gy, relu)
        ref = _bn_reference_forward(x, r, bn.weight, bn.bias, rm0, rv0, momentum, eps, relu)
        wf = _check_bn_forward(case, ref, x, r, bn.weight, bn.bias, rm0, rv0, momentum, y, bn.running_mean, bn.running_var)
        wb = _check_bn_backward(case, ref, bn.weight, relu, y, gy, dx, dres, dgamma, dbeta)
        _report("bn", case, max(wf, wb))
        assert int(bn.num_batches_tracked) == 1
        rm1, rv1 = bn.running_mean.double().clone(), bn.running_var.double().clone()
        _run_bn(bn, x, r, gy, relu)                                       # second step: statistics move on from the first
        assert int(bn.num_batches_tracked) == 2
        ref2 = _bn_reference_forward(x, r, bn.weight, bn.bias, rm1, rv1, momentum, eps, relu)
        _check_bn_forward(case + " step 2", ref2, x, r, bn.weight, bn.bias, rm1, rv1, momentum, y, bn.running_mean, bn.running_var)


def test_bn_act_shifted_mean_is_no_worse_than_torch():
    """Channels with mean / std = 100: the float32 save_mean limits every implementation.  The native y, dx and dgamma are no further
    from float64 than twice torch's own float32 F.batch_norm on the same GPU."""
    gen = _gen(77)
    c, b, momentum, eps = 256, 64, 0.3, 1e-3
    std = _log_scales(c, 1, gen)
    cl = torch.channels_last
    x = (torch.randn(b, c, 10, 9, generator=gen, device="cuda") * std.view(1, -1, 1, 1) + 100 * std.view(1, -1, 1, 1)).contiguous(memory_format=cl)
    gy = torch.randn(b, c, 10, 9, generator=gen, device="cuda")
    bn = _bn_module(c, momentum, eps, gen)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    y, dx, _, dgamma, _ = _run_bn(bn, x, None, gy, False)

    def torch_f32():
        xg = x.clone().requires_grad_(True)
        wg, bg = bn.weight.detach().clone().requires_grad_(True), bn.bias.detach().clone().requires_grad_(True)
        out = F.batch_norm(xg, rm0.clone(), rv0.clone(), wg, bg, True, momentum, eps)
        out.backward(gy)
        return out.detach(), xg.grad, wg.grad

    def f64():
        xg = x.double().requires_grad_(True)
        wg, bg = bn.weight.detach().double().requires_grad_(True), bn.bias.detach().double().requires_grad_(True)
        out = F.batch_norm(xg, rm0.double(), rv0.double(), wg, bg, True, momentum, eps)
        out.backward(gy.double())
        return out.detach(), xg.grad, wg.grad

    for what, nat, tf, ref in zip(("y", "dx", "dgamma"), (y, dx, dgamma), torch_f32(), f64()):
        e_nat = (nat.double() - ref).abs().max().item()
        e_torch = (tf.double() - ref).abs().max().item()
        print("SHIFTED %-6s native %.3e torch %.3e" % (what, e_nat, e_torch))
        assert e_nat <= 2 * e_torch, (what, e_nat, e_torch)


# ------------------------------------------------------------------------------------------------------------------ determinism

def test_wgrad_and_batchnorm_are_deterministic():
    """Fixed-order reductions (split partials, per-segment float64 sums): two calls on the same inputs give the same bits."""
    import copy
    from xiangqi_alphazero_amd import hip
    for c, b in ((64, 35), (256, 257), (512, 1024)):
        x, dy = _operands("gauss", b, c, _gen(c + b))
        assert torch.equal(hip.wino_wgrad(x, dy), hip.wino_wgrad(x, dy)), (c, b)
    gen = _gen(5)
    bn = _bn_module(256, 0.3, 1e-3, gen)
    x, r, gy = _bn_inputs(256, 600, True, gen)
    bn2 = copy.deepcopy(bn)
    a, b_ = _run_bn(bn, x, r, gy, True), _run_bn(bn2, x, r, gy, True)
    for u, v in zip(a, b_):
        assert torch.equal(u, v)
    assert torch.equal(bn.running_mean, bn2.running_mean) and torch.equal(bn.running_var, bn2.running_var)


# ---------------------------------------------------------------------------------------------------- in situ: one real train step

def test_every_kernel_call_of_a_real_step_against_float64(monkeypatch):
    """One forward and backward of XiangqiNet(128, 3) at batch 96 on the native step, with every call of hip.wino_conv3x3, hip.wino_wgrad
    and the two BatchNorm entry points (native_conv.BnAct, which call xq_bn_train_forward / xq_bn_train_backward) captured with its
    real float32 operands and results, each checked against float64 of the same operands.  No ReLU mask can flip between the two:
    each reference sees exactly what its kernel saw."""
    import copy
    from xiangqi_alphazero_amd import hip, model, native_conv, weights
    net = model.XiangqiNet(128, 3)
    net.load_state_dict(weights.make_state_dict(128, 3, seed=9))
    net = net.cuda().train().use_native_conv(True)
    gen = torch.Generator().manual_seed(4)
    x = (torch.rand(96, 15, 10, 9, generator=gen) < 0.1).float().cuda()
    pi = torch.softmax(torch.randn(96, 8100, generator=gen), 1).cuda()
    z = (torch.rand(96, 1, generator=gen) * 2 - 1).cuda()

    filters, convs, wgrads, bn_fwd, bn_bwd = {}, [], [], [], []
    orig_tf, orig_conv, orig_wgrad = hip.wino_transform_filters_device, hip.wino_conv3x3, hip.wino_wgrad
    orig_bf, orig_bb = native_conv.BnAct.forward, native_conv.BnAct.backward

    def tf(w, co_block=64, dgrad=False, out=None, both=False):
        u = orig_tf(w, co_block, dgrad, out, both)
        for k, t in enumerate(u if both else [u]):
            filters[t.data_ptr()] = (w.detach().clone(), bool(k) if both else dgrad)
        return u

    def conv(xv, u, bias, out, residual=None, relu=True, reverse=False):
        assert residual is None and not relu and not reverse and not bias.any()
        res = orig_conv(xv, u, bias, out, residual, relu, reverse)
        convs.append((xv.clone(), filters[u.data_ptr()], out.clone()))
        return res

    def wgrad(xv, gv):
        dw = orig_wgrad(xv, gv)
        wgrads.append((xv.clone(), gv.clone(), dw.clone()))
        return dw

    def bf(ctx, xx, residual, gamma, beta, rmean, rvar, momentum, eps, relu, nbt=None):
        before = (rmean.double().clone(), rvar.double().clone())
        y = orig_bf(ctx, xx, residual, gamma, beta, rmean, rvar, momentum, eps, relu, nbt)
        bn_fwd.append(dict(x=xx.detach().clone(), r=None if residual is None else residual.detach().clone(), gamma=gamma.detach().clone(),
                           beta=beta.detach().clone(), rm0=before[0], rv0=before[1], momentum=momentum, eps=eps, relu=relu,
                           y=y.detach().clone(), rm=rmean.detach().clone(), rv=rvar.detach().clone()))
        return y

    def bb(ctx, gy):
        xv, y, gamma, _, _ = ctx.saved_tensors
        grads = orig_bb(ctx, gy)
        bn_bwd.append(dict(x=xv.permute(0, 3, 1, 2).clone(), y=y.permute(0, 3, 1, 2).clone(), gamma=gamma.clone(), relu=ctx.relu,
                           gy=gy.clone(), dx=grads[0].clone(), dres=None if grads[1] is None else grads[1].clone(),
                           dgamma=grads[2].clone(), dbeta=grads[3].clone()))
        return grads

    monkeypatch.setattr(hip, "wino_transform_filters_device", tf)
    monkeypatch.setattr(hip, "wino_conv3x3", conv)
    monkeypatch.setattr(hip, "wino_wgrad", wgrad)
    monkeypatch.setattr(native_conv.BnAct, "forward", staticmethod(bf))
    monkeypatch.setattr(native_conv.BnAct, "backward", staticmethod(bb))
    logits, value = net(x)
    loss = -torch.mean(torch.sum(pi * F.log_softmax(logits, dim=1), dim=1)) + F.mse_loss(value, z)
    loss.backward()
    torch.cuda.synchronize()
    assert (len(convs), len(wgrads), len(bn_fwd), len(bn_bwd)) == (12, 6, 7, 7)
    assert sum(d for _, (_, d), _ in convs) == 6

    worst = {"fwd": 0.0, "dgrad": 0.0, "wgrad": 0.0, "bn": 0.0}
    for k, (xv, (w, dgrad), out) in enumerate(convs):
        kind = "dgrad" if dgrad else "fwd"
        ref, scale = N.conv3x3_ref_and_scale(_nchw(xv), N.dgrad_filters(w) if dgrad else w)
        worst[kind] = max(worst[kind], N.check_componentwise(_nchw(out), ref, scale, N.KAPPA_CONV, "in-situ conv call %d (%s)" % (k, kind)))
    for k, (xv, gv, dw) in enumerate(wgrads):
        ref, scale = N.wgrad_ref_and_scale(_nchw(xv), _nchw(gv))
        worst["wgrad"] = max(worst["wgrad"], N.check_componentwise(dw, ref, scale, N.KAPPA_WGRAD, "in-situ wgrad call %d" % k))
    for k, f in enumerate(bn_fwd):
        case = "in-situ bn call %d" % k
        ref = _bn_reference_forward(f["x"], f["r"], f["gamma"], f["beta"], f["rm0"], f["rv0"], f["momentum"], f["eps"], f["relu"])
        worst["bn"] = max(worst["bn"], _check_bn_forward(case, ref, f["x"], f["r"], f["gamma"], f["beta"], f["rm0"], f["rv0"],
                                                         f["momentum"], f["y"], f["rm"], f["rv"]))
    for k, bw in enumerate(bn_bwd):                         # backward runs the layers in reverse order
        f = bn_fwd[len(bn_fwd) - 1 - k]
        assert torch.equal(bw["x"], f["x"]) and torch.equal(bw["y"], f["y"])
        ref = _bn_reference_forward(f["x"], f["r"], f["gamma"], f["beta"], f["rm0"], f["rv0"], f["momentum"], f["eps"], f["relu"])
        worst["bn"] = max(worst["bn"], _check_bn_backward("in-situ bn backward call %d" % k, ref, bw["gamma"], bw["relu"], bw["y"],
                                                          bw["gy"], bw["dx"], bw["dres"], bw["dgamma"], bw["dbeta"]))
    for kind, v in worst.items():
        _report(kind, "in-situ 128x3 B=96", v)
