"""The evaluator's kernels (csrc/xq_conv.hip, xq_conv_bf16.hip, xq_nn.hip), entry by entry against float64.

The counterpart of tests/test_train_kernels.py for the inference direction: every check is componentwise (tests/numerics.py), so
a channel or a Winograd tile at 1e-3 of the largest scale is checked as hard as the largest, and a failure names the channel and
the tile.  The absolute-bound tests of tests/test_nn_parity.py and tests/test_nn_fullsize.py stay beside these.  Operands: unit
Gaussian, post-ReLU, per-channel activation scales log-uniform over 10^-4 .. 10^4, filters scaled per output channel over
10^-2 .. 10^2 as folded BatchNorm gives them (bias and residual at their own scales, channel 7 at 1e-3), the encoder's planes of
corpus boards for the stem.  Shapes on both sides of every switch of the launch code: every legal co_block, ragged last tile
groups, grid rows with fewer tile groups than `per`, the 32-bit buffer-offset limit, and the *_live entry points.
The bf16 throughput convolution is held to its OWN arithmetic (numerics.wino_bf16_ref_and_scale), not to the fp32 result.
Each test prints "RATIO <kernel> <case> <worst |err| / (2^-24 scale)>" (run with -s to see them)."""
import numpy as np
import pytest
import torch

import golden_io as G
import numerics as N

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _report(kernel, case, worst):
    print("RATIO %-6s %-44s %8.2f" % (kernel, case, worst))


def _log_scales(c, decades, gen):
    return 10.0 ** ((torch.rand(c, generator=gen, device="cuda") * 2 - 1) * decades)


def _nchw(t):
    b, _, c = t.shape
    return t.view(b, 10, 9, c).permute(0, 3, 1, 2)


FAMILIES = ("gauss", "relu", "scaled", "folded")


def _conv_operands(family, b, c, gen):
    """x, w, bias, residual: x and residual float32 [B, 90, C], w [C, C, 3, 3], bias [C].  'folded': rows of w and the bias scaled
    per output channel over 10^-2 .. 10^2, the residual per channel over 10^-2 .. 10^2, and channel 7 at 1e-3 in all three (bias 3e-4)."""
    rn = lambda *s: torch.randn(*s, generator=gen, device="cuda")
    x = rn(b, 90, c)
    w = rn(c, c, 3, 3) * (2.0 / (9 * c)) ** 0.5
    bias = rn(c) * 0.1
    res = rn(b, 90, c)
    if family == "relu":
        x = torch.relu(x + 0.3)
    elif family == "scaled":
        x = torch.relu(x + 0.3) * _log_scales(c, 4, gen)
        res = res * _log_scales(c, 4, gen)
    elif family == "folded":
        x = torch.relu(x + 0.3)
        s = _log_scales(c, 2, gen)
        s[7] = 1e-3
        sr = _log_scales(c, 2, gen)
        sr[7] = 1e-3
        w, bias, res = w * s.view(-1, 1, 1, 1), rn(c) * 0.3 * s, res * sr
        bias[7] = 3e-4                                                  # not left to chance: 0.3 times the channel's scale
    return x.contiguous(), w.contiguous(), bias.contiguous(), res.contiguous()


# ------------------------------------------------------------------------------------------------------ k_wino_conv (inference)

_CONV_BLOCKS = [(c, blk) for c in (64, 128, 256, 512) for blk in (64, 128) if c % blk == 0]
_SWITCHES = [(False, True, False), (True, True, True), (True, False, False), (False, False, True)]     # residual, relu, reverse


def _groups(b):
    return (b * 15 + 31) // 32


@pytest.mark.parametrize("batch", [1, 2, 3, 35])
@pytest.mark.parametrize("channels,block", _CONV_BLOCKS)
def test_wino_conv_componentwise(channels, block, batch):
    """hip.wino_conv3x3 with the evaluator's epilogue: every operand family, each with its own (residual, ReLU, reverse) switch
    setting, per entry within KAPPA_EVAL_CONV * 2^-24 * (conv64(|x|, |w|) + |bias| + |residual|).  B = 35: 17 tile groups, the last
    one partial, and a partial last grid row for every per = 8 / (C / block) > 1; B = 1, 2, 3: one or two groups.  The reversed
    launch gives the same bits as the forward one."""
    from xiangqi_alphazero_amd import hip
    per = 8 // (channels // block)
    assert per == 1 or _groups(35) % per
    for k, family in enumerate(FAMILIES):
        with_res, relu, reverse = _SWITCHES[(k + batch) % 4]
        x, w, bias, res = _conv_operands(family, batch, channels, _gen(channels * 7 + block + batch * 100 + k))
        u = hip.wino_transform_weights(w, block)
        residual = res if with_res else None
        out = torch.full_like(x, SENTINEL)
        hip.wino_conv3x3(x, u, bias, out, residual, relu, reverse)
        other = hip.wino_conv3x3(x, u, bias, torch.full_like(x, SENTINEL), residual, relu, not reverse)
        assert torch.equal(out, other), family
        ref, scale = N.conv_epilogue_ref_and_scale(_nchw(x), w, bias, None if residual is None else _nchw(residual), relu)
        case = "C=%d block=%d B=%d %s res=%d relu=%d rev=%d" % (channels, block, batch, family, with_res, relu, reverse)
        _report("conv", case, N.check_componentwise(_nchw(out), ref, scale, N.KAPPA_EVAL_CONV, "wino_conv " + case))


# ------------------------------------------------------------------------------------------------------- the 4 GB buffer limit

EDGE_C, EDGE_B = 512, 23301


def test_buffer_offset_limit_at_512_channels():
    """B * 90 * C * 4 < 2^32 is the limit of the kernels' 32-bit buffer offsets: at C = 512 the largest batch, 23 301 boards (4.29 GB
    per tensor), is accepted by both fp32 variants and the bf16 kernel, and its first and last 64 boards meet the per-entry bound;
    23 302 boards raise XqError and leave the output untouched."""
    from xiangqi_alphazero_amd import hip
    assert EDGE_B * 90 * EDGE_C * 4 < 1 << 32 <= (EDGE_B + 1) * 90 * EDGE_C * 4
    gen = _gen(4242)
    x = torch.randn(EDGE_B + 1, 90, EDGE_C, generator=gen, device="cuda")
    res = torch.randn(EDGE_B, 90, EDGE_C, generator=gen, device="cuda")
    w = torch.randn(EDGE_C, EDGE_C, 3, 3, generator=gen, device="cuda") * (2.0 / (9 * EDGE_C)) ** 0.5
    bias = torch.randn(EDGE_C, generator=gen, device="cuda") * 0.1
    out = torch.full_like(x, SENTINEL)
    ends = torch.cat([torch.arange(64), torch.arange(EDGE_B - 64, EDGE_B)]).cuda()
    runs = [("fp32 block=64", hip.wino_conv3x3, hip.wino_transform_weights(w, 64)),
            ("fp32 block=128", hip.wino_conv3x3, hip.wino_transform_weights(w, 128)),
            ("bf16", hip.wino_conv3x3_bf16, hip.wino_transform_weights_bf16(w))]
    for name, fn, u in runs:
        with pytest.raises(hip.XqError):
            fn(x, u, bias, out, None, True)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), name
    for k, (name, fn, u) in enumerate(runs):
        residual = res if k != 1 else None
        fn(x[:EDGE_B], u, bias, out[:EDGE_B], residual, k != 2)
        torch.cuda.synchronize()
        assert bool((out[EDGE_B] == SENTINEL).all()), name
        xs, os_ = x[ends], out[ends]
        rs = None if residual is None else res[ends]
        if name == "bf16":
            ref, scale, allow, _ = N.wino_bf16_ref_and_scale(xs, u, bias, rs, False)
            worst = N.check_componentwise(_nchw(os_), ref, scale, N.KAPPA_BF16, "edge " + name, allow)
        else:
            ref, scale = N.conv_epilogue_ref_and_scale(_nchw(xs), w, bias, None if rs is None else _nchw(rs), True)
            worst = N.check_componentwise(_nchw(os_), ref, scale, N.KAPPA_EVAL_CONV, "edge " + name)
        _report("bf16" if name == "bf16" else "conv", "C=512 B=23301 %s ends" % name, worst)
        out[:EDGE_B].fill_(SENTINEL)


# ------------------------------------------------------------------------------------------------------------------ k_stem_conv

def _corpus_planes(games, seed):
    from xiangqi_alphazero_amd import hip
    d = G.corpus()
    idx = torch.randint(0, len(d["board"]), (games,), generator=torch.Generator().manual_seed(seed)).numpy()
    return hip.encode(torch.from_numpy(d["board"][idx]).cuda(), torch.from_numpy(d["side"][idx].astype(np.int8)).cuda())


def _stem_operands(family, games, c, gen):
    planes = _corpus_planes(games, games + c) if family != "gauss" else torch.randn(games, 15, 10, 9, generator=gen, device="cuda")
    w = torch.randn(c, 15, 3, 3, generator=gen, device="cuda") * 0.2
    bias = torch.randn(c, generator=gen, device="cuda") * 0.1
    if family == "folded":
        s = _log_scales(c, 2, gen)
        w, bias = w * s.view(-1, 1, 1, 1), bias * s
    return planes.contiguous(), w, bias


@pytest.mark.parametrize("channels", [64, 128, 256, 512])
def test_stem_conv_componentwise(channels):
    """hip.stem_conv on the encoder's planes of corpus boards (and Gaussian planes: the kernel skips zero inputs, so it must be right
    for any input), filters per output channel over 10^-2 .. 10^2: relu(conv64 + bias) within KAPPA_STEM * 2^-24 * (conv64(|x|, |w|)
    + |bias|)."""
    from xiangqi_alphazero_amd import hip
    for k, (family, games) in enumerate((("planes", 37), ("folded", 64), ("gauss", 5))):
        planes, w, bias = _stem_operands(family, games, channels, _gen(channels + 10 * k))
        out = torch.full((games, 90, channels), SENTINEL, device="cuda")
        hip.stem_conv(planes, hip.stem_weights(w).contiguous(), bias, out)
        ref, scale = N.conv_epilogue_ref_and_scale(planes, w, bias, None, True)
        case = "C=%d G=%d %s" % (channels, games, family)
        _report("stem", case, N.check_componentwise(_nchw(out), ref, scale, N.KAPPA_STEM, "stem " + case))


# ------------------------------------------------------------------------------------------------------------------ k_heads_1x1

@pytest.mark.parametrize("channels", [64, 128, 256, 512])
def test_heads_1x1_componentwise(channels):
    """hip.heads_1x1 for row counts around multiples of 16 (a wave takes 16 rows) and the rows of 37 positions; tower outputs with
    channel scales over 10^-4 .. 10^4, head weights per output over 10^-2 .. 10^2: relu(h W^T + b) within KAPPA_HEADS * 2^-24 *
    (|h| |W|^T + |b|) for both outputs."""
    from xiangqi_alphazero_amd import hip
    for rows in (1, 15, 16, 17, 31, 33, 90 * 37):
        gen = _gen(channels * 1000 + rows)
        h = torch.relu(torch.randn(rows, channels, generator=gen, device="cuda") + 0.3) * _log_scales(channels, 4, gen)
        s = _log_scales(36, 2, gen)
        w = torch.randn(36, channels, generator=gen, device="cuda") * channels ** -0.5 * s.view(-1, 1)
        bias = torch.randn(36, generator=gen, device="cuda") * s
        p, v = hip.heads_1x1(h.contiguous(), w.contiguous(), bias)
        ref, scale = N.heads_ref_and_scale(h, w, bias)
        case = "C=%d R=%d" % (channels, rows)
        _report("heads", case, N.check_componentwise(torch.cat([p, v], 1), ref, scale, N.KAPPA_HEADS, "heads " + case))


# --------------------------------------------------------------------------------------------------------------- k_policy_legal

_COUNTS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, -1, -100]


def _policy_operands(games, gen, small_plane=True):
    feat = torch.relu(torch.randn(games, 2880, generator=gen, device="cuda"))
    if small_plane:
        feat.view(games, 90, 32)[:, :, 5] *= 1e-3                   # one policy plane at 1e-3 of the others
    w = torch.randn(8100, 2880, generator=gen, device="cuda") * 0.02
    bias = torch.randn(8100, generator=gen, device="cuda") * 0.1
    cpu = torch.Generator().manual_seed(games)
    moves = torch.stack([torch.randperm(8100, generator=cpu)[:128] for _ in range(games)])
    moves[0, 0], moves[1, 1], moves[2, 63], moves[3, 127] = 0, 8099, 8099, 0      # the first and last action ids
    moves[4, :2] = torch.tensor([8099, 0])
    counts = torch.randint(0, 129, (games,), generator=cpu).to(torch.int32)
    counts[:len(_COUNTS)] = torch.tensor(_COUNTS, dtype=torch.int32)
    m16 = torch.from_numpy(moves.numpy().astype(np.uint16).view(np.int16)).cuda()
    return feat, w, bias, moves.cuda(), m16, counts.cuda()


def _check_policy(case, out, feat, w, bias, moves, counts, rows):
    """Per entry for m < clamp(count, 0, 128); the sentinel elsewhere."""
    ref, scale = N.policy_legal_ref_and_scale(feat[rows], w, bias, moves[rows])
    valid = torch.arange(128, device="cuda").view(1, -1) < counts[rows].clamp(0, 128).view(-1, 1)
    got = out[rows]
    assert bool((got[~valid] == SENTINEL).all()), case
    worst = N.check_componentwise(torch.where(valid, got, ref.float()), ref, scale, N.KAPPA_POLICY, "policy " + case)
    return worst


def test_policy_head_legal_componentwise():
    """hip.policy_head_legal with counts 0, 1, 2, 63, 64, 65, 127, 128 and counts above 128 and below 0 (clamped), action ids 0 and
    8099, one policy plane at 1e-3 of the others: each logit within KAPPA_POLICY * 2^-24 * (sum_k |feat_k| |W[a, k]| + |bias[a]|);
    entries past a game's count untouched."""
    from xiangqi_alphazero_amd import hip
    games = 37
    feat, w, bias, moves, m16, counts = _policy_operands(games, _gen(31))
    out = torch.full((games, 128), SENTINEL, device="cuda")
    hip.policy_head_legal(feat, w, bias, m16, counts, out)
    worst = _check_policy("G=37", out, feat, w, bias, moves, counts, slice(0, games))
    _report("policy", "G=37 counts 0..128, >128, <0", worst)


# ----------------------------------------------------------------------------------------------------------------- k_value_head

def _value_operands(games, gen, saturate=False):
    vf = torch.relu(torch.randn(games, 360, generator=gen, device="cuda"))
    w1 = torch.randn(128, 360, generator=gen, device="cuda") * 0.08
    b1 = torch.randn(128, generator=gen, device="cuda") * 0.1
    w2 = torch.randn(128, generator=gen, device="cuda")
    w2 = w2.abs() * 3.0 if saturate else w2 * 0.1                  # saturate: w2 . h of order 100, tanh = 1 in float32
    b2 = torch.randn(1, generator=gen, device="cuda") * 0.1
    # hidden units 0 .. 31 of game 0 with pre-activations within a few float32 roundings of 0
    b1[:32] = -(vf[0].double() @ w1[:32].double().t()).float()
    return vf, w1, b1, w2, b2


@pytest.mark.parametrize("games", [1, 3, 4, 5, 8191])
def test_value_head_componentwise(games):
    """hip.value_head (VGB = 4 games per block: 1, 3, 4, 5 and a ragged 8191), hidden units with pre-activations near 0 (the ReLU
    kink), and outputs in tanh's saturated range (|w2 . h| >> 1): within KAPPA_VALUE * 2^-24 * numerics.value_ref_and_scale."""
    from xiangqi_alphazero_amd import hip
    for saturate in (False, True):
        vf, w1, b1, w2, b2 = _value_operands(games, _gen(games * 2 + saturate), saturate)
        got = hip.value_head(vf, w1.t().contiguous(), b1, w2, b2)
        ref, scale = N.value_ref_and_scale(vf, w1, b1, w2, b2)
        if saturate:
            assert ref.abs().max().item() > 0.999
        case = "G=%d%s" % (games, " saturated" if saturate else "")
        _report("value", case, N.check_componentwise(got.view(-1, 1), ref.view(-1, 1), scale.view(-1, 1), N.KAPPA_VALUE, "value " + case))


# --------------------------------------------------------------------------------------------------------- k_wino_conv_bf16

@pytest.mark.parametrize("batch", [3, 35])
@pytest.mark.parametrize("channels", [128, 256, 512])
def test_wino_conv_bf16_componentwise(channels, batch):
    """hip.wino_conv3x3_bf16 against its own arithmetic -- the kernel's bf16 U, its float32 input transform rounded to bf16 (nearest
    even), float64 products, sums and output transform -- per entry within KAPPA_BF16 * 2^-24 * the same pipeline on |U|, |V|, |A|
    plus |bias| + |residual|, plus one bf16 ulp per V whose rounding one float32 ulp would flip (counted, printed).  Ragged batches,
    every operand family, residual, ReLU and reverse."""
    from xiangqi_alphazero_amd import hip
    for k, family in enumerate(FAMILIES):
        with_res, relu, reverse = _SWITCHES[(k + batch) % 4]
        x, w, bias, res = _conv_operands(family, batch, channels, _gen(channels * 11 + batch * 100 + k))
        u = hip.wino_transform_weights_bf16(w)
        residual = res if with_res else None
        out = hip.wino_conv3x3_bf16(x, u, bias, torch.full_like(x, SENTINEL), residual, relu, reverse)
        other = hip.wino_conv3x3_bf16(x, u, bias, torch.full_like(x, SENTINEL), residual, relu, not reverse)
        assert torch.equal(out, other), family
        ref, scale, allow, fragile = N.wino_bf16_ref_and_scale(x, u, bias, residual, relu)
        case = "C=%d B=%d %s res=%d relu=%d rev=%d" % (channels, batch, family, with_res, relu, reverse)
        worst = N.check_componentwise(_nchw(out), ref, scale, N.KAPPA_BF16, "bf16 " + case, allow)
        needed = int(((_nchw(out).double() - ref).abs() > N.KAPPA_BF16 * N.U32 * scale).sum())
        print("BF16-ALLOWANCE %s fragile V %d, entries that needed the allowance %d" % (case, fragile, needed))
        _report("bf16", case, worst)


# ---------------------------------------------------------------------------------------------------------- the *_live entry points

CAP = 37


def _live_counts():
    return (0, 1, CAP - 1, CAP)


def _n(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def _poison(t, n):
    """NaN in rows >= n of an input (what a dead slot may hold)."""
    t = t.clone()
    t[n:] = float("nan")
    return t


@pytest.mark.parametrize("kernel", ["conv64", "conv128", "bf16"])
def test_live_conv_entry_points(kernel):
    """xq_wino_conv3x3_live (both variants) and xq_wino_conv3x3_bf16_live at n_live = 0, 1, cap - 1, cap with NaN in the dead input and
    residual rows: live rows meet the per-entry bound, dead rows keep their sentinel bit for bit."""
    from xiangqi_alphazero_amd import hip
    c = 256
    x, w, bias, res = _conv_operands("folded", CAP, c, _gen(99))
    u = hip.wino_transform_weights_bf16(w) if kernel == "bf16" else hip.wino_transform_weights(w, int(kernel[4:]))
    fn = hip.wino_conv3x3_bf16 if kernel == "bf16" else hip.wino_conv3x3
    for n in _live_counts():
        xp, rp = _poison(x, n), _poison(res, n)
        out = torch.full_like(x, SENTINEL)
        fn(xp, u, bias, out, rp, True, False, n_live=_n(n))
        assert bool((out[n:] == SENTINEL).all()), (kernel, n)
        if n == 0:
            continue
        case = "live C=%d n=%d/%d" % (c, n, CAP)
        if kernel == "bf16":
            ref, scale, allow, _ = N.wino_bf16_ref_and_scale(x[:n], u, bias, res[:n], True)
            worst = N.check_componentwise(_nchw(out[:n]), ref, scale, N.KAPPA_BF16, "bf16 " + case, allow)
        else:
            ref, scale = N.conv_epilogue_ref_and_scale(_nchw(x[:n]), w, bias, _nchw(res[:n]), True)
            worst = N.check_componentwise(_nchw(out[:n]), ref, scale, N.KAPPA_EVAL_CONV, kernel + " " + case)
        _report("bf16" if kernel == "bf16" else "conv", case + " " + kernel, worst)


def test_live_stem_heads_policy_value_entry_points():
    """xq_stem_conv_live, xq_heads_1x1_live (n_live in positions of 90 rows), xq_policy_head_legal_live and xq_value_head_live at
    n_live = 0, 1, cap - 1, cap, NaN in the dead input rows: live rows within their kernel's bound, dead rows untouched."""
    from xiangqi_alphazero_amd import hip
    c = 128
    gen = _gen(123)
    planes, ws, bs = _stem_operands("planes", CAP, c, gen)
    h = torch.relu(torch.randn(CAP * 90, c, generator=gen, device="cuda") + 0.3) * _log_scales(c, 4, gen)
    wh = torch.randn(36, c, generator=gen, device="cuda") * c ** -0.5
    bh = torch.randn(36, generator=gen, device="cuda") * 0.1
    feat, wp, bp, moves, m16, counts = _policy_operands(CAP, gen)
    vf, w1, b1, w2, b2 = _value_operands(CAP, gen)
    worst = {"stem": 0.0, "heads": 0.0, "policy": 0.0, "value": 0.0}
    for n in _live_counts():
        out = torch.full((CAP, 90, c), SENTINEL, device="cuda")
        hip.stem_conv(_poison(planes, n), hip.stem_weights(ws).contiguous(), bs, out, n_live=_n(n))
        p, v = torch.full((CAP * 90, 32), SENTINEL, device="cuda"), torch.full((CAP * 90, 4), SENTINEL, device="cuda")
        hip.heads_1x1(_poison(h, 90 * n), wh, bh, n_live=_n(n), out=(p, v))
        pol = torch.full((CAP, 128), SENTINEL, device="cuda")
        hip.policy_head_legal(_poison(feat, n), wp, bp, m16, counts, pol, n_live=_n(n))
        val = torch.full((CAP,), SENTINEL, device="cuda")
        hip.value_head(_poison(vf, n), w1.t().contiguous(), b1, w2, b2, n_live=_n(n), out=val)
        assert bool((out[n:] == SENTINEL).all()) and bool((p[90 * n:] == SENTINEL).all()) and bool((v[90 * n:] == SENTINEL).all())
        assert bool((pol[n:] == SENTINEL).all()) and bool((val[n:] == SENTINEL).all())
        if n == 0:
            continue
        ref, scale = N.conv_epilogue_ref_and_scale(planes[:n], ws, bs, None, True)
        worst["stem"] = max(worst["stem"], N.check_componentwise(_nchw(out[:n]), ref, scale, N.KAPPA_STEM, "stem live n=%d" % n))
        ref, scale = N.heads_ref_and_scale(h[:90 * n], wh, bh)
        worst["heads"] = max(worst["heads"], N.check_componentwise(torch.cat([p[:90 * n], v[:90 * n]], 1), ref, scale, N.KAPPA_HEADS,
                                                                   "heads live n=%d" % n))
        worst["policy"] = max(worst["policy"], _check_policy("live n=%d" % n, pol, feat, wp, bp, moves, counts, slice(0, n)))
        ref, scale = N.value_ref_and_scale(vf[:n], w1, b1, w2, b2)
        worst["value"] = max(worst["value"], N.check_componentwise(val[:n].view(-1, 1), ref.view(-1, 1), scale.view(-1, 1),
                                                                   N.KAPPA_VALUE, "value live n=%d" % n))
    for kernel, r in worst.items():
        _report(kernel, "live n=1,%d,%d" % (CAP - 1, CAP), r)
