"""Float64 references of the train-step and evaluator kernels and a componentwise comparator.

A bound relative to the largest entry of a tensor does not check the small entries at all: a channel whose activations are 1e-4 of
the largest one can be wrong by 100 % and pass.  The comparator here bounds every entry by the scale a rounding-error analysis gives
it instead:

  * convolution (forward, data gradient):  scale = conv64(|x|, |w|), the float64 convolution of absolute values;
  * weight gradient:  scale[co, ci] = sum over the 9 taps of wgrad64(|x|, |dy|)[co, ci], broadcast over the taps (the Winograd
    transforms mix the taps of one channel pair);
  * assertion:  |got - ref64| <= kappa * 2^-24 * scale, entry by entry.

  * the evaluator (tests/test_eval_kernels.py):  the same with the epilogue's |bias| + |residual| added, |h| |W|^T + |b| for the
    1x1 heads and the policy rows, and for the bf16 convolution its own arithmetic (wino_bf16_ref_and_scale).

The references are im2col GEMMs in float64, in batch chunks, on whatever device the operands are on (CPU in the CPU tests).
Tensors are logical [B, C, 10, 9] (any memory format); filters and weight gradients [C_out, C_in, 3, 3].
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24                     # unit roundoff of float32

# kappa per kernel family: 2 to 4 times the worst |err| / (2^-24 * scale) measured on an MI355X over every case of
# tests/test_train_kernels.py (all the kernels are deterministic: the same seeds give the same ratios on every run)
KAPPA_CONV = 64                      # k_wino_conv forward and data gradient; worst 29.1 (data gradient of a real 128x3 step)
KAPPA_WGRAD = 4                      # k_wino_wgrad + k_wgrad_reduce; worst 1.08 (C = 128, B = 255, non-negative scaled operands)
KAPPA_BN = 8                         # k_bn_* (y, dx, dgamma, dbeta) against per-channel scales; worst 3.34 (C = 256, B = 600)
KAPPA_BN_RUNNING = 4                 # running statistics: one float32 rounding of a float64 value
# the evaluator, over every case of tests/test_eval_kernels.py (same rule; the references and scales are the functions below)
KAPPA_EVAL_CONV = 128                # k_wino_conv, inference epilogue, narrow and wide; worst 51.1 (C = 256, wide, B = 35, scaled, residual)
KAPPA_STEM = 12                      # k_stem_conv; worst 4.64 (C = 512, Gaussian planes)
KAPPA_HEADS = 12                     # k_heads_1x1; worst 3.88 (C = 128, 3 330 rows)
KAPPA_POLICY = 1                     # k_policy_legal; worst 0.36 (live rows)
KAPPA_VALUE = 0.5                    # k_value_head; worst 0.16 (8 191 games)
KAPPA_BF16 = 4                       # k_wino_conv_bf16 against its own arithmetic (wino_bf16_ref_and_scale); worst 1.67 (C = 128, B = 35)

_CHUNK_ELEMS = 1 << 25               # float64 elements of one im2col chunk (256 MB)


def _chunks(batch: int, channels: int):
    step = max(1, _CHUNK_ELEMS // (9 * channels * 90))
    for lo in range(0, batch, step):
        yield lo, min(batch, lo + step)


def _cols(x: torch.Tensor) -> torch.Tensor:
    """[b, C, 10, 9] -> float64 [b, 9 C, 90], rows ordered (c, r, s) like w.view(C_out, 9 C)."""
    return F.unfold(x.double(), 3, padding=1)


def conv3x3_64(x: torch.Tensor, w: torch.Tensor, absolute: bool = False) -> torch.Tensor:
    """float64 F.conv2d(x, w, padding=1) (of |x|, |w| when `absolute`) as an im2col GEMM."""
    b, _, h, wd = x.shape
    wm = w.double().reshape(w.shape[0], -1)
    if absolute:
        wm = wm.abs()
    out = torch.empty(b, w.shape[0], h, wd, dtype=torch.float64, device=x.device)
    for lo, hi in _chunks(b, x.shape[1]):
        xs = x[lo:hi].double()
        out[lo:hi] = torch.matmul(wm, _cols(xs.abs() if absolute else xs)).view(hi - lo, w.shape[0], h, wd)
    return out


def conv3x3_ref_and_scale(x: torch.Tensor, w: torch.Tensor):
    return conv3x3_64(x, w), conv3x3_64(x, w, absolute=True)


def dgrad_filters(w: torch.Tensor) -> torch.Tensor:
    """The data gradient of a 3x3 padding-1 convolution is the convolution of dL/dy with these filters."""
    return w.flip(2, 3).transpose(0, 1)


def wgrad64(x: torch.Tensor, dy: torch.Tensor, absolute: bool = False) -> torch.Tensor:
    """float64 dL/dw of y = conv2d(x, w, padding=1) for dL/dy = dy (of |x|, |dy| when `absolute`): sum over the batch of
    dy[b] [C, 90] @ im2col(x[b])^T [90, 9 C]."""
    b, c = x.shape[:2]
    acc = torch.zeros(dy.shape[1], 9 * c, dtype=torch.float64, device=x.device)
    for lo, hi in _chunks(b, c):
        xs, gs = x[lo:hi].double(), dy[lo:hi].double()
        if absolute:
            xs, gs = xs.abs(), gs.abs()
        cols = _cols(xs).transpose(1, 2).reshape(-1, 9 * c)                        # [(b, pos), 9 C]
        g = gs.reshape(hi - lo, dy.shape[1], -1).permute(1, 0, 2).reshape(dy.shape[1], -1)    # [C_out, (b, pos)]
        acc += g @ cols
    return acc.view(dy.shape[1], c, 3, 3)


def wgrad_ref_and_scale(x: torch.Tensor, dy: torch.Tensor):
    ref = wgrad64(x, dy)
    scale = wgrad64(x, dy, absolute=True).sum(dim=(2, 3), keepdim=True).expand_as(ref)
    return ref, scale


# ---- the evaluator's kernels (inference direction): NHWC operands, float64 references and the scales of their error analysis

def conv_epilogue_ref_and_scale(x, w, bias, residual=None, relu=True):
    """relu?(conv64(x, w) + bias + residual) and conv64(|x|, |w|) + |bias| + |residual| (ReLU is 1-Lipschitz: the bound on the
    pre-activation carries over).  x, residual: logical [B, C_in, 10, 9] / [B, C_out, 10, 9]; w [C_out, C_in, 3, 3] (the stem's
    C_in = 15 included)."""
    ref, scale = conv3x3_ref_and_scale(x, w)
    ref += bias.double().view(1, -1, 1, 1)
    scale += bias.double().abs().view(1, -1, 1, 1)
    if residual is not None:
        ref += residual.double()
        scale += residual.double().abs()
    return (torch.relu(ref) if relu else ref), scale


def heads_ref_and_scale(h, w, bias):
    """relu(h W^T + b) and |h| |W|^T + |b| for rows h [R, C], w [36, C]."""
    wd = w.double()
    ref = torch.empty(h.shape[0], w.shape[0], dtype=torch.float64, device=h.device)
    scale = torch.empty_like(ref)
    step = max(1, _CHUNK_ELEMS // h.shape[1])
    for lo in range(0, h.shape[0], step):
        hs = h[lo:lo + step].double()
        ref[lo:lo + step] = torch.relu(hs @ wd.t() + bias.double())
        scale[lo:lo + step] = hs.abs() @ wd.abs().t() + bias.double().abs()
    return ref, scale


def policy_legal_ref_and_scale(feat, w, bias, moves):
    """feat [G, 2880] . W[a] + bias[a] for every listed move a = moves[g, m] (int64 [G, 128], any count: the caller masks) and
    sum_k |feat_k| |W[a, k]| + |bias[a]|."""
    g = feat.shape[0]
    ref = torch.empty(g, moves.shape[1], dtype=torch.float64, device=feat.device)
    scale = torch.empty_like(ref)
    step = max(1, _CHUNK_ELEMS // (moves.shape[1] * feat.shape[1]))
    for lo in range(0, g, step):
        mv = moves[lo:lo + step]
        wg, f = w[mv].double(), feat[lo:lo + step].double()                        # [n, 128, 2880], [n, 2880]
        ref[lo:lo + step] = torch.einsum("gmk,gk->gm", wg, f) + bias[mv].double()
        scale[lo:lo + step] = torch.einsum("gmk,gk->gm", wg.abs(), f.abs()) + bias[mv].double().abs()
    return ref, scale


TANH_ULPS = 8                        # tanhf's own error, in units of 2^-24 |v| (4 ulps of a float32 in [0.5, 1))


def value_ref_and_scale(vf, w1, b1, w2, b2):
    """tanh(w2 . relu(W1 vf + b1) + b2) for vf [G, 360], w1 [128, 360], and its scale: first layer s_j = sum_k |vf_k| |w1_jk| + |b1_j|,
    then sum_j |w2_j| (|h_j| + s_j) + |b2| (tanh and ReLU are 1-Lipschitz) plus TANH_ULPS |v| for tanhf itself."""
    v64, w1d = vf.double(), w1.double()
    h = torch.relu(v64 @ w1d.t() + b1.double())
    s = v64.abs() @ w1d.abs().t() + b1.double().abs()
    v = torch.tanh(h @ w2.double().view(-1) + b2.double().view(()))
    scale = (h.abs() + s) @ w2.double().abs().view(-1) + b2.double().abs().view(()) + TANH_ULPS * v.abs()
    return v, scale


# ---- the bf16 throughput convolution (k_wino_conv_bf16) in its own arithmetic

def bf16_u_decode(ub: torch.Tensor) -> torch.Tensor:
    """The kernel's bf16 weights [C/128][C/16][20][2][128][8] (xi = 5 p + j, co = 128 cog + col, ci = 16 chunk + 8 h + k) ->
    float64 U[xi, co, ci]."""
    ng, nch = ub.shape[0], ub.shape[1]
    c = 16 * nch
    assert ub.shape == (ng, nch, 20, 2, 128, 8) and ng * 128 == c
    return ub.double().permute(2, 0, 4, 1, 3, 5).reshape(20, c, c)


def _pad_nchw(x_nhwc: torch.Tensor) -> torch.Tensor:
    b, _, c = x_nhwc.shape
    return F.pad(x_nhwc.view(b, 10, 9, c).permute(0, 3, 1, 2), (1, 1, 1, 1))        # [b, C, 12, 11]


def bf16_input_transform_f32(x_nhwc: torch.Tensor) -> torch.Tensor:
    """k_wino_conv_bf16's input transform in float32, operation by operation in its order (the kernel is built without contraction
    and without fast math): [20, b * 15 tiles, C] (xi = 5 p + j).  Rows (p): d0 - d2, d1 + d2, d1 - d2, d1 - d3 -- the third is the
    negative of the textbook row, as in U; columns: the F(3, 3) B^T rows times (2, 2, 6, 6, 1).  Tile t = 3 ty + tx covers output rows
    2 ty, 2 ty + 1 and columns 3 tx .. 3 tx + 2; its 4 x 5 patch starts at padded row 2 ty, padded column 3 tx."""
    xp = _pad_nchw(x_nhwc.float())
    b, c = xp.shape[:2]
    d = [torch.stack([xp[:, :, 2 * ty + r:2 * ty + r + 1, :] for ty in range(5)], 2).squeeze(3) for r in range(4)]   # [b, C, 5, 11]
    rows = [d[0] - d[2], d[1] + d[2], d[1] - d[2], d[1] - d[3]]
    out = []
    for w_row in rows:
        w = [torch.stack([w_row[..., 3 * tx + k] for tx in range(3)], -1) for k in range(5)]      # [b, C, 5 ty, 3 tx]
        t = w[3] - w[1]
        v = [2.0 * (w[0] - w[2]) + t, (2.0 * w[1] - w[3]) + w[2], 3.0 * w[2] - (2.0 * w[1] + w[3]), t, (w[4] - w[2]) - 2.0 * t]
        out += [vj.permute(0, 2, 3, 1).reshape(b * 15, c) for vj in v]
    return torch.stack(out)                                                                        # [20, b * 15, C]


def bf16_input_transform(x_nhwc: torch.Tensor) -> torch.Tensor:
    """The transformed input as the MFMA reads it: bf16_input_transform_f32 rounded to bf16, to nearest even."""
    return bf16_input_transform_f32(x_nhwc).to(torch.bfloat16)


def _bf16_fragile(v32: torch.Tensor) -> torch.Tensor:
    """Entries whose bf16 rounding a one-ulp change of the float32 value would flip."""
    vb = v32.to(torch.bfloat16)
    up = torch.nextafter(v32, torch.full_like(v32, float("inf"))).to(torch.bfloat16)
    dn = torch.nextafter(v32, torch.full_like(v32, float("-inf"))).to(torch.bfloat16)
    return (up != vb) | (dn != vb)


def _bf16_ulp(vb: torch.Tensor) -> torch.Tensor:
    """One unit in the last place of a bf16 value (8 significand bits), float64."""
    e = torch.frexp(vb.double().abs().clamp(min=2.0 ** -126))[1]
    return torch.ldexp(torch.ones_like(vb, dtype=torch.float64), e - 8)


def _wino_output(m: torch.Tensor, b: int) -> torch.Tensor:
    """Output transform of the products m [4 p, 5 j, b * 15, C] (float64) -> [b, C, 10, 9]: columns y0 = m0 + m1 + m2 + m3,
    y1 = m1 - m2 + 2 m3, y2 = m1 + m2 + 4 m3 + m4; rows r0 + r1 + r2 and r1 - r2 - r3."""
    col = torch.stack([m[:, 0] + m[:, 1] + m[:, 2] + m[:, 3], m[:, 1] - m[:, 2] + 2 * m[:, 3],
                       m[:, 1] + m[:, 2] + 4 * m[:, 3] + m[:, 4]], 1)                              # [4, 3, b * 15, C]
    y = torch.stack([col[0] + col[1] + col[2], col[1] - col[2] - col[3]], 0)                       # [2 ya, 3 yb, b * 15, C]
    c = y.shape[-1]
    y = y.view(2, 3, b, 5, 3, c).permute(2, 5, 3, 0, 4, 1)                                          # b, C, ty, ya, tx, yb
    return y.reshape(b, c, 10, 9)


_BF16_CHUNK = 1 << 24                # float64 elements of one transformed-input chunk (20 * tiles * C)


def wino_bf16_ref_and_scale(x_nhwc, ub, bias, residual=None, relu=True):
    """Float64 pipeline of k_wino_conv_bf16's own arithmetic: U = the kernel's bf16 weights, V = its float32 input transform
    rounded to bf16 (bf16_input_transform), products and channel sums and output transform in float64, then bias, residual and
    ReLU.  scale: the same pipeline on |U|, |V| and |A| plus |bias| + |residual| (what float32 accumulation and the float32 output
    transform can get wrong).  allow: the same pipeline on |U| and one bf16 ulp of every V whose rounding one float32 ulp of the
    transform would flip: granted in case the kernel's float32 transform differs from the emulation in the last bit somewhere (the
    tests count the entries that needed it; on an MI355X none has: the emulation is bit for bit).
    x_nhwc, residual [B, 90, C] float32; returns ref, scale, allow as [B, C, 10, 9] float64 and the number of fragile V entries."""
    b, _, c = x_nhwc.shape
    u = bf16_u_decode(ub)                                                 # [20, co, ci]
    ua, a_abs = u.abs(), torch.tensor([[1.0, 1, 1, 1, 0], [0, 1, 1, 2, 0], [0, 1, 1, 4, 1]], dtype=torch.float64)
    ref = torch.empty(b, c, 10, 9, dtype=torch.float64, device=x_nhwc.device)
    scale, allow = torch.empty_like(ref), torch.zeros_like(ref)
    fragile_total = 0
    step = max(1, _BF16_CHUNK // (20 * 15 * c))
    for lo in range(0, b, step):
        hi = min(b, lo + step)
        v32 = bf16_input_transform_f32(x_nhwc[lo:hi])                    # [20, n, ci]
        vb = v32.to(torch.bfloat16)
        v = vb.double()
        m = torch.bmm(v, u.transpose(1, 2)).view(4, 5, -1, c)             # [20, n, co]
        ms = torch.bmm(v.abs(), ua.transpose(1, 2)).view(4, 5, -1, c)
        ref[lo:hi] = _wino_output(m, hi - lo)
        scale[lo:hi] = _wino_output_abs(ms, a_abs, hi - lo)
        fr = _bf16_fragile(v32)
        n_fr = int(fr.sum())
        if n_fr:
            fragile_total += n_fr
            mf = torch.bmm(torch.where(fr, _bf16_ulp(vb), torch.zeros_like(v)), ua.transpose(1, 2)).view(4, 5, -1, c)
            allow[lo:hi] = _wino_output_abs(mf, a_abs, hi - lo)
    ref += bias.double().view(1, -1, 1, 1)
    scale += bias.double().abs().view(1, -1, 1, 1)
    if residual is not None:
        r = residual.double().view(b, 10, 9, c).permute(0, 3, 1, 2)
        ref += r
        scale += r.abs()
    return (torch.relu(ref) if relu else ref), scale, allow, fragile_total


def _wino_output_abs(m: torch.Tensor, a_abs: torch.Tensor, b: int) -> torch.Tensor:
    """|A|^T m |A| for non-negative m [4, 5, n, C]: columns with |A_c| (a_abs [3, 5]), rows with |A_r| = [[1, 1, 1, 0], [0, 1, 1, 1]]."""
    col = torch.einsum("yj,pjnc->pync", a_abs.to(m.device), m)                                     # [4, 3, n, C]
    y = torch.stack([col[0] + col[1] + col[2], col[1] + col[2] + col[3]], 0)
    c = y.shape[-1]
    return y.view(2, 3, b, 5, 3, c).permute(2, 5, 3, 0, 4, 1).reshape(b, c, 10, 9)


def ratio(got: torch.Tensor, ref: torch.Tensor, scale: torch.Tensor, allow: torch.Tensor = None) -> torch.Tensor:
    """|got - ref| / (2^-24 * scale) entrywise; an entry with scale 0 must be exact (inf otherwise).  `allow`: an absolute error
    granted on top of the bound (subtracted from |got - ref| first)."""
    err = (got.double() - ref).abs()
    if allow is not None:
        err = (err - allow).clamp(min=0.0)
    s = U32 * scale.double()
    r = err / torch.where(s > 0, s, torch.ones_like(s))
    return torch.where((s > 0) | (err == 0), r, torch.full_like(r, float("inf")))


def _table(t: torch.Tensor) -> str:
    return "\n".join(" ".join("%8.1f" % v for v in row) for row in t.tolist())


def check_componentwise(got: torch.Tensor, ref: torch.Tensor, scale: torch.Tensor, kappa: float, what: str = "",
                        allow: torch.Tensor = None) -> float:
    """Assert |got - ref| <= kappa * 2^-24 * scale (+ allow) entrywise; returns the worst ratio.  For a weight gradient [C, C, 3, 3]
    the message carries the worst ratio per tap and per 32 x 32 block of channel pairs; for [B, C, ...] tensors, per channel, and for
    [B, C, 10, 9] tensors also the worst ratio per 2 x 3 Winograd output tile."""
    r = ratio(got, ref, scale, allow)
    worst = r.max().item()
    if worst <= kappa:
        return worst
    idx = tuple(int(i) for i in torch.nonzero(r == r.max())[0].tolist())
    msg = ["%s: |err| / (2^-24 scale) = %.4g > kappa %g at %s (got %.9g, ref %.9g, scale %.4g); %d of %d entries over" % (
        what, worst, kappa, idx, got[idx].item(), ref[idx].item(), scale[idx].item(), int((r > kappa).sum()), r.numel())]
    if r.dim() == 4 and r.shape[2:] == (3, 3) and r.shape[0] % 32 == 0 and r.shape[1] % 32 == 0:
        msg.append("worst ratio per tap (r, s):\n" + _table(r.amax(dim=(0, 1))))
        co, ci = r.shape[0] // 32, r.shape[1] // 32
        msg.append("worst ratio per 32x32 block (co block x ci block):\n" + _table(r.amax(dim=(2, 3)).view(co, 32, ci, 32).amax(dim=(1, 3))))
    elif r.dim() >= 2:
        per_c = r.transpose(0, 1).reshape(r.shape[1], -1).amax(dim=1)
        bad = torch.nonzero(per_c > kappa).flatten().tolist()
        msg.append("channels over: %s" % ", ".join("%d (%.3g)" % (c, per_c[c].item()) for c in bad[:16]))
        if r.dim() == 4 and r.shape[2:] == (10, 9):
            per_t = r.reshape(r.shape[0], r.shape[1], 5, 2, 3, 3).amax(dim=(1, 3, 5)).reshape(-1)       # board * 15 + 3 ty + tx
            bad = torch.nonzero(per_t > kappa).flatten().tolist()
            msg.append("tiles over (board, ty, tx): %s" % ", ".join("(%d, %d, %d) %.3g" % (t // 15, t % 15 // 3, t % 3, per_t[t].item())
                                                                     for t in bad[:16]))
    raise AssertionError("\n".join(msg))


# ---- the split-K rule of xq_wino_wgrad (csrc/xq_train.hip: wgrad_blocks, wgrad_splits), mirrored to know which cases have empty splits

def wgrad_blocks(channels: int) -> int:
    return (channels // 128) * (channels // 32) if channels % 128 == 0 else (channels // 64) ** 2


def wgrad_splits(batch: int, channels: int) -> int:
    nblk, pairs = wgrad_blocks(channels), (batch * 15 + 1) // 2
    n = min(max(256 // nblk, 1), pairs)
    while (n * nblk) % 8:
        n += 1
    return n


def wgrad_empty_splits(batch: int, channels: int) -> int:
    """Splits whose tile range is empty: split s covers tile pairs [s * pps, (s + 1) * pps)."""
    n, pairs = wgrad_splits(batch, channels), (batch * 15 + 1) // 2
    pps = -(-pairs // n)
    return n - -(-pairs // pps)
