"""Float64 references of the train-step kernels and a componentwise comparator.

A bound relative to the largest entry of a tensor does not check the small entries at all: a channel whose activations are 1e-4 of
the largest one can be wrong by 100 % and pass.  The comparator here bounds every entry by the scale a rounding-error analysis gives
it instead:

  * convolution (forward, data gradient):  scale = conv64(|x|, |w|), the float64 convolution of absolute values;
  * weight gradient:  scale[co, ci] = sum over the 9 taps of wgrad64(|x|, |dy|)[co, ci], broadcast over the taps (the Winograd
    transforms mix the taps of one channel pair);
  * assertion:  |got - ref64| <= kappa * 2^-24 * scale, entry by entry.

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


def ratio(got: torch.Tensor, ref: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """|got - ref| / (2^-24 * scale) entrywise; an entry with scale 0 must be exact (inf otherwise)."""
    err = (got.double() - ref).abs()
    s = U32 * scale.double()
    r = err / torch.where(s > 0, s, torch.ones_like(s))
    return torch.where((s > 0) | (err == 0), r, torch.full_like(r, float("inf")))


def _table(t: torch.Tensor) -> str:
    return "\n".join(" ".join("%8.1f" % v for v in row) for row in t.tolist())


def check_componentwise(got: torch.Tensor, ref: torch.Tensor, scale: torch.Tensor, kappa: float, what: str = "") -> float:
    """Assert |got - ref| <= kappa * 2^-24 * scale entrywise; returns the worst ratio.  For a weight gradient [C, C, 3, 3] the
    message carries the worst ratio per tap and per 32 x 32 block of channel pairs; for [B, C, ...] tensors, per channel."""
    r = ratio(got, ref, scale)
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
