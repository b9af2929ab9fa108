"""The wide Winograd convolution's epilogue (k_wino_conv<4, HAS_RES>: exchange rounds through LDS planes, output vectors stored a
round late, LDS reads shared between pixel rows and fetched a column ahead, residual as a template argument) at the smallest
shapes at which it can go wrong.

C = 128, 256: one and two channel groups.  B = 1, 2, 3, 17: 15, 30, 45 and 255 tiles -- a lone partial tile group, a group that
straddles boards, a partial last group.  Every (residual, ReLU, reverse) setting.  Each case checks

  * wide == narrow bit for bit (the narrow variant's epilogue stores each vector as it is finished, in one code path);
  * every entry within tests/numerics.py's per-entry bound (KAPPA_EVAL_CONV) of the float64 convolution of the same operands,
    on Gaussian and on post-ReLU activations -- the guard that stays if a later change touches both variants;
  * with zero activations the output is bias + residual EXACTLY, for a residual that is a different integer at every (board,
    pixel, channel quad): a vector stored from the wrong round, plane set or pending register cannot pass;
  * with `n_live`: boards at or beyond it keep the NaN they were prefilled with, boards below it hold none.
"""
import itertools

import pytest
import torch

import numerics as N

pytestmark = pytest.mark.gpu

SWITCHES = list(itertools.product((False, True), repeat=3))             # residual, relu, reverse


def _nchw(t):
    b, _, c = t.shape
    return t.view(b, 10, 9, c).permute(0, 3, 1, 2)


def _pattern(b, c):
    """[B, 90, C] in [-1, 1), constant over a channel quad, different for every (pixel, quad) of a board and shifted per board."""
    quad = (torch.arange(c, device="cuda") // 4).view(1, 1, c)
    pos = torch.arange(90, device="cuda").view(1, 90, 1)
    brd = torch.arange(b, device="cuda").view(b, 1, 1)
    idx = (quad * 90 + pos + 37 * brd) % (90 * c // 4)
    return idx.float() / (45 * c // 4) - 1.0


def _operands(family, b, c, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, device="cuda")
    x = rn(b, 90, c)
    if family == "relu":
        x = torch.relu(x + 0.3)
    w = rn(c, c, 3, 3) * (2.0 / (9 * c)) ** 0.5
    bias = rn(c) * 0.1
    res = rn(b, 90, c) * 0.5 + _pattern(b, c)      # differs per channel quad and per pixel by construction, not by chance
    return x.contiguous(), w.contiguous(), bias.contiguous(), res.contiguous()


def _expected(ref0, scale0, bias, res, relu):
    """The float64 reference and its scale for one switch setting, from the shared conv64 pair (left unchanged)."""
    ref = ref0 + bias.double().view(1, -1, 1, 1)
    scale = scale0 + bias.double().abs().view(1, -1, 1, 1)
    if res is not None:
        ref = ref + _nchw(res).double()
        scale = scale + _nchw(res).double().abs()
    return (torch.relu(ref) if relu else ref), scale


@pytest.mark.parametrize("batch", [1, 2, 3, 17])
@pytest.mark.parametrize("channels", [128, 256])
def test_wide_epilogue_equals_narrow_and_float64(channels, batch):
    from xiangqi_alphazero_amd import hip
    for k, family in enumerate(("gauss", "relu")):
        x, w, bias, res = _operands(family, batch, channels, 1000 * channels + 10 * batch + k)
        u_wide, u_narrow = hip.wino_transform_weights(w, 128), hip.wino_transform_weights(w, 64)
        ref0, scale0 = N.conv3x3_ref_and_scale(_nchw(x), w)
        for with_res, relu, reverse in SWITCHES:
            r = res if with_res else None
            case = "C=%d B=%d %s res=%d relu=%d rev=%d" % (channels, batch, family, with_res, relu, reverse)
            wide = hip.wino_conv3x3(x, u_wide, bias, torch.full_like(x, float("nan")), r, relu, reverse)
            narrow = hip.wino_conv3x3(x, u_narrow, bias, torch.full_like(x, float("nan")), r, relu, reverse)
            assert torch.equal(wide, narrow), case
            ref, scale = _expected(ref0, scale0, bias, r, relu)
            worst = N.check_componentwise(_nchw(wide), ref, scale, N.KAPPA_EVAL_CONV, "wide epilogue " + case)
            print("RATIO %-52s %8.2f" % (case, worst))


@pytest.mark.parametrize("batch", [1, 2, 3, 17])
@pytest.mark.parametrize("channels", [128, 256])
def test_every_vector_lands_where_it_belongs(channels, batch):
    """Zero activations: every accumulator is +0.0, so the output is bias + residual rounded once -- torch's own float32 sum.  The
    residual is an integer code of (board, pixel, channel quad) and the bias a different fraction per channel."""
    from xiangqi_alphazero_amd import hip
    gen = torch.Generator(device="cuda").manual_seed(channels + batch)
    x = torch.zeros(batch, 90, channels, device="cuda")
    w = torch.randn(channels, channels, 3, 3, generator=gen, device="cuda")
    u = hip.wino_transform_weights(w, 128)
    bias = (torch.arange(channels, device="cuda").float() + 1.0) / 1024.0
    quad = (torch.arange(channels, device="cuda") // 4).view(1, 1, -1)
    code = (torch.arange(batch, device="cuda").view(-1, 1, 1) * 90 + torch.arange(90, device="cuda").view(1, 90, 1)) * 64 + quad
    res = (code.float() - 1000.0).contiguous()                            # exact integers, both signs (ReLU clips some)
    for with_res, relu, reverse in SWITCHES:
        want = bias.view(1, 1, -1) + res if with_res else bias.view(1, 1, -1).expand(batch, 90, channels)
        want = torch.relu(want) if relu else want
        got = hip.wino_conv3x3(x, u, bias, torch.full_like(x, float("nan")), res if with_res else None, relu, reverse)
        assert torch.equal(got, want.contiguous()), "C=%d B=%d res=%d relu=%d rev=%d" % (channels, batch, with_res, relu, reverse)


@pytest.mark.parametrize("n_live", [None, 0, 5])
@pytest.mark.parametrize("channels", [128, 256])
def test_live_rows_only(channels, n_live):
    """B = 17 as the capacity: boards [0, n_live) are computed -- bit for bit what the narrow variant computes, within the float64
    bound, no NaN left -- and boards at or beyond n_live keep their NaN prefill.  The dead input boards are NaN too."""
    from xiangqi_alphazero_amd import hip
    cap = 17
    n = cap if n_live is None else n_live
    x, w, bias, res = _operands("relu", cap, channels, 77 * channels + 3 * n)
    u_wide, u_narrow = hip.wino_transform_weights(w, 128), hip.wino_transform_weights(w, 64)
    ref0, scale0 = N.conv3x3_ref_and_scale(_nchw(x), w)
    xp = x.clone()
    xp[n:] = float("nan")
    live = None if n_live is None else torch.tensor([n_live], dtype=torch.int32, device="cuda")
    for with_res, relu, reverse in SWITCHES:
        r = res if with_res else None
        case = "C=%d n_live=%s res=%d relu=%d rev=%d" % (channels, n_live, with_res, relu, reverse)
        wide = hip.wino_conv3x3(xp, u_wide, bias, torch.full_like(x, float("nan")), r, relu, reverse, n_live=live)
        narrow = hip.wino_conv3x3(xp, u_narrow, bias, torch.full_like(x, float("nan")), r, relu, reverse, n_live=live)
        assert torch.isnan(wide[n:]).all(), case + ": a board at or beyond n_live was written"
        assert not torch.isnan(wide[:n]).any(), case + ": a live board kept its NaN"
        assert torch.equal(wide[:n], narrow[:n]), case
        if n:
            ref, scale = _expected(ref0[:n], scale0[:n], bias, None if r is None else r[:n], relu)
            N.check_componentwise(_nchw(wide[:n]), ref, scale, N.KAPPA_EVAL_CONV, "live " + case)
