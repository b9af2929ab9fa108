"""CPU tests of the float64 references and the componentwise comparator of tests/numerics.py, and of the host-side argument checks
and split-K rule of the train-step entry points (xq_wino_wgrad, xq_bn_train_forward), which refuse a call before any HIP call."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import numerics as N

XQ_ERR_ARG = -1


def _scaled(shape, scales, gen):
    """Gaussian [B, C, 10, 9] with channel c multiplied by scales[c]."""
    return torch.randn(*shape, generator=gen, dtype=torch.float64) * scales.view(1, -1, 1, 1)


def _small_pair_case(c=64, b=3, small=1e-2, seed=0):
    """x, dy with unit-scale channels except x channel 5 and dy channel 7, which are `small`: the pair (7, 5) has a scale 1e-4 of
    the largest."""
    gen = torch.Generator().manual_seed(seed)
    sx, sy = torch.ones(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64)
    sx[5], sy[7] = small, small
    x, dy = _scaled((b, c, 10, 9), sx, gen), _scaled((b, c, 10, 9), sy, gen)
    return x, dy


def test_references_equal_torch_float64():
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(3, 64, 10, 9, generator=gen, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(64, 64, 3, 3, generator=gen, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(3, 64, 10, 9, generator=gen, dtype=torch.float64)
    y = F.conv2d(x, w, None, padding=1)
    y.backward(dy)
    assert torch.allclose(N.conv3x3_64(x.detach(), w.detach()), y, rtol=1e-12, atol=1e-12)
    assert torch.allclose(N.conv3x3_64(dy, N.dgrad_filters(w.detach())), x.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(N.wgrad64(x.detach(), dy), w.grad, rtol=1e-12, atol=1e-12)
    assert torch.equal(N.conv3x3_64(x.detach(), w.detach(), absolute=True), N.conv3x3_64(x.detach().abs(), w.detach().abs()))
    ref, scale = N.wgrad_ref_and_scale(x.detach(), dy)
    assert torch.allclose(scale[:, :, 0, 0], N.wgrad64(x.detach().abs(), dy.abs()).sum(dim=(2, 3)), rtol=1e-12)
    assert (ref.abs() <= scale).all()
    old = N._CHUNK_ELEMS                              # chunked over the batch: the same sums
    try:
        N._CHUNK_ELEMS = 9 * 64 * 90
        assert torch.allclose(N.wgrad64(x.detach(), dy), w.grad, rtol=1e-12, atol=1e-12)
        assert torch.allclose(N.conv3x3_64(x.detach(), w.detach()), y, rtol=1e-12, atol=1e-12)
    finally:
        N._CHUNK_ELEMS = old


def test_comparator_passes_float32_rounding_of_the_reference():
    x, dy = _small_pair_case()
    ref, scale = N.wgrad_ref_and_scale(x, dy)
    assert N.check_componentwise(ref.float(), ref, scale, 1.0, "wgrad") <= 1.0
    w = torch.randn(64, 64, 3, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    yref, yscale = N.conv3x3_ref_and_scale(x, w)
    assert N.check_componentwise(yref.float(), yref, yscale, 1.0, "conv") <= 1.0


def test_comparator_flags_a_missing_tile_in_a_small_scale_pair():
    """The weight gradient of channel pair (7, 5) -- scale 1e-4 of the largest -- without one 2 x 3 output tile's contribution."""
    x, dy = _small_pair_case()
    ref, scale = N.wgrad_ref_and_scale(x, dy)
    assert scale[7, 5, 0, 0] <= 1.01e-4 * scale.max()
    dy_cut = dy.clone()
    dy_cut[2, :, 8:10, 6:9] = 0.0                     # the last tile of the last board
    got = ref.clone()
    got[7, 5] = N.wgrad64(x, dy_cut)[7, 5]
    assert (got - ref).abs().max() <= 1e-5 * ref.abs().max()        # the tensor-wide bound does not see it
    with pytest.raises(AssertionError, match=r"per tap[\s\S]*per 32x32 block"):
        N.check_componentwise(got.float(), ref, scale, N.KAPPA_WGRAD, "wgrad")


def test_comparator_flags_a_single_wrong_tap():
    """Tap (0, 2) of the small-scale pair computed with the board wrapped around instead of zero-padded (a masking error at the
    edge column)."""
    x, dy = _small_pair_case()
    ref, scale = N.wgrad_ref_and_scale(x, dy)
    wrapped = F.pad(x, (1, 1, 1, 1))
    wrapped[..., :, -1] = wrapped[..., :, 1]          # the padding column right of the board holds the left column
    tap = (dy[:, 7:8] * wrapped[:, 5:6, 0:10, 2:11]).sum()
    got = ref.clone()
    got[7, 5, 0, 2] = tap
    assert (tap - ref[7, 5, 0, 2]).abs() > 0
    with pytest.raises(AssertionError, match=r"at \(7, 5, 0, 2\)"):
        N.check_componentwise(got.float(), ref, scale, N.KAPPA_WGRAD, "wgrad")


def test_comparator_flags_a_scaled_block_and_a_wrong_conv_channel():
    """A 1e-3 relative error in one 32 x 32 block holding the small pair, and in one small-scale output channel of a convolution."""
    x, dy = _small_pair_case(b=35)
    xp, dyp = x.abs(), dy.abs()                       # non-negative operands: ref = scale, so the bound is relative
    ref, scale = N.wgrad_ref_and_scale(xp, dyp)
    got = ref.clone()
    got[0:32, 0:32] *= 1.0 + 1e-3
    with pytest.raises(AssertionError):
        N.check_componentwise(got.float(), ref, scale, N.KAPPA_WGRAD, "wgrad")
    w = torch.randn(64, 64, 3, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    w[7] *= 1e-4
    yref, yscale = N.conv3x3_ref_and_scale(x, w)
    got = yref.clone()
    got[:, 7] *= 1.0 + 1e-3
    with pytest.raises(AssertionError, match="channels over: 7 "):
        N.check_componentwise(got.float(), yref, yscale, N.KAPPA_CONV, "conv")


# ---- host-side checks of the entry points (the calls below are all refused before any HIP call)

def _lib():
    from xiangqi_alphazero_amd import hip
    hip.build()
    return hip.lib()


FAKE = 0x7F0000000000                                 # 16-byte aligned, never dereferenced: every call below is refused


def test_wgrad_entry_point_refuses_bad_arguments():
    L = _lib()
    p = [FAKE, FAKE + 0x1000000, FAKE + 0x2000000, FAKE + 0x3000000]
    for c in (96, 1024, 0, 32, 320):
        assert L.xq_wino_wgrad(*p, 4, c, None) == XQ_ERR_ARG, c
    for b in (0, -1, -(1 << 31)):
        assert L.xq_wino_wgrad(*p, b, 64, None) == XQ_ERR_ARG, b
    for i in range(4):                                # one operand off 16-byte alignment
        q = list(p)
        q[i] += 4
        assert L.xq_wino_wgrad(*q, 4, 256, None) == XQ_ERR_ARG, i
        q[i] = p[i] + 8
        assert L.xq_wino_wgrad(*q, 4, 256, None) == XQ_ERR_ARG, i
    for c in (64, 128, 256, 512):                     # first batch whose buffer offsets overflow the 32-bit limit
        b = next(b for b in range(1, 1 << 20) if (b * 90 + 64) * c * 4 >= 0xFFF00000)
        assert b * 90 * c * 4 < 1 << 32
        assert L.xq_wino_wgrad(*p, b, c, None) == XQ_ERR_ARG, c
        assert L.xq_wino_wgrad(*p, 1 << 20, c, None) == XQ_ERR_ARG, c


def test_bn_forward_entry_point_refuses_bad_arguments():
    L = _lib()
    x, r, g, bt, rm, rv, y, sm, si, nbt, scr = [FAKE + i * 0x1000000 for i in range(11)]

    def call(rows=900, c=64, rm=rm, rv=rv):
        return L.xq_bn_train_forward(x, r, g, bt, rm, rv, ctypes.c_float(0.1), ctypes.c_float(1e-5), rows, c, 1, y, sm, si, nbt,
                                     scr, None)
    assert call(rows=0) == XQ_ERR_ARG
    assert call(rows=-90) == XQ_ERR_ARG
    assert call(c=96) == XQ_ERR_ARG
    assert call(c=2048) == XQ_ERR_ARG
    assert call(rm=None) == XQ_ERR_ARG
    assert call(rv=None) == XQ_ERR_ARG
    assert L.xq_bn_train_forward(x + 4, r, g, bt, rm, rv, ctypes.c_float(0.1), ctypes.c_float(1e-5), 900, 64, 1, y, sm, si, nbt, scr,
                                 None) == XQ_ERR_ARG


def test_wgrad_split_count_for_every_batch():
    """xq_wino_wgrad_scratch_bytes = n_split * 9 * C^2 * 4 with the split rule mirrored in tests/numerics.py: for every batch 1..4096
    at least one split and a multiple of 8 workgroups; the edge cases of tests/test_train_kernels.py really have empty splits."""
    L = _lib()
    for c in (64, 128, 256, 512):
        blocks = N.wgrad_blocks(c)
        for b in range(1, 4097):
            nbytes = L.xq_wino_wgrad_scratch_bytes(b, c)
            assert nbytes % (9 * c * c * 4) == 0, (b, c)
            n = nbytes // (9 * c * c * 4)
            assert n >= 1 and (n * blocks) % 8 == 0, (b, c, n)
            assert n == N.wgrad_splits(b, c), (b, c)
    assert L.xq_wino_wgrad_scratch_bytes(0, 64) == 0 and L.xq_wino_wgrad_scratch_bytes(4, 96) == 0
    assert N.wgrad_empty_splits(3, 64) == 1 and N.wgrad_empty_splits(3, 128) >= 1
    assert N.wgrad_splits(35, 64) == 256 and N.wgrad_empty_splits(35, 64) == 124          # 263 pairs, 2 per split


# ---- the evaluator's references (tests/test_eval_kernels.py)

def _nhwc_to_nchw(t):
    b, _, c = t.shape
    return t.view(b, 10, 9, c).permute(0, 3, 1, 2)


def test_evaluator_references_equal_torch_float64():
    gen = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    x, w, bias, res = rn(3, 64, 10, 9), rn(64, 64, 3, 3), rn(64), rn(3, 64, 10, 9)
    for residual in (None, res):
        for relu in (False, True):
            want = F.conv2d(x, w, bias, padding=1) + (0 if residual is None else residual)
            want = torch.relu(want) if relu else want
            ref, scale = N.conv_epilogue_ref_and_scale(x, w, bias, residual, relu)
            assert torch.allclose(ref, want, rtol=1e-12, atol=1e-12)
            sc = F.conv2d(x.abs(), w.abs(), bias.abs(), padding=1) + (0 if residual is None else residual.abs())
            assert torch.allclose(scale, sc, rtol=1e-12, atol=1e-12)
    planes, ws = (torch.rand(2, 15, 10, 9, generator=gen) < 0.1).double(), rn(128, 15, 3, 3)       # the stem: 15 input planes
    ref, _ = N.conv_epilogue_ref_and_scale(planes, ws, bias[:1].expand(128), None, True)
    assert torch.allclose(ref, torch.relu(F.conv2d(planes, ws, bias[:1].expand(128), padding=1)), rtol=1e-12, atol=1e-12)

    h, wh, bh = rn(37, 128), rn(36, 128), rn(36)
    ref, scale = N.heads_ref_and_scale(h, wh, bh)
    assert torch.allclose(ref, torch.relu(h @ wh.t() + bh), rtol=1e-12, atol=1e-12)
    assert torch.allclose(scale, h.abs() @ wh.abs().t() + bh.abs(), rtol=1e-12)

    feat, wp, bp = rn(5, 2880), rn(8100, 2880) * 0.01, rn(8100)
    moves = torch.stack([torch.randperm(8100, generator=gen)[:128] for _ in range(5)])
    moves[0, 0], moves[1, 127] = 0, 8099
    ref, scale = N.policy_legal_ref_and_scale(feat, wp, bp, moves)
    dense = feat @ wp.t() + bp
    assert torch.allclose(ref, torch.gather(dense, 1, moves), rtol=1e-12, atol=1e-12)
    assert torch.allclose(scale, torch.gather(feat.abs() @ wp.abs().t() + bp.abs(), 1, moves), rtol=1e-12)

    vf, w1, b1, w2, b2 = rn(7, 360).relu(), rn(128, 360) * 0.05, rn(128) * 0.1, rn(128) * 0.1, rn(1) * 0.1
    v, scale = N.value_ref_and_scale(vf, w1, b1, w2, b2)
    hid = torch.relu(vf @ w1.t() + b1)
    assert torch.allclose(v, torch.tanh(hid @ w2 + b2), rtol=1e-12, atol=1e-12)
    s = vf.abs() @ w1.abs().t() + b1.abs()
    assert torch.allclose(scale, (hid + s) @ w2.abs() + b2.abs() + N.TANH_ULPS * v.abs(), rtol=1e-12)


@pytest.mark.parametrize("channels", [128, 256])
def test_bf16_reference_equals_the_direct_convolution_on_exact_operands(channels):
    """Filters 6 k and inputs in {-2 .. 2}: every U (G g G^T has the factors 1/2 and 1/6) and every V is a small binary fraction,
    exact in bf16, so the bf16 pipeline must equal the float64 direct convolution -- which pins the decoding of the kernel's weight
    layout (two channel groups at C = 256), the sign of the third Winograd row, the tile order and the output transform."""
    from xiangqi_alphazero_amd import hip
    gen = torch.Generator().manual_seed(channels)
    b = 3
    x = torch.randint(-2, 3, (b, 90, channels), generator=gen).float()
    w = 6.0 * torch.randint(-1, 2, (channels, channels, 3, 3), generator=gen).float()
    bias = torch.randint(-4, 5, (channels,), generator=gen).float() / 4
    res = torch.randint(-8, 9, (b, 90, channels), generator=gen).float()
    ub = hip.wino_transform_weights_bf16(w)
    u = N.bf16_u_decode(ub)
    assert torch.equal(u.float().to(torch.bfloat16).double(), u)
    assert torch.equal(N.bf16_input_transform(x).double(), N.bf16_input_transform_f32(x).double())     # V exact too
    xn = _nhwc_to_nchw(x)
    for residual, relu in ((None, False), (res, True)):
        ref, scale, allow, fragile = N.wino_bf16_ref_and_scale(x, ub, bias, residual, relu)
        want = F.conv2d(xn.double(), w.double(), bias.double(), padding=1)
        if residual is not None:
            want = want + _nhwc_to_nchw(residual).double()
        want = torch.relu(want) if relu else want
        assert torch.equal(ref, want)
        assert fragile == 0 and not allow.any()
        assert (ref.abs() <= scale).all()


def test_bf16_reference_flags_truncation_and_passes_float32_rounding():
    """Gaussian operands: the float32 rounding of the bf16 pipeline passes at kappa 1; the same pipeline with V truncated to bf16
    (toward zero) instead of rounded to nearest even -- a conversion-mode fault -- does not pass KAPPA_BF16."""
    from xiangqi_alphazero_amd import hip
    gen = torch.Generator().manual_seed(5)
    c, b = 128, 4
    x = torch.randn(b, 90, c, generator=gen)
    w = torch.randn(c, c, 3, 3, generator=gen) * (2.0 / (9 * c)) ** 0.5
    bias = torch.randn(c, generator=gen) * 0.1
    ub = hip.wino_transform_weights_bf16(w)
    ref, scale, allow, fragile = N.wino_bf16_ref_and_scale(x, ub, bias, None, False)
    print("fragile V entries: %d of %d" % (fragile, 20 * 15 * b * c))
    assert N.check_componentwise(ref.float(), ref, scale, 1.0, "bf16 f32 rounding", allow) <= 1.0
    v32 = N.bf16_input_transform_f32(x)
    vt = (v32.view(torch.int32) & ~0xFFFF).view(torch.float32).double()                            # truncated to bf16
    m = torch.bmm(vt, N.bf16_u_decode(ub).transpose(1, 2)).view(4, 5, -1, c)
    got = N._wino_output(m, b) + bias.double().view(1, -1, 1, 1)
    with pytest.raises(AssertionError, match="tiles over"):
        N.check_componentwise(got.float(), ref, scale, N.KAPPA_BF16, "bf16 truncated", allow)


def test_comparator_flags_a_wrong_output_tile_and_a_small_channel():
    """One 2 x 3 output tile of one board computed from its neighbour's patch, and a channel at 1e-3 of the largest scale off by
    1e-3 relative: both within 4e-5 absolute of the reference, both flagged per entry, located by board, tile and channel."""
    gen = torch.Generator().manual_seed(8)
    b, c = 35, 64
    x = torch.relu(torch.randn(b, c, 10, 9, generator=gen, dtype=torch.float64) + 0.3)
    w = torch.randn(c, c, 3, 3, generator=gen, dtype=torch.float64) * (2.0 / (9 * c)) ** 0.5
    w[5] *= 1e-3
    bias = torch.randn(c, generator=gen, dtype=torch.float64) * 0.1
    bias[5] *= 1e-3
    ref, scale = N.conv_epilogue_ref_and_scale(x, w, bias, None, False)
    assert N.check_componentwise(ref.float(), ref, scale, 1.0, "conv") <= 1.0
    got = ref.clone()
    got[34, :, 8:10, 3:6] = ref[34, :, 8:10, 0:3]                                               # tile (4, 1) of the last board
    with pytest.raises(AssertionError, match=r"tiles over \(board, ty, tx\): \(34, 4, 1\)"):
        N.check_componentwise(got.float(), ref, scale, N.KAPPA_EVAL_CONV, "conv tile")
    got = ref.clone()
    got[:, 5] *= 1.0 + 1e-3
    assert (got - ref).abs().max() < 4e-5
    with pytest.raises(AssertionError, match="channels over: 5 "):
        N.check_componentwise(got.float(), ref, scale, N.KAPPA_EVAL_CONV, "conv channel")
