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
