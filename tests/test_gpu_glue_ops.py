"""GPU: the small NHWC operators of csrc/kernels_misc.hip alone, through their developer entries - maxpool2x2s1_kernel (zero padding: a
border takes max(.., 0)), avgpool3x2_kernel with its compact line-table form, mask_cols_kernel, upsample_kernel with and without
accumulate, add_kernel - and det_head_tail_kernel<24,24> with the engine's own weight repack (rd_debug_det_head_tail).

Where the operation is exact in fp32 (max-pool, mask, upsample copy, upsample accumulate and add = one fp32 addition) the result must be
bit-equal to torch fp32.  The average pool is bounded by 7 * 2^-24 * sum|x| / 6 against fp64; the head tail by the yardstick rule of
tests/test_gpu_attention.py (4 x the error of torch fp32 + 4 * 2^-24 * max|reference|).  Every map is a strided view inside a
sentinel-filled buffer.  Cases and measured ratios: docs/notebook/glue_kernels.md."""
import pytest
import torch

from glue_helpers import SENTINEL, View, check_linear, check_yardstick, lib

pytestmark = pytest.mark.gpu
F = torch.nn.functional


def bit_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------------------------------------ max-pool
@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (5, 1), (5, 7)])
@pytest.mark.parametrize("c,xs,ys", [(4, (4, 0), (4, 0)), (96, (128, 32), (112, 8))], ids=["C4", "C96-slots"])
def test_maxpool_zero_padding_decides_the_border(h, w, c, xs, ys):
    n = 2
    g = torch.Generator().manual_seed(h * 10 + w)
    x = -(torch.rand((n, h, w, c), generator=g) + 0.1)               # all negative: only the zero padding can give 0
    xv, yv = View(n * h * w, c, *xs, data=x), View(n * h * w, c, *ys)
    assert lib().rd_debug_maxpool2x2s1(n, h, w, c, xs[0], ys[0], xv.ptr, yv.ptr) == 0
    y = yv.owned().view(n, h, w, c)
    ref = nhwc(F.max_pool2d(F.pad(nchw(x), (0, 1, 0, 1)), 2, stride=1))
    assert bit_equal(y, ref), float((y - ref).abs().max())
    assert bool((y[:, -1] == 0).all()) and bool((y[:, :, -1] == 0).all()), "the last row and the last column take the padding's zero"
    assert bool((y[:, :-1, :-1] < 0).all()), "the interior stays negative"
    yv.assert_outside_untouched("maxpool")
    xv.assert_unchanged("maxpool")


# ------------------------------------------------------------------------------------------------------------------------------ avg-pool
@pytest.mark.parametrize("h", [3, 4, 5, 7])
@pytest.mark.parametrize("w,c,xs,ys", [(9, 24, (24, 0), (24, 0)), (16, 96, (128, 16), (104, 8))], ids=["W9", "W16-slots"])
def test_avgpool3x2_matches_fp64(h, w, c, xs, ys):
    n = 2
    oh, ow = h // 3, w // 2
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn((n, h, w, c), generator=g)
    xv, yv = View(n * h * w, c, *xs, data=x), View(n * oh * ow, c, *ys)
    assert lib().rd_debug_avgpool3x2(n, h, w, c, xs[0], ys[0], xv.ptr, yv.ptr, None) == 0
    ref = nhwc(F.avg_pool2d(nchw(x.double()), (3, 2), stride=(3, 2)))
    mag = nhwc(F.avg_pool2d(nchw(x.double().abs()), (3, 2), stride=(3, 2)))          # = sum|x| / 6
    assert ref.shape == (n, oh, ow, c)
    check_linear(yv.owned().view(n, oh, ow, c), ref, mag, 7, "avgpool %dx%dx%d" % (h, w, c))
    yv.assert_outside_untouched("avgpool")
    xv.assert_unchanged("avgpool")


def test_avgpool3x2_compact_line_table():
    """OH = 1; line n writes its w4 / 2 tokens at row line_tab[n][3] of the token buffer: three lines of different widths at non-contiguous
    offsets, the rows between them keep the sentinel"""
    n, h, w, c = 3, 3, 16, 96
    w4, off, rows = [16, 7, 2], [10, 2, 20], 24
    g = torch.Generator().manual_seed(5)
    x = torch.randn((n, h, w, c), generator=g)
    xv, yv = View(n * h * w, c, data=x), View(rows, c, 128, 32, data=torch.full((rows, c), SENTINEL))      # (no NaN here: unowned rows are compared)
    tab = torch.tensor([[4 * v, 2 * v, v, o] for v, o in zip(w4, off)], dtype=torch.int32, device="cuda")
    assert tab.shape[1] == 4                                                       # kLineTabStride
    assert lib().rd_debug_avgpool3x2(n, h, w, c, c, 128, xv.ptr, yv.ptr, tab.data_ptr()) == 0
    ref = nhwc(F.avg_pool2d(nchw(x.double()), (3, 2), stride=(3, 2)))[:, 0]        # [n][8][c]
    mag = nhwc(F.avg_pool2d(nchw(x.double().abs()), (3, 2), stride=(3, 2)))[:, 0]
    y = yv.owned()
    owned = torch.zeros(rows, dtype=torch.bool)
    for i in range(n):
        t = w4[i] // 2
        owned[off[i]:off[i] + t] = True
        check_linear(y[off[i]:off[i] + t], ref[i, :t], mag[i, :t], 7, "avgpool compact line %d (%d tokens at %d)" % (i, t, off[i]))
    assert int(owned.sum()) == 8 + 3 + 1
    yv.assert_outside_untouched("avgpool compact", owned_rows=owned)
    assert lib().rd_debug_avgpool3x2(n, 7, w, c, c, 128, xv.ptr, yv.ptr, tab.data_ptr()) == -1      # the compact form is one row of tokens


# ------------------------------------------------------------------------------------------------------------------------------ mask
def test_mask_cols_zeroes_beyond_each_width_and_nothing_else():
    n, h, w, c = 3, 2, 7, 24
    widths = [0, 7, 3]
    g = torch.Generator().manual_seed(6)
    y0 = torch.randn((n, h, w, c), generator=g)
    yv = View(n * h * w, c, 40, 12, data=y0)
    # the widths sit at column 2 of a line table, as the engine passes them
    tab = torch.tensor([[0, 0, v, 0] for v in widths], dtype=torch.int32, device="cuda")
    assert lib().rd_debug_mask_cols(n, h, w, c, 40, yv.ptr, tab.data_ptr() + 8, 4) == 0
    want = y0.clone()
    for i, v in enumerate(widths):
        want[i, :, v:] = 0.0
    assert bit_equal(yv.owned().view(n, h, w, c), want)
    yv.assert_outside_untouched("mask_cols")


# ------------------------------------------------------------------------------------------------------------------------------ upsample, add
@pytest.mark.parametrize("acc", [0, 1], ids=["copy", "accumulate"])
@pytest.mark.parametrize("f,h,w", [(1, 3, 5), (2, 6, 10), (4, 4, 12), (8, 16, 24)])
@pytest.mark.parametrize("c,xs,ys", [(4, (4, 0), (4, 0)), (24, (32, 8), (96, 48))], ids=["C4", "C24-slot-of-96"])
def test_upsample_is_bit_exact(f, h, w, c, xs, ys, acc):
    n = 2
    assert f == 8 or (n * h * w * (c // 4)) % 256 != 0                # (f = 8 at C = 24: 18 blocks; the others end inside a block)
    g = torch.Generator().manual_seed(f * 10 + c)
    x = torch.randn((n, h // f, w // f, c), generator=g)
    y0 = torch.randn((n, h, w, c), generator=g) if acc else None
    xv, yv = View(x.numel() // c, c, *xs, data=x), View(n * h * w, c, *ys, data=y0)
    assert lib().rd_debug_upsample(n, h, w, c, f, acc, xs[0], ys[0], xv.ptr, yv.ptr) == 0
    up = x.repeat_interleave(f, dim=1).repeat_interleave(f, dim=2)
    want = up + y0 if acc else up                                     # accumulate = one fp32 addition: exact to the bit
    assert bit_equal(yv.owned().view(n, h, w, c), want)
    yv.assert_outside_untouched("upsample")
    xv.assert_unchanged("upsample")


def test_upsample_declines_a_map_that_is_no_multiple_of_f():
    v = View(64, 4)
    assert lib().rd_debug_upsample(1, 5, 8, 4, 2, 0, 4, 4, v.ptr, v.ptr) == -1
    assert bool(torch.isnan(v.owned()).all())


@pytest.mark.parametrize("m,c", [(37, 24), (1, 4), (700, 96)])
def test_add_is_bit_exact_on_three_leading_dimensions(m, c):
    g = torch.Generator().manual_seed(m)
    a, b = torch.randn((m, c), generator=g), torch.randn((m, c), generator=g)
    av, bv, yv = View(m, c, c + 16, 8, data=a), View(m, c, c + 8, 0, data=b), View(m, c, c + 24, 20)
    assert lib().rd_debug_add(m, c, c + 16, c + 8, c + 24, av.ptr, bv.ptr, yv.ptr) == 0
    assert bit_equal(yv.owned(), a + b)
    yv.assert_outside_untouched("add")
    av.assert_unchanged("add")
    bv.assert_unchanged("add")


# ------------------------------------------------------------------------------------------------------------------------------ DB head tail
TAP1 = torch.tensor([[1.0, 0.3], [-0.6, 1.7]])       # per-tap gains [dy][dx]: a swapped dy / dx or tap order moves the result by O(0.1)
TAP2 = torch.tensor([[0.5, 1.5], [-1.0, 0.2]])


def head_tail_reference(x, w1, b1, w2, b2, dtype):
    """x NHWC [N][H][W][24] -> [N][4H][4W]: ConvTranspose2d(24, 24, 2, 2) -> ReLU -> ConvTranspose2d(24, 1, 2, 2) -> sigmoid in `dtype`"""
    t = F.conv_transpose2d(nchw(x.to(dtype)), w1.to(dtype), b1.to(dtype), stride=2).clamp_min(0)
    return torch.sigmoid(F.conv_transpose2d(t, w2.to(dtype), b2.to(dtype), stride=2))[:, 0]


@pytest.mark.parametrize("n,h,w", [(2, 5, 7), (1, 17, 31)], ids=["2x5x7-one-block-mostly-masked", "1x17x31-tail-block"])
@pytest.mark.parametrize("xld", [24, 40])
def test_det_head_tail_matches_fp64(n, h, w, xld):
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + xld)
    x = torch.randn((n, h, w, 24), generator=g)
    w1 = torch.randn((24, 24, 2, 2), generator=g) / 24 ** 0.5 * TAP1          # checkpoint layouts: [cin][cmid][2][2], [cmid][1][2][2]
    w2 = torch.randn((24, 1, 2, 2), generator=g) / 3.0 * TAP2
    b1, b2 = torch.rand((24,), generator=g) - 0.5, torch.tensor([0.3])
    xv, yv = View(n * h * w, 24, xld, xld - 24, data=x), View(n * 4 * h, 4 * w)
    dev = [t.contiguous().cuda() for t in (w1, b1, w2, b2)]
    assert lib().rd_debug_det_head_tail(n, h, w, xld, xv.ptr, *[t.data_ptr() for t in dev], yv.ptr) == 0
    ref = head_tail_reference(x, w1, b1, w2, b2, torch.float64)
    yard = head_tail_reference(x, w1, b1, w2, b2, torch.float32)
    # what a swapped dy / dx in the kernel or a swapped tap order in the repack would give is far outside the bound
    swapped = head_tail_reference(x, w1.transpose(2, 3), b1, w2.transpose(2, 3), b2, torch.float64)
    assert float((swapped - ref).abs().max()) > 0.05
    check_yardstick(yv.owned().view(n, 4 * h, 4 * w), ref, yard, "det_head_tail %dx%dx%d xld %d" % (n, h, w, xld))
    yv.assert_outside_untouched("det_head_tail")
    xv.assert_unchanged("det_head_tail")
