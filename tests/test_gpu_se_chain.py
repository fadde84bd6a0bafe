"""GPU: the squeeze-excite chain gap_partial_kernel -> se_fc_kernel -> scale_channels_kernel (csrc/kernels_misc.hip) alone against fp64,
through the developer entry rd_debug_se_chain: the channel counts at which se_fc_kernel changes its slice / quad split, hidden-unit counts
that leave a wavefront nothing or a butterfly a tail, both forms of the W2 row, empty pooling chunks, the three gates, the RSE residual
form, strided maps, the width limit, and the pooling extent of a line table fed by the depthwise kernel's own partial sums.

Reference: gate = act(W2 relu(W1 mean + b1) + b2), y = x (gate + alpha) in fp64 on the same fp32 values.  Bound: the rule of
tests/test_gpu_attention.py - the same formula by torch in plain fp32 on the CPU is the yardstick; the kernel's max-abs error may be at
most 4 x the yardstick's plus 4 * 2^-24 * max|reference|.  Cases and measured ratios: docs/notebook/glue_kernels.md."""
import ctypes as C

import pytest
import torch

from glue_helpers import SENTINEL, View, check_linear, check_yardstick, lib

pytestmark = pytest.mark.gpu

SIGMOID, HSIG, HSIG_PADDLE = 4, 5, 6          # rd::Act

# (C, Cr, chunks, H, W, N, gate, alpha, xld, yld, why)
CASES = [
    (8, 2, 1, 1, 1, 1, SIGMOID, 0.0, 8, 8, "fewer hidden units than wavefronts; one pixel, one chunk"),
    (24, 6, 4, 1, 5, 3, HSIG, 1.0, 40, 32, "Cr % 4 != 0: the scalar W2 row, wave 3 owns nothing; the last of 4 chunks is empty"),
    (96, 24, 3, 7, 1, 1, HSIG_PADDLE, 0.0, 96, 96, "the recogniser's width; HW = 7 in 3 chunks"),
    (120, 30, 64, 1, 193, 3, SIGMOID, 1.0, 128, 136, "Cr % 8 != 0 inside a wave: the butterfly has a tail; 64 chunks, 15 of them empty"),
    (256, 64, 3, 7, 1, 3, HSIG, 0.0, 256, 256, "KS = 4"),
    (260, 65, 4, 5, 1, 1, HSIG_PADDLE, 1.0, 264, 272, "c4n = 65, KS = 3, the second 16-byte step of a W1 row, Cr odd"),
    (512, 128, 64, 193, 1, 1, SIGMOID, 0.0, 512, 512, "the limit"),
    (512, 128, 1, 1, 1, 3, HSIG, 1.0, 512, 512, "the limit, one pixel, N = 3"),
    (260, 65, 64, 1, 193, 3, HSIG, 0.0, 260, 260, "KS = 3 over 64 chunks"),
    (24, 6, 1, 1, 1, 1, HSIG_PADDLE, 0.0, 24, 24, "one pixel"),
    (120, 30, 3, 1, 7, 1, HSIG, 1.0, 120, 120, "butterfly tail, 3 chunks"),
    (8, 2, 64, 193, 1, 3, HSIG_PADDLE, 1.0, 16, 12, "KS = 8 over 64 chunks, strided"),
    (96, 24, 4, 5, 1, 3, SIGMOID, 0.0, 96, 96, "empty last chunk, N = 3"),
    (256, 64, 64, 1, 193, 1, HSIG_PADDLE, 1.0, 256, 256, "KS = 4 over 64 chunks"),
]


def gate_of(pre, act):
    if act == SIGMOID:
        return torch.sigmoid(pre)
    return (pre / 6 + 0.5).clamp(0, 1) if act == HSIG else (0.2 * pre + 0.5).clamp(0, 1)


def se_formula(pooled_sum, extent, w1, b1, w2, b2, act, dtype):
    """gate [N][C] from the pooled sums [N][C] and each image's pooling extent [N], evaluated in `dtype`"""
    mean = pooled_sum.to(dtype) / extent.to(dtype)[:, None]
    hid = (mean @ w1.to(dtype).t() + b1.to(dtype)).clamp_min(0)
    pre = hid @ w2.to(dtype).t() + b2.to(dtype)
    return gate_of(pre, act), pre


def draw_weights(c, cr, pooled_mean, g):
    """W1, b1 at unit scale; W2, b2 scaled and shifted so that the gate pre-activations of this input span [-4, 4]: beyond the clamps of
    both hard sigmoids (+-3, +-2.5) on either side"""
    w1 = torch.randn((cr, c), generator=g) / c ** 0.5
    b1 = torch.rand((cr,), generator=g) - 0.3
    w2 = torch.randn((c, cr), generator=g)
    hid = (pooled_mean.double() @ w1.double().t() + b1.double()).clamp_min(0)
    z = hid @ w2.double().t()
    s = 8.0 / float(z.max() - z.min())
    w2 = (w2 * s).float()
    b2 = (-4.0 - s * float(z.min()) + 0.1 * (torch.rand((c,), generator=g) - 0.5)).float()
    return w1, b1, w2, b2


def launch(n, h, w, c, cr, chunks, act, alpha, x_view, y_view, weights, partial, gate, fill, line_w=None):
    dev = [t.cuda() for t in weights]
    rc = lib().rd_debug_se_chain(n, h, w, c, cr, chunks, act, alpha, x_view.ld if x_view else 0, y_view.ld if y_view else 0, fill,
                                 x_view.ptr if x_view else None, *[t.data_ptr() for t in dev], line_w.data_ptr() if line_w is not None else None,
                                 partial.ptr, gate.ptr, y_view.ptr if y_view else None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: "C%d-Cr%d-ch%d-hw%d" % (CASES[i][0], CASES[i][1], CASES[i][2], CASES[i][3] * CASES[i][4]))
def test_se_chain_matches_fp64(i):
    c, cr, chunks, h, w, n, act, alpha, xld, yld, why = CASES[i]
    hw = h * w
    tag = "se C%d Cr%d chunks%d HW%d N%d gate%d alpha%g" % (c, cr, chunks, hw, n, act, alpha)
    g = torch.Generator().manual_seed(500 + i)
    x = torch.randn((n, hw, c), generator=g) + 0.5
    weights = draw_weights(c, cr, x.double().mean(1), g)
    xv = View(n * hw, c, xld, (xld - c) // 2 // 4 * 4, data=x)
    yv = View(n * hw, c, yld, (yld - c) // 4 * 4)
    pv, gv = View(n * chunks, c), View(n, c)
    assert launch(n, h, w, c, cr, chunks, act, alpha, xv, yv, weights, pv, gv, 1) == 0
    extent = torch.full((n,), float(hw))
    ref_gate, pre = se_formula(x.double().sum(1), extent, *weights, act, torch.float64)
    assert float(pre.max()) > 3.2 and float(pre.min()) < -3.2, (tag, "the pre-activations do not span the clamps", float(pre.min()), float(pre.max()))
    yard_gate, _ = se_formula(x.sum(1), extent, *weights, act, torch.float32)
    # the pooling partial sums: chunk k owns pixels [k per, (k + 1) per), an empty chunk writes zeros
    per = -(-hw // chunks)
    part = pv.owned().view(n, chunks, c)
    for k in range(chunks):
        if k * per >= hw:
            assert bool((part[:, k] == 0).all()), (tag, "empty chunk", k)
    check_linear(part.double().sum(1), x.double().sum(1), x.double().abs().sum(1), hw + 2, tag + " pooled sums")
    check_yardstick(gv.owned(), ref_gate, yard_gate, tag + " gate")
    ref_y = x.double() * (ref_gate[:, None, :] + alpha)
    yard_y = x * (yard_gate[:, None, :] + torch.tensor(alpha, dtype=torch.float32))
    check_yardstick(yv.owned().view(n, hw, c), ref_y, yard_y, tag + " scaled map")
    for v in (yv, pv, gv):
        v.assert_outside_untouched(tag)
    xv.assert_unchanged(tag)


def test_gate_alone_leaves_y_out():
    """y = null: launch_scale_channels does not run; the caller's partial sums are used as they are"""
    c, cr, n, chunks = 96, 24, 2, 5
    g = torch.Generator().manual_seed(7)
    part = torch.randn((n, chunks, c), generator=g) + 2.0
    weights = draw_weights(c, cr, part.double().sum(1) / 40.0, g)
    pv, gv = View(n * chunks, c, data=part), View(n, c)
    assert launch(n, 5, 8, c, cr, chunks, HSIG, 0.0, None, None, weights, pv, gv, 0) == 0
    extent = torch.full((n,), 40.0)
    ref, _ = se_formula(part.double().sum(1), extent, *weights, HSIG, torch.float64)
    yard, _ = se_formula(part.sum(1), extent, *weights, HSIG, torch.float32)
    check_yardstick(gv.owned(), ref, yard, "se gate alone")
    gv.assert_outside_untouched("se gate alone")
    pv.assert_unchanged("se gate alone")


@pytest.mark.parametrize("c", [8, 96, 132, 256, 512])
@pytest.mark.parametrize("chunks", [5, 64])
def test_pooled_mean_has_the_documented_fixed_order(c, chunks):
    """se_fc_kernel's comment promises a fixed order for every sum: slice sl of KS = max(1, min(8, 256 / (C / 4))) adds the partial rows
    sl, sl + KS, .., then the slices are added in order and the sum is multiplied by 1 / HW.  With W1 = W2 = identity (Cr = C), zero
    biases, no gate activation and positive sums every later product is by 0 or 1 and every later addition is of 0, so the gate IS that
    mean, to the bit (this is what notices a changed slice count, which the error bounds cannot: it only re-associates)."""
    n, hw = 3, 77
    g = torch.Generator().manual_seed(c + chunks)
    part = torch.rand((n, chunks, c), generator=g) + 0.25
    eye, zero = torch.eye(c), torch.zeros(c)
    pv, gv = View(n * chunks, c, data=part), View(n, c)
    assert launch(n, 7, 11, c, c, chunks, 0, 0.0, None, None, (eye, zero, eye, zero), pv, gv, 0) == 0
    ks = max(1, min(8, 256 // (c // 4)))
    total = torch.zeros((n, c))
    for sl in range(ks):
        s = torch.zeros((n, c))
        for k in range(sl, chunks, ks):
            s = s + part[:, k]
        total = total + s
    want = total * (torch.tensor(1.0) / torch.tensor(float(hw)))
    got = gv.owned()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), float((got - want).abs().max())
    gv.assert_outside_untouched("pooled mean order")


@pytest.mark.parametrize("c,cr", [(516, 129), (6, 2)])
def test_widths_beyond_the_limits_return_minus_one_and_touch_nothing(c, cr):
    n, hw = 2, 3
    ld = (c + 3) // 4 * 4
    g = torch.Generator().manual_seed(9)
    weights = (torch.randn((cr, c), generator=g), torch.zeros(cr), torch.randn((c, cr), generator=g), torch.zeros(c))
    xv = View(n * hw, c, ld, 0, data=torch.randn((n * hw, c), generator=g))
    yv, pv, gv = View(n * hw, c, ld, 0), View(n * 2, c, ld, 0), View(n, c, ld, 0)
    assert launch(n, 1, hw, c, cr, 2, HSIG, 0.0, xv, yv, weights, pv, gv, 1) == -1
    for v in (yv, pv, gv):
        assert bool(torch.isnan(v.owned()).all())
        v.assert_outside_untouched("declined width")
    xv.assert_unchanged("declined width")


def test_se_chain_fed_by_the_depthwise_partial_sums_under_a_line_table():
    """How the v6 recogniser blocks run under a line table: the 3x3 depthwise kernel (tiled8) writes the partial sums of its output over each
    line's own columns, se_fc_kernel divides them by H * line_w[n]."""
    n, h, w, c, cr = 3, 5, 21, 96, 24
    widths = [21, 1, 10]
    g = torch.Generator().manual_seed(11)
    x = torch.rand((n, h, w, c), generator=g) - 0.3
    wt = torch.rand((9, c), generator=g) - 0.5
    b = torch.rand((c,), generator=g) - 0.5
    xv, tv = View(n * h * w, c, data=x), View(n * h * w, c)
    lw = torch.tensor(widths, dtype=torch.int32, device="cuda")
    gap_cap = n * h * w * c
    gap = torch.full((gap_cap,), SENTINEL, device="cuda")
    chunks, name = C.c_int(-7), C.create_string_buffer(32)
    wd, bd = wt.cuda(), b.cuda()
    ms = lib().rd_debug_dwconv_ex(n, h, w, c, 3, 3, 1, 1, 1, 1, 1, 1, 0, c, c, c, 0, xv.ptr, wd.data_ptr(), bd.data_ptr(), None, tv.ptr, lw.data_ptr(), None,
                                  gap.data_ptr(), C.byref(chunks), name, 32)
    torch.cuda.synchronize()
    assert ms >= 0 and name.value == b"tiled8" and chunks.value > 0, (ms, name.value, chunks.value)
    nch = chunks.value
    xd = x.double().clone()
    for i, wl in enumerate(widths):
        xd[i, :, wl:, :] = 0
    t64 = torch.nn.functional.conv2d(xd.permute(0, 3, 1, 2), wt.double().t().reshape(c, 1, 3, 3), b.double(), padding=1, groups=c).permute(0, 2, 3, 1)
    pooled = torch.stack([t64[i, :, :wl].sum((0, 1)) for i, wl in enumerate(widths)])
    extent = torch.tensor([float(h * wl) for wl in widths])
    weights = draw_weights(c, cr, pooled / extent.double()[:, None], g)
    pv = View(n * nch, c, data=gap[:n * nch * c].cpu())          # the kernel's own sums, into a guarded buffer
    gv, yv = View(n, c), View(n * h * w, c, 128, 16)
    assert launch(n, h, w, c, cr, nch, HSIG, 0.0, tv, yv, weights, pv, gv, 0, line_w=lw) == 0
    ref_gate, pre = se_formula(pooled, extent, *weights, HSIG, torch.float64)
    assert float(pre.max()) > 3.2 and float(pre.min()) < -3.2
    # yardstick: the same chain by torch in fp32 - the depthwise conv, the mean over each line's own columns, the gate, the product
    t32 = torch.nn.functional.conv2d(xd.float().permute(0, 3, 1, 2), wt.t().reshape(c, 1, 3, 3), b, padding=1, groups=c).permute(0, 2, 3, 1)
    pooled32 = torch.stack([t32[i, :, :wl].sum((0, 1)) for i, wl in enumerate(widths)])
    yard_gate, _ = se_formula(pooled32, extent, *weights, HSIG, torch.float32)
    check_yardstick(gv.owned(), ref_gate, yard_gate, "se fed by tiled8, line_w %s: gate" % widths)
    check_yardstick(yv.owned().view(n, h, w, c), t64 * ref_gate[:, None, None, :], t32 * yard_gate[:, None, None, :], "se fed by tiled8: scaled map")
    for v in (gv, yv):
        v.assert_outside_untouched("se fed by tiled8")
    pv.assert_unchanged("se fed by tiled8")
