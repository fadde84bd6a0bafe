"""GPU: the small-M fp32 GEMM of the formula decoder's linears alone (csrc/kernels_conv.hip: skinny2_gemm_kernel<8,4,2>, <8,4,4>, <16,2,2>,
<16,2,4>, <32,2,2> and the chunked skinny_gemm_kernel<8 / 16 / 32>) against fp64 through rd_debug_conv_ex with allow_skinny = 1: every
instantiation launch_skinny picks (M <= 8, <= 16, <= 32; K <= 512, the wide passes up to 2048, the chunked kernel for M = 32 with K > 512 and
for K > 2048), N = 6 (wavefronts that own no column) and 130 (a partial last block), strided x, y and res, and the fused LayerNorm the route
alone honours.  Without the LayerNorm the bound is (K + 3) 2^-24 (sum |x w| + |bias|) + 2^-24 |res| per element, which holds for any
summation order; with it (non-linear) the yardstick rule of glue_helpers.  Cases and measured ratios: docs/notebook/conv_tile_kernels.md."""
import pytest
import torch

from conv_helpers import NONE, RELU, Problem, activation, check_class_bound, check_launch, launch, pointwise
from glue_helpers import check_yardstick

pytestmark = pytest.mark.gpu

MS = [1, 8, 9, 16, 17, 32]
KS = [64, 508, 512, 516, 2048, 2052]


def skinny_case(m, k, n, act, res):
    return pointwise(m, k, n, act=act, res=res, x_slot=(k + 12, 8), y_slot=(n + 7, 5), r_slot=(n + 3, 3) if res else None, why="M %d K %d N %d" % (m, k, n))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m", MS)
def test_skinny_matches_fp64(m, k):
    for n, act, res in ((6, RELU, True), (130, NONE, True), (130, RELU, False)):
        pb = Problem(skinny_case(m, k, n, act, res), 4000 + 100 * m + k + n)
        r = launch(pb, 0, allow_skinny=1)
        check_launch(pb, r, 0, "skinny", "skinny " + pb.cs["why"])
        if k > 200:                                   # (the per-element bound grows with K: the class bound on top)
            check_class_bound(pb, r, "skinny " + pb.cs["why"])


def layer_norm_reference(pb, g, b, dtype):
    x = pb.x.reshape(pb.rows, pb.K).to(dtype)
    xn = torch.nn.functional.layer_norm(x, (pb.K,), g.to(dtype), b.to(dtype), eps=1e-5)
    out = activation(xn @ pb.w_dev_src.to(dtype).t() + pb.b_ck.to(dtype), pb.cs["act"])
    return out + pb.res.to(dtype) if pb.res is not None else out


@pytest.mark.parametrize("k", [64, 508, 512])
@pytest.mark.parametrize("m", MS)
def test_skinny_fused_layernorm(m, k):
    """the pre-LayerNorm (eps 1e-5) of a decode step, fused: fp64 LayerNorm followed by the product"""
    for n, act, res in ((6, NONE, False), (130, RELU, True)):
        pb = Problem(skinny_case(m, k, n, act, res), 5000 + 100 * m + k + n)
        gen = torch.Generator().manual_seed(m * k + n)
        g, b = torch.rand(k, generator=gen) + 0.5, torch.rand(k, generator=gen) - 0.5
        tag = "skinny + LayerNorm " + pb.cs["why"]
        r = launch(pb, 0, allow_skinny=1, ln=(g, b))
        assert r.ms >= 0 and r.route == "skinny" and r.flag == 0, (tag, r.ms, r.route, r.flag)
        r.yv.assert_outside_untouched(tag)
        r.xv.assert_unchanged(tag)
        if r.rv is not None:
            r.rv.assert_unchanged(tag)
        check_yardstick(r.y, layer_norm_reference(pb, g, b, torch.float64), layer_norm_reference(pb, g, b, torch.float32), tag)


def test_what_the_skinny_route_does_not_take():
    """M = 33 is a tile's (asserted, and still right); with ln_g nothing but `skinny` may run: M = 33 and K = 516 are declined, nothing written"""
    pb = Problem(skinny_case(33, 64, 130, RELU, True), 6000)
    check_launch(pb, launch(pb, 0, allow_skinny=1), 0, "128x96", "M = 33 with allow_skinny")
    ones = torch.ones(516)
    for what, pb, kk in (("M = 33 with ln_g", pb, 64), ("K = 516 with ln_g", Problem(skinny_case(8, 516, 130, NONE, False), 6001), 516)):
        r = launch(pb, 0, allow_skinny=1, ln=(ones[:kk], ones[:kk]))
        assert r.ms == -1, (what, r.ms)
        assert bool(torch.isnan(r.y).all()), (what, "the output view was written")
        r.yv.assert_outside_untouched(what)
