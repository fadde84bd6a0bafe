"""GPU: the two generic implicit-GEMM kernels alone - conv_igemm_kernel (fp32 MFMA, csrc/kernels_conv.hip, tiles 128x32 .. 128x128) and
conv_igemm_h3_kernel (split fp16, csrc/kernels_conv_h3.hip, tiles 256x128, 128x96, 256x64, 128x32, 128x64) - against torch's fp64 conv2d /
conv_transpose2d through the developer entry rd_debug_conv_ex, which launches them as the builder does: channel slots of wider buffers
(xld, yld, rld), both strides, OUT_DECONV2X2, the range flag.  A tile is forced by name, so that every tile is run at a few hundred rows
instead of at the M its routing rule needs; every launch asserts the route it ran on.  The bound is per output element (conv_helpers), so
one wrong row, column or tap of a corner tile cannot hide under the tensor's largest value, and every map is a view inside a
sentinel-filled buffer, so a store outside it is seen without a fault.  Across the tiles of one precision the output of a case is
bit-identical: every tile multiplies the same K steps in the same order.  Cases and measured ratios: docs/notebook/conv_tile_kernels.md.

Run as a script (`python tests/test_gpu_conv_tiles.py fast_epi_off FILE`) it runs the buffer-access epilogue's cases under the
environment it was started in and saves their outputs: RD_CONV_FAST_EPI is read once per process, so the test starts a fresh interpreter."""
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for _p in (str(ROOT), str(ROOT / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest
import torch

from conv_helpers import (F32_TILES, GELU, H3_TILES, IMG_3X3, NONE, RELU, SILU, Problem, assert_bit_identical, case, check_class_bound, check_launch, launch,
                          pointwise, tile_dims)

pytestmark = pytest.mark.gpu

TILES = {0: F32_TILES, 1: H3_TILES}
PREC = {0: "f32", 1: "h3"}
BOTH = [0, 1]


def on_every_tile(cs, seed, split, tiles=None, long_k=False, tag=""):
    """the case on each tile of the precision: the common checks per launch, and the outputs bit-identical to the first tile's"""
    pb = Problem(cs, seed)
    tag = "%s %s %s" % (PREC[split], tag, cs["why"])
    first, worst = None, {}
    for t in tiles or TILES[split]:
        r = launch(pb, split, force=t)
        worst[t] = check_launch(pb, r, split, t, tag)
        if long_k:
            check_class_bound(pb, r, tag)
        if first is None:
            first = (t, r.y)
        else:
            assert_bit_identical(first[1], r.y, (tag, first[0], "against", t))
    return pb, first[1], worst


def edge_case(bm, bn, act=RELU, res=True, k=36):
    """tile case 1: partial row and column tiles of a BM x BN tile, K = 36 (a tail of 4: one k-step), every view a slot whose width and
    offset differ from its channels - x at a multiple of 4 floats, y and res not"""
    ng = bn + 5
    return pointwise(bm + 37, k, ng, act=act, res=res, x_slot=(k + 28, 12), y_slot=(ng + 11, 5), r_slot=((ng + 3) if res else ng, 3 if res else 0),
                     why="M = %d + 37, Ng = %d + 5, K = %d, slots" % (bm, bn, k))


GEOMETRY_TILES = sorted(set(F32_TILES + H3_TILES))          # a geometry sized to one tile is run on every tile of the precision


# ----------------------------------------------------------------------------------------------------------------------- pointwise edges
@pytest.mark.parametrize("split", BOTH, ids=PREC.get)
@pytest.mark.parametrize("sized_to", GEOMETRY_TILES)
def test_partial_tiles_in_strided_views(split, sized_to):
    """#1"""
    on_every_tile(edge_case(*tile_dims(sized_to)), 1000 + sum(tile_dims(sized_to)), split, tag="#1")


@pytest.mark.parametrize("split", BOTH, ids=PREC.get)
def test_single_almost_empty_tile(split):
    """#2: M = 5, Ng = 1, K = 4: KT = 1, one quad of K"""
    on_every_tile(pointwise(5, 4, 1, why="M = 5, Ng = 1, K = 4"), 1100, split, tag="#2")


@pytest.mark.parametrize("split", BOTH, ids=PREC.get)
@pytest.mark.parametrize("k", [64, 96, 128])
@pytest.mark.parametrize("sized_to", GEOMETRY_TILES)
def test_exactly_full_tiles(split, k, sized_to):
    """#3: M = BM, Ng = BN; KT = 2, 3, 4: the double-buffered K loop of the 8-wavefront tiles leaves at each of its exits"""
    bm, bn = tile_dims(sized_to)
    on_every_tile(pointwise(bm, k, bn, act=RELU, why="M = %d, Ng = %d, K = %d" % (bm, bn, k)), 1200 + k + bm + bn, split, tag="#3")


@pytest.mark.parametrize("split", BOTH, ids=PREC.get)
def test_k_tail_of_two_k_steps(split):
    """#4: K = 180 = 5 x 32 + 20: the tail tile has kleft in 17 .. 31 (both k-steps of the split kernel, three groups of the fp32 one)"""
    on_every_tile(pointwise(133, 180, 37, res=True, r_slot=(40, 3), y_slot=(45, 7), why="K = 180"), 1300, split, tag="#4")


# ------------------------------------------------------------------------------------------------------------------------------ k x k
KXK = [
    (case(3, 5, 7, 20, 40, k=(3, 3), pad=(1, 1, 1, 1), bias=False, why="3x3 s1 pad 1, N = 3, 5x7x20 -> 40, bias = null: image borders inside a row tile"), False),
    (case(2, 9, 11, 12, 24, k=(3, 3), s=(2, 2), pad=(1, 1, 1, 1), act=SILU, why="3x3 s2 pad 1, 9x11 (odd H and W), SiLU: the B4 down-sampling form"), False),
    (case(1, 8, 9, 8, 16, k=(3, 3), s=(2, 1), pad=(1, 1, 1, 1), why="3x3 stride (2, 1): SH != SW"), False),
    (case(2, 6, 9, 12, 24, k=(2, 2), pad=(0, 0, 1, 1), x_slot=(16, 4), y_slot=(29, 3), why="2x2 pad (0, 0, 1, 1): far sides only (stem2), slots"), False),
    (case(2, 6, 10, 8, 24, k=(5, 5), pad=(2, 2, 2, 2), act=RELU, why="5x5 pad 2, Cin 8 on 6x10, K = 200"), False),
    (case(2, 6, 10, 4, 24, k=(7, 7), pad=(3, 3, 3, 3), res=True, r_slot=(27, 3), why="7x7 pad 3, Cin 4 on 6x10: a map lower than the kernel, K = 196"), False),
    (case(2, 6, 10, 4, 24, k=(9, 9), pad=(4, 4, 4, 4), act=RELU, why="9x9 pad 4, Cin 4 on 6x10, K = 324 (long K: the class bound too)"), True),
]


@pytest.mark.parametrize("split", BOTH, ids=PREC.get)
@pytest.mark.parametrize("i", range(len(KXK)), ids=lambda i: "%dx%d-s%d%d" % (KXK[i][0]["k"] + KXK[i][0]["s"]))
def test_kxk_geometries(split, i):
    """#5 .. #9"""
    on_every_tile(KXK[i][0], 1400 + i, split, long_k=KXK[i][1], tag="#%d" % (5 + min(i, 4)))


# ------------------------------------------------------------------------------------------------------------------------- activations
@pytest.mark.parametrize("split,tile", [(0, "128x64"), (1, "128x96"), (1, "256x64")], ids=["f32-128x64", "h3-128x96", "h3-256x64"])
@pytest.mark.parametrize("act", range(7))
def test_every_activation(split, tile, act):
    """#10: each branch of the epilogue's activation switch on #1's geometry (256x64: its first row tile takes the buffer-access epilogue)"""
    pb = Problem(edge_case(*tile_dims(tile), act=act), 1500 + act)
    check_launch(pb, launch(pb, split, force=tile), split, tile, "#10 %s act %d" % (PREC[split], act))


# ------------------------------------------------------------------------------------------------------------- persistent loop, map_tile
@pytest.mark.parametrize("tile", ["256x128", "256x64"])
def test_persistent_second_round(tile):
    """#11: more tiles than CUs and no multiple of 8: the second round of the persistent loop (the next tile's first K tiles requested across
    the epilogue) and map_tile's remainder branch.  The same problem on a 4-wavefront tile must give the same bits."""
    bm, bn = tile_dims(tile)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ntn = 11
    ntm = next(m for m in range(cus // ntn + 1, 2 * cus // ntn + 1) if (m * ntn) % 8 != 0)
    assert cus < ntm * ntn <= 2 * cus
    ng = 10 * bn + 5
    cs = pointwise(ntm * bm - 19, 36, ng, act=RELU, res=True, x_slot=(64, 12), y_slot=(ng + 11, 5), r_slot=(ng + 3, 3),
                   why="%d x %d = %d tiles on %d CUs" % (ntm, ntn, ntm * ntn, cus))
    on_every_tile(cs, 1600 + bn, 1, tiles=[tile, "128x64"], tag="#11")


@pytest.mark.parametrize("split", BOTH, ids=PREC.get)
@pytest.mark.parametrize("ntm,ntn", [(3, 1), (3, 3)], ids=["3-tiles", "9-tiles"])
def test_tile_numbering_below_eight(split, ntm, ntn):
    """#12: ntiles = 3 and 9: map_tile with q = 0 (r = 3) and q = 1, r = 1"""
    for t in TILES[split]:
        bm, bn = tile_dims(t)
        ng = ntn * bn - 3
        pb = Problem(pointwise(ntm * bm - 5, 36, ng, y_slot=(ng + 6, 1), why="%d x %d tiles of %s" % (ntm, ntn, t)), 1700 + ntn + bm + bn)
        check_launch(pb, launch(pb, split, force=t), split, t, "#12 " + PREC[split])


# ------------------------------------------------------------------------------------------------------------ buffer-access epilogue
FAST_CASES = [(ng, res, act) for ng in (64, 45) for res in (True, False) for act in (RELU, GELU, SILU, NONE)]


def fast_epilogue_outputs():
    """#13: 256x64 forced, M = 2 x 256 + 37: two interior row tiles (buffer accesses, no bounds test) next to a last one on the generic
    epilogue; y and res in slots whose offsets are no multiple of 4"""
    outs = []
    for j, (ng, res, act) in enumerate(FAST_CASES):
        cs = pointwise(2 * 256 + 37, 36, ng, act=act, res=res, x_slot=(64, 12), y_slot=(ng + 11, 5), r_slot=(ng + 3, 3) if res else None,
                       why="Ng = %d, res = %s, act = %d" % (ng, res, act))
        pb = Problem(cs, 1800 + j)
        r = launch(pb, 1, force="256x64")
        check_launch(pb, r, 1, "256x64", "#13 RD_CONV_FAST_EPI=%s" % os.environ.get("RD_CONV_FAST_EPI", "unset"))
        outs.append(r.y)
    return outs


def test_fast_epilogue_gives_the_generic_epilogue_s_bits(tmp_path):
    assert os.environ.get("RD_CONV_FAST_EPI") in (None, "1"), "this test needs the default epilogue in its own process"
    here = fast_epilogue_outputs()
    path = tmp_path / "generic.pt"
    env = dict(os.environ, RD_CONV_FAST_EPI="0")
    r = subprocess.run([sys.executable, __file__, "fast_epi_off", str(path)], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-2500:])
    there = torch.load(path)
    assert len(there) == len(here)
    for (ng, res, act), a, b in zip(FAST_CASES, here, there):
        assert_bit_identical(a, b, ("#13 fast against generic epilogue", ng, res, act))


# ------------------------------------------------------------------------------------------------------------------------------ deconv
@pytest.mark.parametrize("split", BOTH, ids=PREC.get)
@pytest.mark.parametrize("cout", [10, 40])
def test_deconv2x2_scatter(split, cout):
    """#14: OUT_DECONV2X2 from the checkpoint layout through pack_deconv2x2.  Ng = 4 Cout = 40 and 160 (two column tiles of the widest tile,
    tap boundaries inside a tile); the reference with transposed taps is far from the right one, so a dy / dx mix-up cannot pass."""
    cs = case(2, 5, 7, 12, cout, act=RELU, deconv=True, y_slot=(cout + 6, 3), why="deconv 2x5x7x12 -> %d" % cout)
    pb, y, _ = on_every_tile(cs, 1900 + cout, split, tag="#14")
    assert float((pb.ref - pb.transposed).abs().max()) > 0.05
    assert float((y.double() - pb.transposed).abs().max()) > 0.05


# -------------------------------------------------------------------------------------------------------------------------- range flag
@pytest.mark.parametrize("tile", H3_TILES)
def test_range_flag(tile):
    """#15: one activation beyond the fp16 range raises the flag (the same case without it: #1, flag 0); the stores stay inside the view"""
    pb = Problem(edge_case(*tile_dims(tile)), 2000)
    r = launch(pb, 1, force=tile, x_poke=(3, 5, 1e5))
    assert r.ms >= 0 and r.route == tile
    assert r.flag == 1, (tile, "the range flag stayed down")
    r.yv.assert_outside_untouched("#15 " + tile)
    r.xv.assert_unchanged("#15 " + tile)
    r.rv.assert_unchanged("#15 " + tile)
    # the offending activation splits into hi = inf: its row is inf / NaN before the activation (a NaN leaves ReLU as 0); every other row is
    # an ordinary result
    others = torch.arange(pb.rows) != 3
    assert bool(torch.isfinite(r.y[others]).all()), (tile, "a row other than the offending one is not finite")
    err = (r.y.double() - pb.ref).abs()[others]
    assert bool((err <= pb.bound(1)[others]).all()), (tile, "rows beside the offending one", float(err.max()))


# ---------------------------------------------------------------------------------------------------------------------- natural routes
NATURAL = [
    # split: the rules of h3_pick_tile, each on a layer no specialised kernel takes (no one-accumulator image; Cin > 64 or Cout > 96 keeps
    # the streaming kernel away, Ng < 96 the LDS-DMA GEMM)
    (1, "256x128", case(2, 9, 11, 8, 100, k=(3, 3), s=(2, 2), pad=(1, 1, 1, 1), why="Ng > 96 (3x3 stride 2)")),
    (1, "256x64", pointwise(65536, 68, 40, why="32 < Ng <= 64 and M >= 65536")),
    (1, "128x96", pointwise(300, 68, 80, why="64 < Ng <= 96")),
    (1, "128x32", pointwise(300, 68, 24, why="Ng <= 32")),
    (1, "128x32", pointwise(300, 68, 40, why="Ng <= 64, K <= 256")),
    (1, "128x64", pointwise(300, 260, 40, why="32 < Ng <= 64, K > 256, M < 65536")),
    # fp32: the rules of conv_f32_route
    (0, "128x32", pointwise(300, 36, 24, why="Ng <= 32")),
    (0, "128x64", pointwise(300, 36, 40, why="Ng <= 64")),
    (0, "128x96", pointwise(300, 36, 80, why="Ng <= 96")),
    (0, "128x128", pointwise(300, 36, 100, why="Ng = 100: 128 padded columns against 192")),
    (0, "128x96", pointwise(300, 36, 130, why="Ng = 130: 192 padded columns against 256")),
]


@pytest.mark.parametrize("i", range(len(NATURAL)), ids=lambda i: "%s-%s-%d" % (PREC[NATURAL[i][0]], NATURAL[i][1], i))
def test_natural_route_is_the_forced_tile(i):
    """#16: without `force` the entry asks conv_split_route / conv_f32_route as the builder does; the result equals the forced run of that tile"""
    split, tile, cs = NATURAL[i]
    pb = Problem(cs, 2100 + i)
    nat = launch(pb, split)
    check_launch(pb, nat, split, tile, "#16 natural " + cs["why"])
    forced = launch(pb, split, force=tile)
    check_launch(pb, forced, split, tile, "#16 forced " + cs["why"])
    assert_bit_identical(nat.y, forced.y, ("#16", cs["why"]))


# ----------------------------------------------------------------------------------------------------------------------------- refusals
def test_refused_arguments_launch_nothing():
    """-1: Cin % 4, xld % 4, views narrower than their channels, res or a k x k geometry with OUT_DECONV2X2, a `force` that is no tile of the
    precision, ln_g on a route that is not "skinny".  -2: ascale, which no kernel applies - the launcher throws instead of running the layer
    ungated.  Nothing is written in any of them."""
    pb = Problem(edge_case(128, 64), 2200)
    ones = torch.ones(64)
    dec = Problem(case(2, 5, 7, 12, 10, deconv=True, why="deconv"), 2201)
    spare = launch(Problem(case(2, 10, 14, 12, 10, why="a buffer for the residual pointer"), 2202), 0)
    runs = [
        ("Cin % 4", launch(pb, 1, force="128x64", overrides=dict(Cin=34)), -1),
        ("xld % 4", launch(pb, 1, force="128x64", overrides=dict(xld=62)), -1),
        ("xld < Cin", launch(pb, 0, force="128x64", overrides=dict(xld=32)), -1),
        ("yld < Cout", launch(pb, 0, force="128x64", overrides=dict(yld=68)), -1),
        ("rld < Cout", launch(pb, 1, force="128x64", overrides=dict(rld=68)), -1),
        ("a split tile on the fp32 path", launch(pb, 0, force="256x64"), -1),
        ("an fp32 tile on the split path", launch(pb, 1, force="128x128"), -1),
        ("no tile at all", launch(pb, 1, force="dma256x128"), -1),
        ("ln_g on a tile", launch(pb, 0, force="128x64", ln=(ones[:36], ones[:36])), -1),
        ("ln_g on the natural split route", launch(pb, 1, ln=(ones[:36], ones[:36])), -1),
        ("deconv with a 3x3 geometry", launch(dec, 1, overrides=dict(KH=3, KW=3, PT=1, PL=1, PB=1, PR=1)), -1),
        ("deconv with a residual", launch(dec, 0, overrides=dict(res=spare.yv.ptr)), -1),
        ("ascale, split, forced", launch(pb, 1, force="128x64", ascale=ones[:36]), -2),
        ("ascale, split, natural", launch(pb, 1, ascale=ones[:36]), -2),
        ("ascale, fp32", launch(pb, 0, ascale=ones[:36]), -2),
    ]
    for what, r, code in runs:
        assert r.ms == code, (what, r.ms)
        assert bool(torch.isnan(r.y).all()), (what, "the output view was written")
        r.yv.assert_outside_untouched(what)
        r.xv.assert_unchanged(what)


def test_rd_debug_conv_still_takes_the_one_accumulator_3x3():
    """rd_debug_conv shares rd_debug_conv_ex's body: with the 3x3 image the natural route of a 3x3 / stride 1 layer is `c3h1` in both, and the
    two entries give the same bits"""
    import ctypes as C
    from glue_helpers import lib
    cs = case(2, 12, 20, 32, 48, k=(3, 3), pad=(1, 1, 1, 1), act=RELU, why="3x3 s1 32 -> 48")
    pb = Problem(cs, 2300)
    r = launch(pb, 1, images=IMG_3X3)
    assert r.ms >= 0 and r.route == "c3h1" and r.flag == 0, (r.ms, r.route, r.flag)
    check_class_bound(pb, r, "rd_debug_conv_ex on c3h1")          # (that kernel's own test: tests/test_gpu_conv3x3_h1.py)
    wf = pb.w_dev_src.cuda()
    hi = wf.half()
    lo = ((wf - hi.float()) * 2048.0).half()
    kp = (pb.K + 31) // 32 * 32
    wh = torch.zeros((48, kp), dtype=torch.float16, device="cuda"); wh[:, :pb.K] = hi
    wl = torch.zeros((48, kp), dtype=torch.float16, device="cuda"); wl[:, :pb.K] = lo
    x, b = pb.x.cuda(), pb.b_ck.cuda()
    y = torch.full((pb.rows, 48), float("nan"), device="cuda")
    used = C.c_int(0)
    ms = lib().rd_debug_conv(2, 12, 20, 32, 48, 3, 3, 1, 1, 1, 1, 1, RELU, 0, x.data_ptr(), wf.data_ptr(), wh.data_ptr(), wl.data_ptr(), b.data_ptr(), None,
                             y.data_ptr(), C.byref(used))
    torch.cuda.synchronize()
    assert ms >= 0 and used.value == 3
    assert_bit_identical(r.y, y.cpu(), "rd_debug_conv against rd_debug_conv_ex")


if __name__ == "__main__":
    assert sys.argv[1] == "fast_epi_off" and os.environ.get("RD_CONV_FAST_EPI") == "0"
    torch.save(fast_epilogue_outputs(), sys.argv[2])
    print("saved", len(FAST_CASES), "outputs")
