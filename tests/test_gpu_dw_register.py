"""GPU: the register depthwise kernels of csrc/kernels_misc.hip alone - dwconv_tiled_kernel<3,3,1,8>, <3,3,2,4>, <5,5,1,8>, <7,7,1,4>, the
per-pixel dwconv_kernel (1 x k, ragged token rows) and, under RD_DW_COL=1, dwconv3x3_col_kernel - against torch's fp64 grouped convolution
through the general developer entry rd_debug_dwconv_ex: strides, strided channel slots, line widths, the SE partial sums, both epilogues.
Every case names the route it expects, so it cannot silently run another kernel, and every buffer is a view inside a sentinel-filled one, so
a store outside it is seen without a fault.  The LDS routes are run once each with xld != C, and their geometries again under RD_DW_LDS=0.

Bound (exact for fp32, any summation or FMA order): |err| <= (taps + 2) 2^-24 (sum |x w| + |bias|) + 2^-24 |res| per output; for the SE sums
the same with OH OW + taps + 2 terms over the summed outputs.  Cases and measured ratios: docs/notebook/glue_kernels.md.

Run as a script (`python tests/test_gpu_dw_register.py lds_off | col | tw`) it runs the cases of one switch: RD_DW_LDS, RD_DW_COL and the
RD_DW*_TW widths are read once per process, so the tests start it in a fresh interpreter."""
import ctypes as C
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

from glue_helpers import SENTINEL, View, check_linear, lib

pytestmark = pytest.mark.gpu

NONE, RELU = 0, 1


def case(n, h, w, c, k=(3, 3), s=(1, 1), route=None, act=NONE, res=False, bias=True, gap=True, widths=None, lines=None, x_slot=None, y_slot=None,
         r_slot=None, chunks=None, why=""):
    """k = (KH, KW), s = (SH, SW), 'same' padding; *_slot = (ld, offset) of the view inside a wider buffer; lines = the token counts of the
    ragged row's text lines (N = H = 1, W = their sum); chunks = the SE chunk count expected (None: not pinned)"""
    return dict(n=n, h=h, w=w, c=c, k=k, s=s, route=route, act=act, res=res, bias=bias, gap=gap, widths=widths, lines=lines, x_slot=x_slot,
                y_slot=y_slot, r_slot=r_slot, chunks=chunks, why=why)


def tiled_chunks(c, oh, ow, tw):
    """dw_tiled_geom on a small map (one group per pixel lane): ceil(OH ceil(OW / TW) / (256 / (C / 4)))"""
    lanes = 256 // (c // 4)
    return -(-(oh * -(-ow // tw)) // lanes)


SLOT_X, SLOT_Y, SLOT_R = (96, 32), (64, 0), (40, 8)          # a 32-channel op: xld, yld, rld differ from C and from each other

CASES = [
    # ---- 3x3 stride 1 -> tiled8 (H outside {3, 6, 12}); OW no multiple of 8; c4n that does not divide 256, c4n = 1, C = 192
    case(2, 5, 33, 24, route="tiled8", act=RELU, res=True, chunks=1, why="252 threads, OW = 33: 25 groups on 42 pixel lanes"),
    case(2, 7, 9, 96, route="tiled8", bias=False, chunks=2, why="240 threads, bias = null, OW = 9: 14 groups = 10 + 4"),
    case(1, 4, 1, 4, route="tiled8", chunks=1, why="c4n = 1, one column, one chunk"),
    case(2, 7, 9, 192, route="tiled8", res=True, chunks=3, why="five pixel lanes: 14 groups = 3 chunks, the last of 4"),
    case(1, 5, 7, 192, route="tiled8", act=RELU, chunks=1, why="one chunk exactly full"),
    case(2, 2, 7, 24, route="tiled8", gap=False, act=RELU, why="no SE sums asked"),
    # ---- line widths on a stride-1 case with the SE sums: W, 1, W - 1, and 10 = inside the TW group 8 .. 15
    case(4, 5, 21, 96, route="tiled8", widths=[21, 1, 20, 10], act=RELU, res=True, why="columns beyond a line: zero to the taps, out of the sums"),
    # ---- 3x3 stride (2, 2) -> tiled4, both parities of H and W
    case(2, 8, 10, 24, s=(2, 2), route="tiled4", act=RELU, why="H even, W even"),
    case(2, 7, 9, 96, s=(2, 2), route="tiled4", res=True, why="H odd, W odd"),
    case(1, 8, 9, 4, s=(2, 2), route="tiled4", bias=False, why="H even, W odd, c4n = 1"),
    case(2, 7, 66, 192, s=(2, 2), route="tiled4", act=RELU, res=True, chunks=tiled_chunks(192, 4, 33, 4), why="H odd, W even, OW = 33, 8 chunks"),
    case(1, 1, 1, 24, s=(2, 2), route="tiled4", why="a 1 x 1 map"),
    # ---- 5x5 / 7x7 with the SE sums wanted: off kxk_lds
    case(2, 6, 9, 96, k=(5, 5), route="tiled8", act=RELU, res=True, why="5x5, C % 32 == 0: only the SE sums keep it off kxk_lds5"),
    case(1, 4, 33, 32, k=(5, 5), route="tiled8", widths=[17], why="5x5 under a line width"),
    case(2, 9, 7, 32, k=(7, 7), route="tiled4", act=RELU, why="7x7, map smaller than the kernel on one side"),
    case(1, 4, 33, 96, k=(7, 7), route="tiled4", res=True, bias=False, why="7x7, OW = 33"),
    # ---- the per-pixel kernel
    case(2, 3, 9, 24, k=(1, 7), route="pixel", act=RELU, res=True, why="1 x 7 'same' (the local mixer of the v5 neck)"),
    case(1, 1, 40, 96, k=(1, 3), route="pixel", lines=[1, 2, 37], res=True, why="ragged token row: taps stop at each line's ends"),
    case(1, 1, 40, 96, k=(1, 3), route="pixel", lines=[37, 1, 2], act=RELU, bias=False, why="ragged row, the short lines last"),
    # ---- strided views: a channel slot of a concat buffer in, another out, a third for the residual
    case(2, 5, 9, 32, route="tiled8", act=RELU, res=True, x_slot=SLOT_X, y_slot=SLOT_Y, r_slot=SLOT_R, why="slots on tiled8"),
    case(2, 3, 9, 32, k=(1, 7), route="pixel", res=True, x_slot=SLOT_X, y_slot=SLOT_Y, r_slot=SLOT_R, why="slots on pixel"),
    case(2, 6, 19, 64, route="lds1", act=RELU, res=True, x_slot=(192, 64), y_slot=(128, 0), r_slot=(80, 16), chunks=2, why="slots on lds1 (xld != C)"),
    case(2, 9, 17, 32, k=(5, 5), route="kxk_lds5", gap=False, act=RELU, res=True, x_slot=SLOT_X, y_slot=SLOT_Y, r_slot=SLOT_R, why="slots on kxk_lds5"),
]

# the geometries of four LDS routes (+ the 7x7 one); under RD_DW_LDS=0 the register kernels take them
LDS_GEOMETRIES = [
    (case(2, 6, 19, 64, act=RELU, res=True, chunks=None), "lds1", "tiled8"),
    (case(2, 12, 17, 32, widths=[17, 9]), "lds2", "tiled8"),
    (case(2, 12, 9, 32, s=(2, 1), act=RELU), "lds4", "tiled8"),
    (case(2, 9, 17, 32, k=(5, 5), gap=False, res=True), "kxk_lds5", "tiled8"),
    (case(1, 5, 9, 32, k=(7, 7), gap=False, act=RELU), "kxk_lds7", "tiled4"),
]

# RD_DW_COL=1: 3x3 stride 1 on the column-strip kernel
COL_CASES = [
    case(1, 1, 1, 4, route="col", chunks=1, why="H = 1, W = 1"),
    case(2, 2, 4, 24, route="col", act=RELU, why="H = 2, one full strip"),
    case(2, 5, 5, 96, route="col", act=RELU, res=True, why="H = 5, W = 5: the second strip has one column"),
    case(3, 5, 33, 96, route="col", widths=[33, 1, 18], res=True, why="line widths, SE sums, residual"),
    case(2, 2, 33, 192, route="col", bias=False, chunks=2, why="9 strips on five pixel lanes: the last chunk is short"),
    case(1, 1, 33, 24, route="col", act=RELU, x_slot=(40, 8), y_slot=(32, 4), why="H = 1, strided"),
]


# RD_DW3_TW=4 RD_DW5_TW=4 RD_DW7_TW=8: the other width of each stride-1 instantiation (<3,3,1,4>, <5,5,1,4>, <7,7,1,8>)
TW_CASES = [
    case(2, 5, 33, 24, route="tiled4", act=RELU, res=True, widths=[33, 6], why="<3,3,1,4>, OW = 33, a line ending inside a group"),
    case(2, 6, 9, 96, k=(5, 5), route="tiled4", bias=False, why="<5,5,1,4>"),
    case(1, 4, 33, 96, k=(7, 7), route="tiled8", act=RELU, res=True, why="<7,7,1,8>, OW = 33"),
]


def reference(cs, x, w, b, r):
    """(output, sum |x w| + |bias|) in fp64, [N][OH][OW][C]; x [N][H][W][C], w [KH KW][C]"""
    n, h, wd, c = x.shape
    kh, kw = cs["k"]
    pt, pl = kh // 2, kw // 2
    xd, wk = x.double().clone(), w.double().t().reshape(c, 1, kh, kw)
    if cs["widths"] is not None:
        for i, wl in enumerate(cs["widths"]):
            xd[i, :, wl:, :] = 0

    def conv(xx, ww, bb):
        f = lambda t: torch.nn.functional.conv2d(t.permute(0, 3, 1, 2), ww, bb, stride=cs["s"], padding=(pt, pl), groups=c).permute(0, 2, 3, 1)
        if cs["lines"] is None:
            return f(xx)
        out, at = [], 0
        for ln in cs["lines"]:                    # the conv applied per text line, zero padding at the line's ends
            out.append(f(xx[:, :, at:at + ln]))
            at += ln
        return torch.cat(out, dim=2)

    ref = conv(xd, wk, b.double() if b is not None else None)
    mag = conv(xd.abs(), wk.abs(), b.double().abs() if b is not None else None)
    if cs["act"] == RELU:
        ref = ref.clamp_min(0)
    if r is not None:
        ref = ref + r.double()
    return ref, mag


def run_case(cs, seed):
    """One launch; asserts the route, the bounds of the output and of the SE sums, and that nothing outside the views was written.  Returns
    (route, chunks, worst output ratio, worst SE-sum ratio or None)."""
    n, h, w, c = cs["n"], cs["h"], cs["w"], cs["c"]
    (kh, kw), (sh, sw) = cs["k"], cs["s"]
    pt, pl = kh // 2, kw // 2
    oh, ow = (h + 2 * pt - kh) // sh + 1, (w + 2 * pl - kw) // sw + 1
    taps = kh * kw
    tag = "dw %dx%d s%d%d N%d %dx%dx%d %s" % (kh, kw, sh, sw, n, h, w, c, cs["why"] or cs["route"])
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((n, h, w, c), generator=g) - 0.5
    wt = torch.rand((taps, c), generator=g) - 0.5
    b = (torch.rand((c,), generator=g) - 0.5) if cs["bias"] else None
    r = (torch.rand((n, oh, ow, c), generator=g) - 0.5) if cs["res"] else None
    xs, ys, rs = cs["x_slot"] or (c, 0), cs["y_slot"] or (c, 0), cs["r_slot"] or (c, 0)
    xv = View(n * h * w, c, xs[0], xs[1], data=x)
    yv = View(n * oh * ow, c, ys[0], ys[1])
    rv = View(n * oh * ow, c, rs[0], rs[1], data=r) if r is not None else None
    wv, bv = wt.cuda(), b.cuda() if b is not None else None
    gap_cap = n * oh * ow * c + c
    gap = torch.full((gap_cap,), SENTINEL, device="cuda")
    lw = torch.tensor(cs["widths"], dtype=torch.int32, device="cuda") if cs["widths"] is not None else None
    ti = None
    if cs["lines"] is not None:
        assert n == 1 and h == 1 and sum(cs["lines"]) == w
        ti = torch.tensor([(ln << 16) | pos for ln in cs["lines"] for pos in range(ln)], dtype=torch.int32, device="cuda")
    chunks, name = C.c_int(-7), C.create_string_buffer(32)
    ms = lib().rd_debug_dwconv_ex(n, h, w, c, kh, kw, sh, sw, pt, pl, pt, pl, cs["act"], xs[0], ys[0], rs[0], 0, xv.ptr, wv.data_ptr(),
                                  bv.data_ptr() if bv is not None else None, rv.ptr if rv is not None else None, yv.ptr,
                                  lw.data_ptr() if lw is not None else None, ti.data_ptr() if ti is not None else None,
                                  gap.data_ptr() if cs["gap"] else None, C.byref(chunks), name, 32)
    torch.cuda.synchronize()
    assert ms >= 0, (tag, "the entry declined the arguments")
    route = name.value.decode()
    assert route == cs["route"], (tag, "ran on", route)
    ref, mag = reference(cs, x, wt, b, r)
    y = yv.owned().reshape(n, oh, ow, c)
    bound_mag = (taps + 2) * mag + (r.double().abs() if r is not None else 0)
    ratio = check_linear(y, ref, bound_mag, 1, tag)
    yv.assert_outside_untouched(tag)
    xv.assert_unchanged(tag)
    if rv is not None:
        rv.assert_unchanged(tag)
    gratio = None
    nch = chunks.value
    if cs["chunks"] is not None:
        assert nch == cs["chunks"], (tag, "SE chunks", nch)
    gap_h = gap.cpu()
    used = n * nch * c if (cs["gap"] and nch > 0) else 0
    if cs["gap"] and route != "pixel":
        assert nch > 0, (tag, "no SE sums from", route)
    assert bool((gap_h[used:] == SENTINEL).all()), (tag, "stores past the SE partial sums")
    if used:
        part = gap_h[:used].view(n, nch, c)
        assert bool(torch.isfinite(part).all()), (tag, "an SE chunk was not written")
        wl = cs["widths"] if cs["widths"] is not None else [ow] * n
        want = torch.stack([ref[i, :, :wl[i], :].sum((0, 1)) for i in range(n)])
        gmag = torch.stack([(mag + (r.double().abs() if r is not None else 0))[i, :, :wl[i], :].sum((0, 1)) for i in range(n)])
        gratio = check_linear(part.double().sum(1), want, gmag, oh * ow + taps + 2, tag + " SE sums")
    return route, nch, ratio, gratio


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: "%02d-%s" % (i, CASES[i]["route"]))
def test_dw_register_matches_fp64(i):
    run_case(CASES[i], 100 + i)


@pytest.mark.parametrize("i", range(len(LDS_GEOMETRIES)), ids=lambda i: LDS_GEOMETRIES[i][1])
def test_lds_geometries_take_the_lds_routes_by_default(i):
    cs, name, _ = LDS_GEOMETRIES[i]
    run_case({**cs, "route": name, "why": "default route"}, 200 + i)


def test_bad_arguments_launch_nothing():
    yv = View(2 * 5 * 9, 32)
    xv = View(2 * 5 * 9, 32, data=torch.zeros(90, 32))
    w = torch.zeros((9, 32), device="cuda")
    name = C.create_string_buffer(32)

    def call(c=32, xld=32, yld=32, sw=1, ti=None, lwp=None, kh=3, n=2, h=5):
        return lib().rd_debug_dwconv_ex(n, h, 9, c, kh, 3, 1, sw, kh // 2, 1, kh // 2, 1, 0, xld, yld, 32, 0, xv.ptr, w.data_ptr(), None, None, yv.ptr, lwp, ti,
                                        None, None, name, 32)
    some = torch.zeros(16, dtype=torch.int32, device="cuda")
    assert call(c=30) == -1 and call(xld=28) == -1 and call(yld=34) == -1                    # channel quads, views at least C wide
    assert call(sw=2, lwp=some.data_ptr()) == -1 and call(ti=some.data_ptr()) == -1          # line widths need OW = W; ragged rows N = H = KH = 1
    torch.cuda.synchronize()
    assert bool(torch.isnan(yv.owned()).all())
    yv.assert_outside_untouched("bad arguments")


def _child(mode):
    env = {k: v for k, v in os.environ.items() if k not in ("RD_DW_LDS", "RD_DW_COL", "RD_DW_DBG", "RD_DW_GPL", "RD_DW3_TW", "RD_DW5_TW", "RD_DW7_TW")}
    env.update({"lds_off": {"RD_DW_LDS": "0"}, "col": {"RD_DW_COL": "1"}, "tw": {"RD_DW3_TW": "4", "RD_DW5_TW": "4", "RD_DW7_TW": "8"}}[mode])
    r = subprocess.run([sys.executable, __file__, mode], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-2500:])
    return r.stdout


def test_lds_geometries_on_the_register_kernels_under_rd_dw_lds_0():
    out = _child("lds_off")
    assert out.count("route tiled") == len(LDS_GEOMETRIES)


def test_column_kernel_under_rd_dw_col_1():
    out = _child("col")
    assert out.count("route col") == len(COL_CASES)


def test_the_other_tile_widths_under_rd_dw_tw():
    out = _child("tw")
    assert out.count("route tiled") == len(TW_CASES)


if __name__ == "__main__":
    todo = {"lds_off": [({**cs, "route": tiled, "why": "RD_DW_LDS=0, by default " + name}) for cs, name, tiled in LDS_GEOMETRIES], "col": COL_CASES,
            "tw": TW_CASES}[sys.argv[1]]
    for j, cs_ in enumerate(todo):
        seed_ = {"lds_off": 200, "col": 300, "tw": 400}[sys.argv[1]] + j
        print("route %s chunks %d ratio %.3f SE %s" % run_case(cs_, seed_))
