"""Shared by tests/test_gpu_conv_tiles.py, test_gpu_gemm_dma.py and test_gpu_skinny_gemm.py: one dense convolution through the developer
entry rd_debug_conv_ex on strided views inside sentinel-filled buffers (glue_helpers.View), its fp64 reference and its per-element bound.

Bound of an output element with S = sum_k |x_k w_k| + |bias| (docs/notebook/conv_tile_kernels.md):
  fp32 path   (K + 3) 2^-24 S
  split path  sum_k (|w_k| e(x_k) + |x_k| e(w_k) + 2^-22 |x_k w_k|) + (K + 3) 2^-24 S,  e(v) = max(2^-22 |v|, 2^-36)
              (csrc/kernels_conv_h3.hip: |x - hi - lo 2^-11| <= 2^-22 |x|, floor = 2^-11 times half an fp16 subnormal step)
times the activation's Lipschitz constant; GELU, SiLU and sigmoid add the yardstick term of glue_helpers (4 x the error of the same formula
in torch fp32 on the CPU + 4 * 2^-24 * max|ref|), GELU also 0.5 |v| 1.5e-7 (rd_gelu's erf, csrc/rd_device.h); a residual adds 2^-24 |res|."""
import ctypes as C

import torch

from glue_helpers import U, View, lib

F = torch.nn.functional
NONE, RELU, GELU, SILU, SIGMOID, HSIG, HSIG_PADDLE = range(7)
OUT_NHWC, OUT_DECONV2X2 = 0, 1
IMG_H1, IMG_3X3, IMG_9X9 = 2, 4, 8                  # rd_debug_conv_ex's `images` bits
LIPSCHITZ = {NONE: 1.0, RELU: 1.0, GELU: 1.13, SILU: 1.1, SIGMOID: 0.25, HSIG: 1.0 / 6.0, HSIG_PADDLE: 0.2}
F32_TILES = ["128x32", "128x64", "128x96", "128x128"]
H3_TILES = ["256x128", "128x96", "256x64", "128x32", "128x64"]


def tile_dims(name):
    bm, bn = name.split("x")
    return int(bm), int(bn)


def activation(v, act):
    """the epilogue's activation on a tensor of either precision, by torch's own formulas"""
    if act == RELU:
        return v.clamp_min(0)
    if act == GELU:
        return F.gelu(v)
    if act == SILU:
        return F.silu(v)
    if act == SIGMOID:
        return torch.sigmoid(v)
    if act == HSIG:
        return (v / 6 + 0.5).clamp(0, 1)
    if act == HSIG_PADDLE:
        return (0.2 * v + 0.5).clamp(0, 1)
    return v


def split_err(v):
    return torch.maximum(v.abs() * 2.0 ** -22, torch.full_like(v, 2.0 ** -36))


def case(n, h, w, cin, cout, k=(1, 1), s=(1, 1), pad=(0, 0, 0, 0), act=NONE, res=False, bias=True, x_slot=None, y_slot=None, r_slot=None, deconv=False,
         x_range=1.0, why=""):
    """k = (KH, KW), s = (SH, SW), pad = (PT, PL, PB, PR); *_slot = (ld, offset) of the view inside a wider buffer; deconv: the 2x2 / stride-2
    transposed convolution (w in the checkpoint layout, a channel scale and shift standing in for the BatchNorm fold)"""
    return dict(n=n, h=h, w=w, cin=cin, cout=cout, k=k, s=s, pad=pad, act=act, res=res, bias=bias, x_slot=x_slot, y_slot=y_slot, r_slot=r_slot,
                deconv=deconv, x_range=x_range, why=why)


def pointwise(m, k, n, **kw):
    """a 1 x 1 convolution over m rows: [1][1][m][k] -> [1][1][m][n]"""
    return case(1, 1, m, k, n, **kw)


class Problem:
    """The operands of a case from a seeded CPU generator (x in [-x_range, x_range], w in [-0.1, 0.1], bias and res in [-0.5, 0.5]), the fp64
    reference on those fp32 values and the two bounds.  Built once per geometry and shared by the launches that run it."""

    def __init__(self, cs, seed):
        self.cs = cs
        n, h, w, cin, cout = cs["n"], cs["h"], cs["w"], cs["cin"], cs["cout"]
        (kh, kw), (sh, sw), (pt, pl, pb, pr) = cs["k"], cs["s"], cs["pad"]
        g = torch.Generator().manual_seed(seed)
        self.x = (torch.rand((n, h, w, cin), generator=g) * 2 - 1) * cs["x_range"]
        act = cs["act"]
        if cs["deconv"]:
            assert (kh, kw, sh, sw) == (1, 1, 1, 1) and not cs["res"]
            self.oh, self.ow, self.yh, self.yw, self.K = h, w, 2 * h, 2 * w, cin
            self.w_ck = (torch.rand((cin, cout, 2, 2), generator=g) - 0.5) * 0.2       # nn.ConvTranspose2d's [Cin][Cout][2][2]
            self.b_ck = (torch.rand((cout,), generator=g) - 0.5) if cs["bias"] else None
            self.scale = torch.rand((cout,), generator=g) + 0.5
            self.shift = torch.rand((cout,), generator=g) - 0.5
            wf = self.w_ck * self.scale.view(1, -1, 1, 1)                                # the fold, in fp32 as the engine does it
            bf = (self.b_ck * self.scale if self.b_ck is not None else torch.zeros(cout)) + self.shift
            self.w_dev_src = self.w_ck
            lin = lambda xx, ww: F.conv_transpose2d(xx.permute(0, 3, 1, 2), ww, None, stride=2).permute(0, 2, 3, 1)
            self.transposed = lin(self.x.double(), wf.double().transpose(2, 3)) + bf.double()
        else:
            self.oh, self.ow = (h + pt + pb - kh) // sh + 1, (w + pl + pr - kw) // sw + 1
            self.yh, self.yw, self.K = self.oh, self.ow, kh * kw * cin
            w_oihw = (torch.rand((cout, cin, kh, kw), generator=g) - 0.5) * 0.2
            wf = w_oihw
            bf = (torch.rand((cout,), generator=g) - 0.5) if cs["bias"] else None
            self.w_dev_src = w_oihw.permute(0, 2, 3, 1).reshape(cout, self.K).contiguous()       # k = (kh * KW + kw) * Cin + ci
            self.b_ck = bf
            lin = lambda xx, ww: F.conv2d(F.pad(xx.permute(0, 3, 1, 2), (pl, pr, pt, pb)), ww, None, stride=(sh, sw)).permute(0, 2, 3, 1)
        self.rows = n * self.yh * self.yw
        self.res = (torch.rand((self.rows, cout), generator=g) - 0.5) if cs["res"] else None
        xd, wd = self.x.double(), wf.double()
        bd = bf.double() if bf is not None else torch.zeros(cout, dtype=torch.float64)
        pre = (lin(xd, wd) + bd).reshape(self.rows, cout)
        s_mag = (lin(xd.abs(), wd.abs()) + bd.abs()).reshape(self.rows, cout)
        split_terms = (lin(split_err(xd), wd.abs()) + lin(xd.abs(), split_err(wd)) + 2.0 ** -22 * lin(xd.abs(), wd.abs())).reshape(self.rows, cout)
        self.pre = pre
        self.ref = activation(pre, act)
        extra = torch.zeros_like(pre)
        if act in (GELU, SILU, SIGMOID):
            yard = activation(pre.float(), act).double()
            extra = extra + 4.0 * float((yard - self.ref).abs().max()) + 4.0 * U * float(self.ref.abs().max())
        if act == GELU:
            extra = extra + 0.5 * pre.abs() * 1.5e-7
        if self.res is not None:
            self.ref = self.ref + self.res.double()
            extra = extra + U * self.res.double().abs()
        acc = (self.K + 3) * U * s_mag
        self.bound_f32 = LIPSCHITZ[act] * acc + extra
        self.bound_split = LIPSCHITZ[act] * (split_terms + acc) + extra
        if cs["deconv"]:
            self.transposed = activation(self.transposed.reshape(self.rows, cout), act)

    def bound(self, split):
        return self.bound_split if split else self.bound_f32


class Launch:
    """the result of one rd_debug_conv_ex call on fresh views: ms, route, flag, the output view's contents and the views themselves"""


def launch(pb, split, force=None, images=0, allow_skinny=0, ln=None, ascale=None, x_fill=None, x_poke=None, overrides=None):
    """One launch of problem `pb` on fresh sentinel-filled views.  x_fill: a finite value for the x buffer's words outside the view (default:
    the sentinel); x_poke = (row, column, value) written into the view of x before the launch; overrides: entry arguments to falsify
    (xld, cin, rld, ...) for the refusal tests."""
    cs = pb.cs
    n, h, w, cin, cout = cs["n"], cs["h"], cs["w"], cs["cin"], cs["cout"]
    (kh, kw), (sh, sw), (pt, pl, pb_, pr) = cs["k"], cs["s"], cs["pad"]
    xs, ys, rs = cs["x_slot"] or (cin, 0), cs["y_slot"] or (cout, 0), cs["r_slot"] or (cout, 0)
    x = pb.x.reshape(n * h * w, cin)
    if x_poke is not None:
        x = x.clone()
        x[x_poke[0], x_poke[1]] = x_poke[2]
    xv = View(n * h * w, cin, xs[0], xs[1], data=x)
    if x_fill is not None:
        own = xv.owned()
        xv.buf.fill_(x_fill)
        xv.buf[xv.guard:xv.guard + xv.rows, xv.off:xv.off + xv.c] = own.cuda()
        xv.before = xv.buf.clone()
    yv = View(pb.rows, cout, ys[0], ys[1])
    rv = View(pb.rows, cout, rs[0], rs[1], data=pb.res) if pb.res is not None else None
    keep = [pb.w_dev_src.cuda()]
    opt = {}
    for key, t in (("bias", pb.b_ck), ("scale", getattr(pb, "scale", None) if cs["deconv"] else None),
                   ("shift", getattr(pb, "shift", None) if cs["deconv"] else None), ("ln_g", ln[0] if ln else None), ("ln_b", ln[1] if ln else None),
                   ("ascale", ascale)):
        opt[key] = None
        if t is not None:
            keep.append(t.float().cuda())
            opt[key] = keep[-1].data_ptr()
    a = dict(N=n, H=h, W=w, Cin=cin, Cout=cout, KH=kh, KW=kw, SH=sh, SW=sw, PT=pt, PL=pl, PB=pb_, PR=pr, act=cs["act"], xld=xs[0], yld=ys[0], rld=rs[0],
             out_mode=OUT_DECONV2X2 if cs["deconv"] else OUT_NHWC, split=int(split), images=images, allow_skinny=allow_skinny, iters=0, res=rv.ptr if rv else None)
    a.update(overrides or {})
    name, flag = C.create_string_buffer(32), C.c_int(-7)
    ms = lib().rd_debug_conv_ex(a["N"], a["H"], a["W"], a["Cin"], a["Cout"], a["KH"], a["KW"], a["SH"], a["SW"], a["PT"], a["PL"], a["PB"], a["PR"], a["act"],
                                a["xld"], a["yld"], a["rld"], a["out_mode"], a["split"], a["images"], a["allow_skinny"], a["iters"], xv.ptr,
                                keep[0].data_ptr(), opt["bias"], a["res"], yv.ptr, opt["scale"], opt["shift"], opt["ln_g"], opt["ln_b"], opt["ascale"],
                                force.encode() if force else None, name, 32, C.byref(flag))
    torch.cuda.synchronize()
    r = Launch()
    r.ms, r.route, r.flag, r.xv, r.yv, r.rv, r.y = ms, name.value.decode(), flag.value, xv, yv, rv, yv.owned()
    return r


def check_launch(pb, r, split, route, tag, flag=0, bound=None):
    """The common form: the entry ran, on `route`; the range flag; the view is finite and every element inside its own bound; nothing outside the
    view was written; the inputs are unchanged.  Returns the worst error / bound."""
    assert r.ms >= 0, (tag, "the entry declined or the launcher threw", r.ms)
    assert r.route == route, (tag, "ran on", r.route, "expected", route)
    assert r.flag == flag, (tag, "range flag", r.flag)
    r.yv.assert_outside_untouched(tag)
    r.xv.assert_unchanged(tag)
    if r.rv is not None:
        r.rv.assert_unchanged(tag)
    assert bool(torch.isfinite(r.y).all()), (tag, "not finite: rows", torch.nonzero(~torch.isfinite(r.y))[:8].tolist())
    err = (r.y.double() - pb.ref).abs()
    bound = pb.bound(split) if bound is None else bound
    ratio = err / bound.clamp_min(1e-300)
    worst = float(ratio.max())
    print(f"{tag} [{route}]: max err {float(err.max()):.3e} worst err/bound {worst:.3f}")
    if worst > 1.0:
        bad = torch.nonzero(ratio > 1.0)
        at = [(int(i), int(j), float(err[i, j]), float(bound[i, j])) for i, j in bad[:8].tolist()]
        raise AssertionError((tag, route, "%d elements beyond their bound; (row, column, err, bound):" % len(bad), at))
    return worst


def check_class_bound(pb, r, tag):
    """long-K cases: the class bound of test_direct_conv_matches_fp64 on top of the per-element one"""
    err = float((r.y.double() - pb.ref).abs().max())
    assert err < 2e-5 * max(1.0, float(pb.ref.abs().max())), (tag, err)


def bit_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def assert_bit_identical(a, b, tag):
    """two outputs of the same problem: which elements differ, and by how much"""
    a, b = a.contiguous(), b.contiguous()
    if not bit_equal(a, b):
        d = torch.nonzero(a.view(torch.int32) != b.view(torch.int32))
        at = [(int(i), int(j), float(a[i, j]), float(b[i, j])) for i, j in d[:8].tolist()]
        raise AssertionError((tag, "%d elements differ; (row, column, a, b):" % len(d), at, "max |a - b|", float((a.double() - b.double()).abs().max())))
