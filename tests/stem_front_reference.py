"""The stem front (csrc/kernels_stem_fused.hip; rec_lcnetv4.py:148-169, rec_pphgnetv2.py StemBlock) restated on the CPU: its operands from a
seeded generator, the float64 reference, the per-element error bound of the split-fp16 kernel, and a torch emulation of the kernel's arithmetic
with switches for the ways such a kernel goes wrong.  Shared by tests/test_stem_front_reference.py (CPU) and tests/test_gpu_stem_front.py.

    e = relu(conv3x3 s2 p1 (x))            a = relu(conv2x2 (pad_rb(e)))            b = relu(conv2x2 (pad_rb(a)))
    p = max_pool2d(pad_rb(e), 2, 1)        cat = [p | b]                            pad_rb = F.pad(., (0, 1, 0, 1))

(in_ch == 1 repeats the plane).  With a line table, image n is computed on x[n, :, :, :w_in] alone and cat is zero at columns >= w2.

THE BOUND, from the arithmetic the kernel's header states (nothing here is a measured error).  One product of the kernel is

    y = ((b s + sum_k xh_k Wh_k) + sum_k (xh_k Wl_k + xl_k Wh_k)) / s          two fp32 accumulators on the matrix cores, K_pad slots each

with x = xh + xl + dx, w s = Wh + Wl + dW, s the matrix's power of two (max |w| s in [2^13, 2^14)), 1 / s exact.
  * activations: xh = fp16(x), xl = fp16(x - xh) UNSCALED, fp16 subnormals kept: |dx| <= 2^-22 |x| where xl is a normal fp16 number (it has
    11 bits below xh's 11), an absolute 2^-25 (half a subnormal step) where it is not: |dx| <= 2^-22 |x| + 2^-25.
  * weights: |dW| <= 2^-22 |w s| where Wl is normal - the pre-scale makes that so for every weight within 2^-16 of the matrix's largest; below,
    half a subnormal step of the scaled plane: 2^-25 / s <= 2^-38 max |w|.  |dw| <= 2^-22 |w| + 2^-38 max |w|.
  * the dropped product: |xl Wl| <= 2^-11 |x| 2^-11 |w s| = 2^-22 |x w s|.
  * accumulation: fp32, K_pad products + the bias in the first accumulator, one addition of the two, the same (K + 3) 2^-24 S the dense-conv
    tests use for a K-term fp32 sum on the matrix cores (tests/conv_helpers.py), with K_pad = 48 (stem1: 3 kernel rows x 16 slots), 4 C1
    (stem2a), 4 CB (stem2b; CB = C1 / 2 rounded up to 8); padded slots multiply by zero, counting them only loosens the bound.
Per product, with S = |b| + sum_k |x_k| |w_k| over the taps inside the map:

    own(y) <= c_K S + 2^-25 sum_k |w_k| + 2^-38 max |w| sum_k |x_k|,        c_K = 3 * 2^-22 + (K_pad + 3) 2^-24

and an operand that itself carries an error d(x) (e into stem2a and the pool, a into stem2b) adds sum_k d(x_k) |w_k| and enters S as
|x| + d(x).  ReLU and max have Lipschitz constant 1, so the bounds go e -> a -> b and e -> p through absolute-value convolutions / a max-pool
of the bound, all in float64; a last factor 1 + 2^-9 pays for the second-order terms (|xh| <= (1 + 2^-11) |x| and the like).
The fp32 kernel of route 0 (stem_conv3x3s2_kernel, one fma chain of K = 27 behind the bias): (27 + 3) 2^-24 S."""
import math

import torch

F = torch.nn.functional
U = 2.0 ** -24
INSTANCES = (24, 32, 48)
TILE_H, TILE_W = 8, 32                 # a cat tile; "inner" when ty0 + 10 <= H2 and tx0 + 34 <= W2n

# (N, H, W): what each covers is the table of the issue / docs/notebook/stem_front_kernel.md
SHAPES = {
    "inner_cut_right_bottom": (2, 48, 160),     # cat 24 x 80: inner tiles, a cut right tile, a bottom tile row that is never inner
    "odd_narrow": (2, 37, 45),                  # cat 19 x 23: odd sizes, narrower than a tile, a 3-row bottom tile
    "one_exact_tile": (1, 16, 64),              # cat 8 x 32: all halo is padding
    "one_row_one_col_edge": (1, 18, 130),       # cat 9 x 65: a one-row and a one-column edge tile
    "tiny_3x5": (5, 3, 5),                      # cat 2 x 3
    "tiny_1x1": (5, 1, 1),                      # cat 1 x 1
}
PARITY_SHAPES = {"even_h_odd_w": (1, 16, 67), "odd_h_even_w": (1, 17, 66)}      # the last input row / column is or is not read
PERSISTENT = (40, 48, 320)                      # 600 tiles on 256 CUs: workgroups run 2 and 3 tiles
LINES_HW = (48, 160)


def line_widths(W):
    return [W, W - 1, 77, 16, 2, 1]


def gpu_cases():
    """Every launch tests/test_gpu_stem_front.py compares with float64: (tag, Case arguments, line widths or None, (yld, channel offset) or
    None for a dense buffer).  tests/test_stem_front_reference.py runs the emulated kernel and its mutants on the same operands."""
    out = []
    for c1 in INSTANCES:
        for i, (name, (n, h, w)) in enumerate(SHAPES.items()):
            out.append((f"C{c1}_{name}", dict(N=n, H=h, W=w, C1=c1, seed=i), None, None))
    for i, (name, (n, h, w)) in enumerate(PARITY_SHAPES.items()):
        out.append((f"C32_{name}", dict(N=n, H=h, W=w, C1=32, seed=10 + i), None, None))
    out.append(("C32_grey", dict(N=2, H=37, W=45, C1=32, in_ch=1, seed=20), None, None))
    out.append(("C24_yld72", dict(N=2, H=48, W=160, C1=24, seed=21), None, (2 * 24 + 24, 8)))
    out.append(("C32_yld384", dict(N=1, H=18, W=130, C1=32, seed=22), None, (384, 0)))
    for c1 in INSTANCES:
        for which in ("e", "a"):
            out.append((f"C{c1}_coherent_{which}", dict(N=1, H=18, W=130, C1=c1, seed=50, coherent=which), None, None))
    for c1 in INSTANCES:
        n, h, w = PERSISTENT
        out.append((f"C{c1}_persistent", dict(N=n, H=h, W=w, C1=c1, seed=30), None, None))
        h, w = LINES_HW
        out.append((f"C{c1}_lines", dict(N=len(line_widths(w)), H=h, W=w, C1=c1, seed=40), line_widths(w), None))
    return out


def build_case(kw, widths):
    case = Case(**kw)
    return zero_beyond_widths(case, widths) if widths is not None else case


def pad_rb(t):
    return F.pad(t, (0, 1, 0, 1))


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


class Case:
    """x uniform in [-1, 1]; weights uniform in +-0.1 times per-output-channel magnitudes spread over logspace(-2, 0.5); biases in
    [-0.12, 0.18]: the small channels are all-zero or all-positive, the large ones mix, a real share of ReLU zeros over all."""

    def __init__(self, N, H, W, C1, in_ch=3, seed=0, coherent=None):
        self.N, self.H, self.W, self.C1, self.in_ch, self.NA = N, H, W, C1, in_ch, C1 // 2
        self.CB = (self.NA + 7) // 8 * 8
        g = torch.Generator().manual_seed(1000 * seed + 7 * C1 + in_ch)

        def weight(co, ci, k):
            w = (torch.rand((co, ci, k, k), generator=g) - 0.5) * 0.2
            return w * torch.logspace(-2, 0.5, co)[torch.randperm(co, generator=g)][:, None, None, None]

        self.w1, self.w2a, self.w2b = weight(C1, 3, 3), weight(self.NA, C1, 2), weight(C1, self.NA, 2)
        self.b1, self.b2a, self.b2b = ((torch.rand((c,), generator=g) - 0.4) * 0.3 for c in (C1, self.NA, C1))
        self.x = torch.rand((N, in_ch, H, W), generator=g) * 2 - 1
        # Coherent low planes.  On random operands the low planes' signs are random and a missing lo(x) * hi(w) product of a long-K
        # convolution is a 2^-12 S / sqrt(K) random walk, below any worst-case accumulation bound at K = 192.  Here the operand of one
        # product is the same value h + 0.45 ulp_fp16(h) at every pixel (the previous layer: zero weights, that bias) and the product's
        # weights are non-negative: every low plane is +0.45 ulp and the missing product is a coherent ~2^-12 S.
        if coherent is not None:
            low = lambda c: (1 + torch.rand((c,), generator=g)).half().float() + 0.45 * 2.0 ** -10
            if coherent == "e":
                self.w1.zero_()
                self.b1, self.w2a = low(C1), self.w2a.abs()
            else:
                assert coherent == "a"
                self.w2a.zero_()
                self.b2a, self.w2b = low(self.NA), self.w2b.abs()

    def clone(self):
        c = Case.__new__(Case)
        c.__dict__.update({k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.__dict__.items()})
        return c

    # the layouts rd_debug_stem_front takes
    def w1_stem(self):
        return self.w1.permute(2, 3, 1, 0).reshape(27, self.C1).contiguous()              # row (kh * 3 + kw) * 3 + ci, co fastest

    def w2a_folded(self):
        return self.w2a.permute(0, 2, 3, 1).reshape(self.NA, 4 * self.C1).contiguous()   # k = tap * C1 + c, tap = dy * 2 + dx

    def w2b_folded(self):
        return self.w2b.permute(0, 2, 3, 1).reshape(self.C1, 4 * self.NA).contiguous()

    def x3(self, x=None):
        x = self.x if x is None else x
        return x.expand(-1, 3, -1, -1) if self.in_ch == 1 else x


def zero_beyond_widths(case, widths):
    """the line table's contract: columns >= w_in of image n are zero"""
    for n, w_in in enumerate(widths):
        case.x[n, :, :, w_in:] = 0
    return case


def line_table(widths):
    """int32 [N][4] (csrc/rd_kernels.h LineTab): w_in, w2, w4, first token"""
    rows, tok = [], 0
    for w_in in widths:
        w2 = (w_in - 1) // 2 + 1
        w4 = (w2 - 1) // 2 + 1
        rows.append([w_in, w2, w4, tok])
        tok += w4 // 2
    return torch.tensor(rows, dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------- float64 reference and bound
def _front64(case, x):
    d = lambda t: t.double()
    e = F.relu(F.conv2d(d(case.x3(x)), d(case.w1), d(case.b1), stride=2, padding=1))
    a = F.relu(F.conv2d(pad_rb(e), d(case.w2a), d(case.b2a)))
    b = F.relu(F.conv2d(pad_rb(a), d(case.w2b), d(case.b2b)))
    p = F.max_pool2d(pad_rb(e), 2, 1)
    return e, a, b, p


def _c(kpad):
    return 3 * 2.0 ** -22 + (kpad + 3) * U


def _product_bound(lin, xa, xerr, w, b, kpad):
    """lin(t, weight): the convolution's linear map with its zero padding, no bias.  xa = |operand| in float64, xerr = its own bound."""
    aw = w.double().abs()
    xin = xa + xerr
    S = lin(xin, aw) + b.double().abs().view(1, -1, 1, 1)
    own = _c(kpad) * S + 2.0 ** -25 * lin(torch.ones_like(xa), aw) + 2.0 ** -38 * float(aw.max()) * lin(xin, torch.ones_like(aw))
    return (own + lin(xerr, aw)) * (1 + 2.0 ** -9)


def _bounds64(case, x, e, a):
    lin1 = lambda t, w: F.conv2d(t, w, None, stride=2, padding=1)
    lin2 = lambda t, w: F.conv2d(pad_rb(t), w)
    xa = case.x3(x).double().abs()
    be = _product_bound(lin1, xa, torch.zeros_like(xa), case.w1, case.b1, 48)
    ba = _product_bound(lin2, e, be, case.w2a, case.b2a, 4 * case.C1)
    bb = _product_bound(lin2, a, ba, case.w2b, case.b2b, 4 * case.CB)
    bp = F.max_pool2d(pad_rb(be), 2, 1)
    return be, ba, bb, bp


def bound_route0(case):
    """stem_conv3x3s2_kernel: e NHWC and its fp32 bound"""
    e = _front64(case, case.x)[0]
    S = F.conv2d(case.x3().double().abs(), case.w1.double().abs(), case.b1.double().abs(), stride=2, padding=1)
    return e.permute(0, 2, 3, 1).contiguous(), ((27 + 3) * U * S).permute(0, 2, 3, 1).contiguous()


class Reference:
    """cat and its bound, NHWC float64 [N][H2][W2][2 C1] (p at channel 0, b at channel C1); e / a and their bounds (NCHW) without a line table"""

    def __init__(self, case, widths=None):
        H2, W2 = out_hw(case.H, case.W)
        if widths is None:
            e, a, b, p = _front64(case, case.x)
            be, ba, bb, bp = _bounds64(case, case.x, e, a)
            self.e, self.a, self.e_bound, self.a_bound = e, a, be, ba
            cat, bound = torch.cat([p, b], 1), torch.cat([bp, bb], 1)
        else:
            cat = torch.zeros((case.N, 2 * case.C1, H2, W2), dtype=torch.float64)
            bound = torch.zeros_like(cat)
            for n, w_in in enumerate(widths):
                x = case.x[n:n + 1, :, :, :w_in]
                e, a, b, p = _front64(case, x)
                be, ba, bb, bp = _bounds64(case, x, e, a)
                cat[n, :, :, :e.shape[3]] = torch.cat([p, b], 1)[0]
                bound[n, :, :, :e.shape[3]] = torch.cat([bp, bb], 1)[0]
        self.cat, self.bound = cat.permute(0, 2, 3, 1).contiguous(), bound.permute(0, 2, 3, 1).contiguous()


# -------------------------------------------------------------------------------------------------- the kernel's arithmetic, emulated in torch
MUTANTS = ("drop_lo_hi_stem1", "drop_lo_hi_stem2a", "drop_lo_hi_stem2b", "drop_lo_hi", "stem2a_tap_shifted", "e_map_halo_kept", "line_halo_kept",
           "a_pad_nonzero", "a_pad_nonzero_w_pad_nonzero", "n_block_row_stem1", "n_block_row_stem2b")


def split16(v):
    """fp32 -> (hi, lo) fp16 values held in fp32: hi = fp16(v), lo = fp16(v - hi), subnormals kept"""
    hi = v.half().float()
    return hi, (v - hi).half().float()


def weight_planes(w):
    """[Cout][K] fp32 -> (hi, lo, s): one power-of-two scale per matrix with max |w| s in [2^13, 2^14) (csrc/rd_host.h rd_pow2_exp)"""
    mx = float(w.abs().max())
    ex = 14 - math.frexp(mx)[1] if mx > 0 else 0
    hi, lo = split16(torch.ldexp(w, torch.tensor(ex)))
    return hi, lo, 2.0 ** ex


def _product(A, w, b, drop_lo_hi=False):
    """A [M][K] fp32, w [Cout][K], b [Cout] -> [M][Cout]: three fp32-accumulated products of fp16 planes, the bias in the first accumulator"""
    wh, wl, s = weight_planes(w)
    ah, al = split16(A)
    acc1 = ah @ wh.t() + b * s
    acc2 = ah @ wl.t()
    if not drop_lo_hi:
        acc2 = acc2 + al @ wh.t()
    return (acc1 + acc2) * (1.0 / s)


def _taps2x2(t, oh, ow, shift_tap1=False):
    """[N][C][>= oh + 1][>= ow + 2] -> [N oh ow][4 C], k = tap * C + c"""
    taps = []
    for dy in (0, 1):
        for dx in (0, 1):
            dxx = dx + 1 if (shift_tap1 and dy == 0 and dx == 1) else dx
            taps.append(t[:, :, dy:dy + oh, dxx:dxx + ow])
    return torch.cat(taps, 1).permute(0, 2, 3, 1).reshape(-1, 4 * t.shape[1])


def emulate(case, widths=None, mutant=None):
    """cat NHWC fp32 [N][H2][W2][2 C1] the way the kernel computes it: e and a on the tile's halo (one row / column beyond the map, from the
    zero-padded image), zeroed beyond the map and beyond a line's own width, a's channels padded to CB, stem2b over 4 CB slots whose pad
    weights are zero.  `mutant`: one of MUTANTS, a kernel that is wrong in that way."""
    assert mutant is None or mutant in MUTANTS
    N, C1, NA, CB = case.N, case.C1, case.NA, case.CB
    H2, W2 = out_hw(case.H, case.W)
    w2n = torch.tensor([W2 if widths is None else min(W2, (w - 1) // 2 + 1) for w in (widths or [0] * N)])
    drop = lambda which: mutant in ("drop_lo_hi", "drop_lo_hi_" + which)

    def keep(t, map_edge, line_edge):
        """zero t [N][C][h][w] at rows >= H2 / columns >= W2 (map_edge) and at columns in [w2n, W2) (line_edge)"""
        h, w = t.shape[2:]
        rows, cols = torch.arange(h).view(1, 1, h, 1), torch.arange(w).view(1, 1, 1, w)
        m = torch.ones((N, 1, h, w), dtype=torch.bool)
        if map_edge:
            m = m & (rows < H2) & (cols < W2)
        if line_edge:
            m = m & ((cols < w2n.view(N, 1, 1, 1)) | (cols >= W2))
        return t * m

    # stem1 on [H2 + 2][W2 + 3] e pixels (the halo, + one column for the shifted-tap mutant), K = 27
    eh, ew = H2 + 2, W2 + 3
    xp = F.pad(case.x3().float(), (1, 2 * ew - case.W, 1, 2 * eh - case.H))      # 2 eh + 1 rows, 2 ew + 1 columns
    A = F.unfold(xp, 3, stride=2).transpose(1, 2).reshape(-1, 27)               # [N eh ew][27], k = ci * 9 + kh * 3 + kw
    e = F.relu(_product(A, case.w1.reshape(C1, 27), case.b1, drop("stem1")))
    if mutant == "n_block_row_stem1" and C1 > 32:
        e[:, 32:] = e[:, C1 - 1:C1]
    e = e.reshape(N, eh, ew, C1).permute(0, 3, 1, 2)
    e = keep(e, mutant != "e_map_halo_kept", mutant != "line_halo_kept")

    # stem2a on [H2 + 1][W2 + 1] a pixels, K = 4 C1
    ah, aw = H2 + 1, W2 + 1
    a = F.relu(_product(_taps2x2(e, ah, aw, mutant == "stem2a_tap_shifted"), case.w2a_folded(), case.b2a, drop("stem2a")))
    a = a.reshape(N, ah, aw, NA).permute(0, 3, 1, 2)
    pad_ch = a[:, NA - 1:NA].expand(-1, CB - NA, -1, -1) if mutant in ("a_pad_nonzero", "a_pad_nonzero_w_pad_nonzero") else torch.zeros((N, CB - NA, ah, aw))
    a = keep(torch.cat([a, pad_ch], 1), True, mutant != "line_halo_kept")

    # stem2b on the map, K = 4 CB with the weight rows padded per tap
    w2b = torch.zeros((C1, 4, CB))
    w2b[:, :, :NA] = case.w2b_folded().reshape(C1, 4, NA)
    if mutant == "a_pad_nonzero_w_pad_nonzero":
        w2b[:, :, NA:] = w2b[:, :, NA - 1:NA]
    b = F.relu(_product(_taps2x2(a, H2, W2), w2b.reshape(C1, 4 * CB), case.b2b, drop("stem2b")))
    if mutant == "n_block_row_stem2b" and C1 > 32:
        b[:, 32:] = b[:, C1 - 1:C1]
    b = b.reshape(N, H2, W2, C1).permute(0, 3, 1, 2)
    b = keep(b, True, True)
    p = F.max_pool2d(e[:, :, :H2 + 1, :W2 + 1], 2, 1)
    return torch.cat([p, b], 1).permute(0, 2, 3, 1).contiguous()
