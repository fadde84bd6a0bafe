"""GPU: the fused CTC head (csrc/kernels_ctc.hip: `ctc_head_kernel` on the fp32 matrix cores, `ctc_head_h3_kernel` on split fp16, and
`ctc_merge_kernel` over the class splits) alone against fp64 through the developer entry `rd_debug_ctc_head`: dictionaries from 1 class to
PP-OCRv6's 18710, token counts around the 32 / 128 / 256 token tiles, a row stride wider than K, flat to peaked logits, forced split counts
(empty splits included), winners planted at the first / last class, at split borders and in front of a partial tail tile, and exact ties
whose two classes sit in different lane halves, register slices, class tiles and class splits (the lowest class must win, as numpy's argmax
and the reference's `preds.argmax(axis=2)`).

Reference: fp64 logits x @ W^T + b, their argmax and largest softmax value.  With d = 2e-6 max|logit| (the split kernels' bound of
tests/test_gpu_gemm_h1.py, used for both routes):
  index        the fp64 logit of the chosen class is within 2 d of the row maximum, for every token; the index is the fp64 argmax wherever
               the fp64 top-2 gap exceeds 2 d;
  probability  |prob - ref| <= 2 d p (1 - p) + 2^-20 p  (a logit perturbation of +-d moves 1 / sum exp by at most the first term; the
               second covers fp32 summation over up to 18710 terms).
Measured maxima: docs/notebook/rec_tail_kernels.md."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 120
MS = [1, 31, 33, 255, 257, 300]
CS = [1, 3, 5, 40, 63, 65, 1279, 1281, 6625, 18385, 18710]
# every C with two of the Ms (and so every M several times), alternating the row stride; plus the 128-token tile edge of the fp32 kernel
SHAPES = [(MS[(i + j) % 6], c, 136 if (i + j) % 2 else 120) for i, c in enumerate(CS) for j in (0, 3)] + [(127, 65, 120), (129, 1281, 136)]


def _lib():
    from rapiddoc_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=4)
def _problem(M, Ccls, gain, seed=0):
    """Unit-scale inputs as tools/microbench.py:ctc (x in +-0.5, w in +-0.1, bias in +-0.5), weights and bias times `gain`.
    Returns (x [M][K], W' [C][128] with the bias in column K), both fp32 on the CPU.  Cached: both kernels see the same problem."""
    g = torch.Generator().manual_seed(seed + 7 * M + Ccls)
    x = torch.rand((M, K), generator=g) - 0.5
    wp = torch.zeros((Ccls, 128))
    wp[:, :K] = (torch.rand((Ccls, K), generator=g) - 0.5) * 0.2 * gain
    wp[:, K] = (torch.rand((Ccls,), generator=g) - 0.5) * gain
    return x, wp


def plant(x, wp, cls, tok, alpha=20.0):
    """Class `cls` becomes alpha x_tok / |x_tok|^2 with bias 0: its logit is alpha for token `tok`."""
    wp[cls, :] = 0.0
    wp[cls, :K] = alpha * x[tok] / float(x[tok].double().pow(2).sum())


def run(x, wp, split, xld=K, nsplit=0):
    """One launch.  Returns (idx int64 [M], prob fp32 [M], split count used, range flag)."""
    M, Ccls = x.shape[0], wp.shape[0]
    xb = torch.full((M, xld), 1.0e3)                             # columns past K belong to nobody
    xb[:, :K] = x
    xd, wd = xb.cuda(), wp.cuda()
    hi = wd.half()
    lo = ((wd - hi.float()) * 2048.0).half()
    part = torch.zeros((M * 64 * 4,), device="cuda")
    idx = torch.full((M + 2,), -5, dtype=torch.int32, device="cuda")
    prob = torch.full((M + 2,), -5.0, device="cuda")
    ns, flag = C.c_int(0), C.c_int(-1)
    rc = _lib().rd_debug_ctc_head(M, K, Ccls, xd.data_ptr(), xld, wd.data_ptr(), hi.data_ptr() if split else None,
                                  lo.data_ptr() if split else None, part.data_ptr(), idx.data_ptr(), prob.data_ptr(), nsplit,
                                  C.byref(ns), C.byref(flag))
    assert rc == 0, rc
    idx, prob = idx.cpu(), prob.cpu()
    assert idx[M:].tolist() == [-5, -5] and prob[M:].tolist() == [-5.0, -5.0]      # nothing past the last token
    return idx[:M].long(), prob[:M], ns.value, flag.value


def check(x, wp, idx, prob, tag):
    """The bounds of the module docstring.  Returns (fp64 logits, d)."""
    M, Ccls = x.shape[0], wp.shape[0]
    lg = x.double() @ wp[:, :K].double().t() + wp[:, K].double()
    d = 2e-6 * float(lg.abs().max())
    assert bool(((idx >= 0) & (idx < Ccls)).all()), (tag, idx.min(), idx.max())
    assert bool(torch.isfinite(prob).all()), tag
    ref_idx = torch.from_numpy(np.argmax(lg.numpy(), axis=1))    # first index on ties
    top = lg.max(dim=1).values
    short = top - lg.gather(1, idx[:, None])[:, 0]               # how far the chosen class is below the row maximum
    if Ccls > 1:
        t2 = torch.topk(lg, 2, dim=1).values
        clear = (t2[:, 0] - t2[:, 1]) > 2 * d
    else:
        clear = torch.ones(M, dtype=torch.bool)
    p = torch.softmax(lg, dim=1).max(dim=1).values
    perr = (prob.double() - p).abs()
    pbound = 2 * d * p * (1 - p) + 2.0 ** -20 * p
    print(f"ctc {tag}: d {d:.2e} chosen-logit shortfall {float(short.max()):.2e} (2d = {2 * d:.2e}), clear tokens {int(clear.sum())}/{M}, "
          f"prob err / bound {float((perr / pbound).max()):.3f} (max err {float(perr.max()):.2e})")
    assert float(short.max()) <= 2 * d, (tag, float(short.max()), d)
    assert bool((idx == ref_idx)[clear].all()), (tag, int((idx != ref_idx)[clear].sum()))
    assert bool((perr <= pbound).all()), (tag, float((perr / pbound).max()))
    return lg, d


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "h3"])
@pytest.mark.parametrize("M,Ccls,xld", SHAPES, ids=lambda v: str(v))
def test_shapes_and_row_strides(M, Ccls, xld, split):
    x, wp = _problem(M, Ccls, 1.0)
    idx, prob, ns, flag = run(x, wp, split, xld=xld)
    assert flag == 0 and 1 <= ns <= 64
    check(x, wp, idx, prob, f"{'h3' if split else 'fp32'} M{M} C{Ccls} xld{xld} nsplit{ns}")


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "h3"])
@pytest.mark.parametrize("gain", [8.0, 30.0])
@pytest.mark.parametrize("M,Ccls", [(300, 6625), (257, 18710)])
def test_logit_gain(M, Ccls, gain, split):
    """x 8: moderately peaked rows; x 30: |logit| around 40, the range of the v5 server recogniser."""
    x, wp = _problem(M, Ccls, gain)
    idx, prob, ns, flag = run(x, wp, split)
    assert flag == 0
    lg, _d = check(x, wp, idx, prob, f"{'h3' if split else 'fp32'} M{M} C{Ccls} gain{gain:g}")
    assert float(lg.abs().max()) > (30.0 if gain == 30.0 else 8.0)


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "h3"])
@pytest.mark.parametrize("M,Ccls,nsplit", [(300, 40, 64), (257, 18710, 1), (257, 18710, 64)])
def test_forced_split_counts(M, Ccls, nsplit, split):
    """C = 40 over 64 splits: 10 splits own 4 classes each, 54 are empty (for every wavefront of the 256-token tile, the ones that run
    their statistics one tile late included).  C = 18710 in one split and in 64."""
    x, wp = _problem(M, Ccls, 1.0)
    idx, prob, ns, flag = run(x, wp, split, nsplit=nsplit)
    assert ns == nsplit and flag == 0
    check(x, wp, idx, prob, f"{'h3' if split else 'fp32'} M{M} C{Ccls} forced nsplit{nsplit}")
    idx1, prob1, _ns, _f = run(x, wp, split)                     # the natural split count picks the same classes
    assert torch.equal(idx, idx1)


def _classes_per_split(Ccls, ns):
    return ((Ccls + ns - 1) // ns + 3) // 4 * 4


TOKENS = [0, 31, 32, 255, 256, 299, 127, 128, 100, 200]


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "h3"])
@pytest.mark.parametrize("Ccls", [65, 6625, 18710])
def test_planted_winners_at_the_borders(Ccls, split):
    M = 300
    x, wp = _problem(M, Ccls, 1.0)
    wp = wp.clone()
    _i, _p, ns, _f = run(x, wp, split)
    cps = _classes_per_split(Ccls, ns)
    last_begin = (ns - 1) * cps                                  # the last split ends at C: its tail tile is partial unless it divides
    want = [0, Ccls - 1, cps - 1, cps]                           # first, last, last class of split 0, first of split 1
    for tile in (64, 128):                                       # class tiles of the split-fp16 / the fp32 kernel
        full = (Ccls - last_begin) // tile * tile
        if full and full != Ccls - last_begin:
            want.append(last_begin + full - 1)                   # the last class in front of a partial tail tile
    planted = sorted({c for c in want if 0 <= c < Ccls})
    owner = {c: TOKENS[i] for i, c in enumerate(planted)}
    for c, t in owner.items():
        plant(x, wp, c, t)
    idx, prob, ns2, flag = run(x, wp, split)
    assert ns2 == ns and flag == 0
    lg, d = check(x, wp, idx, prob, f"{'h3' if split else 'fp32'} C{Ccls} planted {planted}")
    for c, t in owner.items():
        assert float(lg[t, c]) - float(torch.cat([lg[t, :c], lg[t, c + 1:]]).max()) > 5.0      # a clear winner by construction
        assert int(idx[t]) == c, (c, t, int(idx[t]))


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "h3"])
@pytest.mark.parametrize("Ccls", [6625, 18710])
def test_exact_ties_go_to_the_lowest_class(Ccls, split):
    """c2 is a copy of the planted c1 (row and bias): equal logits to the last bit.  c2 - c1 = 1 (next register), 4 (other lane half),
    8 (next register group), 16 (next slice of 8), 32 (next MFMA tile), 64 / 128 (next class tile of the split / fp32 kernel), one split
    further, and the pair (0, C - 1).  Each pair is owned by a different token."""
    M = 300
    x, wp = _problem(M, Ccls, 1.0)
    wp = wp.clone()
    _i, _p, ns, _f = run(x, wp, split)
    cps = _classes_per_split(Ccls, ns)
    pairs = [(128 * (k + 1) + 1, 128 * (k + 1) + 1 + off) for k, off in enumerate((1, 4, 8, 16, 32, 64, 128))]
    pairs += [(5, 5 + cps), (0, Ccls - 1)]
    assert ns >= 2 and max(c for p in pairs[:7] for c in p) < cps and len({c for p in pairs for c in p}) == 2 * len(pairs)
    for (c1, c2), t in zip(pairs, TOKENS):
        plant(x, wp, c1, t)
        wp[c2] = wp[c1]
    idx, prob, _ns, flag = run(x, wp, split)
    assert flag == 0
    lg, d = check(x, wp, idx, prob, f"{'h3' if split else 'fp32'} C{Ccls} ties")
    for (c1, c2), t in zip(pairs, TOKENS):
        # (equal rows: the two fp64 logits differ by the reference GEMM's own blocking at most)
        assert abs(float(lg[t, c1]) - float(lg[t, c2])) < 1e-12 and float(lg[t].max()) - float(lg[t, c1]) < 1e-12
        assert int(idx[t]) == min(c1, c2), (c1, c2, t, int(idx[t]))
        assert abs(float(prob[t]) - 0.5) < 1e-3                  # (the bound itself was applied by check)
    # A planted row also scores several times the natural logits for tokens it was not made for, so most rows of this problem are led by a
    # twin pair: with the copies struck out, the index must be the argmax of what is left wherever that one is clear by 2 d.
    rest = lg.clone()
    rest[:, [c2 for _c1, c2 in pairs]] = float("-inf")
    t2 = torch.topk(rest, 2, dim=1).values
    clear = (t2[:, 0] - t2[:, 1]) > 2 * d
    assert int(clear.sum()) > 250
    assert bool((idx == rest.argmax(dim=1))[clear].all())


def test_an_activation_beyond_the_fp16_range_raises_the_range_flag():
    x, wp = _problem(257, 1281, 1.0)
    x = x.clone()
    x[200, 77] = 1.0e5
    _idx, _prob, _ns, flag = run(x, wp, True)
    assert flag == 1
    idx, prob, _ns, flag = run(x, wp, False)                     # the fp32 kernel converts nothing: no flag, and it computes
    assert flag == 0
    check(x, wp, idx, prob, "fp32 kernel, x = 1e5")


def test_shapes_the_kernels_do_not_take_are_refused():
    x, wp = _problem(4, 5, 1.0)
    xd, wd = x.cuda(), wp.cuda()
    part = torch.zeros(4 * 64 * 4, device="cuda")
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    prob = torch.zeros(4, device="cuda")
    lib = _lib()
    args = (xd.data_ptr(), K, wd.data_ptr(), None, None, part.data_ptr(), idx.data_ptr(), prob.data_ptr())
    assert lib.rd_debug_ctc_head(4, K, 5, *args, 0, None, None) == 0
    assert lib.rd_debug_ctc_head(4, K, 5, *args, 65, None, None) == -1                       # the workspace holds 64 splits
    assert lib.rd_debug_ctc_head(4, 128, 5, *args, 0, None, None) == -1                      # K < 128: the bias column
    assert lib.rd_debug_ctc_head(4, K, 5, xd.data_ptr(), K + 2, *args[2:], 0, None, None) == -1    # rows are read as float4
