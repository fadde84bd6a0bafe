"""GPU: the fused stem front alone (csrc/kernels_stem_fused.hip, stem_fused_kernel<24 | 32 | 48>) and the fp32 stem1 kernel of the four-kernel
plan (stem_conv3x3s2_kernel) through the developer entry rd_debug_stem_front, element by element against the float64 reference and the
derived bound of tests/stem_front_reference.py (tests/test_stem_front_reference.py shows on the CPU that the bound holds for a correct
kernel and is broken by each wrong one).  Cases, measured err / bound and the range-flag findings: docs/notebook/stem_front_kernel.md.

Every output lives in a sentinel-filled buffer with guard rows (glue_helpers.View): nothing beside the view may change."""
import functools

import pytest
import torch

import stem_front_reference as R
from glue_helpers import View, lib

pytestmark = pytest.mark.gpu

CASES = {tag: (kw, widths, slot) for tag, kw, widths, slot in R.gpu_cases()}


@functools.lru_cache(maxsize=None)
def _problem(tag):
    kw, widths, slot = CASES[tag]
    case = R.build_case(kw, widths)
    return case, widths, slot, R.Reference(case, widths)


def _launch(case, route=1, widths=None, slot=None, flag=None, overrides=None):
    """One launch on a fresh sentinel-filled output view; returns (ms, view, cat [N][H2][W2][C] on the CPU)."""
    H2, W2 = R.out_hw(case.H, case.W)
    c = 2 * case.C1 if route == 1 else case.C1
    ld, off = slot or (c, 0)
    yv = View(case.N * H2 * W2, c, ld, off)
    dev = [t.contiguous().cuda() for t in (case.x, case.w1_stem(), case.b1, case.w2a_folded(), case.b2a, case.w2b_folded(), case.b2b)]
    tab = R.line_table(widths).cuda() if widths is not None else None
    a = dict(route=route, N=case.N, H=case.H, W=case.W, in_ch=case.in_ch, C1=case.C1, yld=ld)
    a.update(overrides or {})
    ms = lib().rd_debug_stem_front(a["route"], a["N"], a["H"], a["W"], a["in_ch"], a["C1"], a["yld"], 0, *[t.data_ptr() for t in dev], yv.ptr,
                                   tab.data_ptr() if tab is not None else None, flag.data_ptr() if flag is not None else None)
    torch.cuda.synchronize()
    return ms, yv, yv.owned().reshape(case.N, H2, W2, c)


def _check(tag, ms, yv, got, ref, bound):
    assert ms >= 0, (tag, "the entry declined")
    yv.assert_outside_untouched(tag)
    assert bool(torch.isfinite(got).all()), (tag, "not finite at", torch.nonzero(~torch.isfinite(got))[:8].tolist())
    err = (got.double() - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    worst = float(ratio.max())
    print(f"{tag}: max err {float(err.max()):.3e} worst err/bound {worst:.3f}")
    if worst > 1.0:
        bad = torch.nonzero(ratio > 1.0)
        at = [(tuple(i), float(err[tuple(i)]), float(bound[tuple(i)])) for i in bad[:8].tolist()]
        raise AssertionError((tag, "%d elements beyond their bound; ((n, y, x, channel), err, bound):" % len(bad), at))
    return worst


def _flag():
    return torch.zeros(4, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("tag", list(CASES))
def test_fused_kernel_matches_fp64(tag):
    """all three instances on inner / cut / one-row / one-column / tiny tiles, odd and even sizes, the grey input, row strides beyond 2 C1,
    coherent low planes, 2 and 3 tiles per persistent workgroup, a line table; ordinary magnitudes leave the range flag down"""
    case, widths, slot, ref = (_problem.__wrapped__ if "persistent" in tag else _problem)(tag)       # (the large one is not kept)
    flag = _flag()
    ms, yv, cat = _launch(case, 1, widths, slot, flag)
    _check(tag, ms, yv, cat, ref.cat, ref.bound)
    assert int(flag[0]) == 0, (tag, "range flag raised on ordinary magnitudes")


@pytest.mark.parametrize("c1", [24, 48])
@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_fp32_stem1_kernel_matches_fp64(shape, c1):
    """route 0: stem_conv3x3s2_kernel alone, e with ReLU, in a row stride wider than C1; one fp32 fma chain of K = 27"""
    case = _problem(f"C{c1}_{shape}")[0]
    e, bound = R.bound_route0(case)
    ms, yv, got = _launch(case, 0, slot=(c1 + 8, 4))
    _check(f"route0 C{c1}_{shape}", ms, yv, got, e, bound)


@pytest.mark.parametrize("c1", R.INSTANCES)
def test_rows_do_not_depend_on_the_launch(c1):
    """image 0 of a 30-image launch (240 tiles, one per workgroup, another grid) == image 0 alone, bit for bit"""
    case = R.Case(30, 48, 160, c1, seed=60)
    one = case.clone()
    one.N, one.x = 1, case.x[:1].contiguous()
    many = _launch(case)[2]
    alone = _launch(one)[2]
    assert torch.equal(many[:1], alone)


@pytest.mark.parametrize("c1", R.INSTANCES)
def test_line_table(c1):
    """Widths W, W - 1, 77, 16, 2, 1 in one launch: beyond its w2 every line is exactly 0.0, and its own columns are bit for bit what the same
    line gives when launched alone at W = w_in (one accumulation order per output element, whatever the launch or the tile's path)."""
    tag = f"C{c1}_lines"
    case, widths, _, ref = _problem(tag)
    ms, yv, cat = _launch(case, 1, widths)
    _check(tag, ms, yv, cat, ref.cat, ref.bound)           # each line against fp64 on its own crop; the bound is 0 beyond w2
    for n, w_in in enumerate(widths):
        w2 = (w_in - 1) // 2 + 1
        beyond = cat[n, :, w2:]
        assert beyond.numel() == 0 or bool((beyond.view(torch.int32) == 0).all()), (tag, n, "not +0.0 beyond the line's w2")
        one = case.clone()
        one.N, one.W, one.x = 1, w_in, case.x[n:n + 1, :, :, :w_in].contiguous()
        ms1, yv1, alone = _launch(one)
        assert ms1 >= 0
        yv1.assert_outside_untouched((tag, n))
        same = torch.equal(cat[n, :, :w2], alone[0])
        print(f"{tag} line {n} (w_in {w_in}, w2 {w2}): equal to the line alone: {same}")
        assert same, (tag, n, w_in, float((cat[n, :, :w2].double() - alone[0].double()).abs().max()))


@pytest.mark.parametrize("bad", [dict(C1=40), dict(C1=16), dict(in_ch=2), dict(in_ch=4), dict(yld=2 * 32 - 4), dict(yld=2 * 32 + 2), dict(route=2),
                                 dict(route=0, yld=28), dict(N=0)])
def test_bad_arguments_launch_nothing(bad):
    case = R.Case(1, 16, 64, 32, seed=70)
    ms, yv, got = _launch(case, bad.get("route", 1), slot=(96, 0), overrides=bad)
    assert ms == -1.0, bad
    yv.assert_outside_untouched(str(bad))
    assert bool(torch.isnan(got).all()), (bad, "the output view was written")


# ------------------------------------------------------------------------------------------------------------------------------ the range flag
# test_range_guard_falls_back_to_fp32's contract, at this kernel: an operand of a split product (x, e, a) at or beyond 65504 raises the flag -
# never a silently wrong answer.  b is no operand here: beyond 65504 and finite it is legal.
def _over(case, operand, where):
    """drive one operand over the fp16 range at one pixel (x[0, :, 10, 20] is the centre tap of e[0, :, 5, 10] alone) or everywhere"""
    c = case.clone()
    if operand == "x":
        if where == "single":
            c.x[0, :, 10, 20] = 1.0e5
        else:
            c.x *= 1.0e5
    elif operand == "e":
        if where == "single":
            c.x[0, :, 10, 20] = 6.0e4
            c.w1 *= 30
            c.b1 *= 30
        else:
            c.x *= 100
            c.w1 *= 1.0e3
            c.b1 *= 1.0e5
    elif operand == "a":
        if where == "single":
            c.x[0, :, 10, 20] = 6.0e4
            c.w2a *= 100
            c.b2a *= 100
        else:
            c.x *= 30
            c.w2a *= 1.0e5
            c.b2a *= 1.0e5
    return c


@pytest.mark.parametrize("c1", R.INSTANCES)
@pytest.mark.parametrize("where", ["single", "everywhere"])
@pytest.mark.parametrize("operand", ["x", "e", "a"])
def test_operand_beyond_fp16_range_raises_the_flag(operand, where, c1):
    case = _over(_problem(f"C{c1}_inner_cut_right_bottom")[0], operand, where)
    ref = R.Reference(case)
    big = {"x": float(case.x.abs().max()), "e": float(ref.e.max()), "a": float(ref.a.max())}
    order = ["x", "e", "a"]
    assert big[operand] > 65504.0 and all(big[o] < 65504.0 for o in order[:order.index(operand)]), big      # this operand is the first one over
    if where == "single":
        n_over = {"x": int((case.x.abs() > 65504).sum()) // 3, "e": int((ref.e.max(1).values > 65504).sum()), "a": int((ref.a.max(1).values > 65504).sum())}
        assert 1 <= n_over[operand] <= 4, n_over
    flag = _flag()
    ms, yv, cat = _launch(case, flag=flag)
    assert ms >= 0
    yv.assert_outside_untouched((operand, where, c1))
    print(f"C{c1} {operand} over the fp16 range ({where}; max |x| {big['x']:.3g} e {big['e']:.3g} a {big['a']:.3g}): flag {int(flag[0])}, "
          f"cat finite: {bool(torch.isfinite(cat).all())}")
    assert int(flag[0]) != 0, (operand, where, c1, "operand beyond the fp16 range and no flag")


@pytest.mark.parametrize("c1", R.INSTANCES)
@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")])
def test_non_finite_pixel_raises_the_flag(value, c1):
    case = _problem(f"C{c1}_odd_narrow")[0].clone()
    case.x[1, 1, 36, 44] = value                     # the last row and column of the image: an edge tile
    flag = _flag()
    ms, yv, cat = _launch(case, flag=flag)
    assert ms >= 0
    yv.assert_outside_untouched((value, c1))
    print(f"C{c1} x = {value} at one pixel: flag {int(flag[0])}, cat finite: {bool(torch.isfinite(cat).all())}")
    assert int(flag[0]) != 0


@pytest.mark.parametrize("c1", R.INSTANCES)
def test_outputs_beyond_fp16_range_are_legal(c1):
    """b is written, not split: finite values beyond 65504 leave the flag down and stay inside the bound; so does the largest legal operand"""
    case = _problem(f"C{c1}_inner_cut_right_bottom")[0].clone()
    for t, s in ((case.w2a, 100), (case.b2a, 100), (case.w2b, 1.0e4), (case.b2b, 1.0e4)):
        t *= s
    ref = R.Reference(case)
    assert float(ref.a.max()) < 65504.0 < float(ref.cat[..., c1:].max())
    flag = _flag()
    ms, yv, cat = _launch(case, flag=flag)
    _check(f"C{c1} b beyond 65504", ms, yv, cat, ref.cat, ref.bound)
    assert int(flag[0]) == 0
    case = _problem(f"C{c1}_inner_cut_right_bottom")[0].clone()
    case.x[0, 0, 10, 20] = 65000.0                   # the largest magnitudes that are still fp16 operands
    ref = R.Reference(case)
    assert float(ref.e.max()) < 65504.0 and float(ref.a.max()) < 65504.0
    ms, yv, cat = _launch(case, flag=flag)
    _check(f"C{c1} x = 65000 at one pixel", ms, yv, cat, ref.cat, ref.bound)
    assert int(flag[0]) == 0
