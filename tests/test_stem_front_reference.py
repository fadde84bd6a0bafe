"""CPU: how strong tests/test_gpu_stem_front.py is, checked without a GPU (tests/stem_front_reference.py).  On the operands of every GPU case
(a) a torch emulation of the kernel's arithmetic - fp16 hi / lo planes, three fp32-accumulated products per convolution, ReLU, the tile's
halo zeroed beyond the map and beyond a line's width - stays inside the per-element bound, so the bound is not too tight for a correct kernel;
(b) the same emulation made wrong in each way such a kernel goes wrong breaks the bound on the cases meant to catch it."""
import functools

import pytest
import torch

import stem_front_reference as R

CASES = {tag: (kw, widths) for tag, kw, widths, _ in R.gpu_cases()}


def _build(tag):
    kw, widths = CASES[tag]
    case = R.build_case(kw, widths)
    return case, widths, R.Reference(case, widths)


_cached = functools.lru_cache(maxsize=None)(_build)


def _problem(tag):
    return (_build if "persistent" in tag else _cached)(tag)       # (the large ones are used once: not kept)


def _worst(cat, ref):
    err = (cat.double() - ref.cat).abs()
    return float((err / ref.bound.clamp_min(1e-300)).max()), err


def test_reference_with_a_line_table_is_each_line_on_its_own_crop():
    case, widths, ref = _problem("C32_lines")
    H2, W2 = R.out_hw(case.H, case.W)
    for n, w_in in enumerate(widths):
        alone = R.Case.__new__(R.Case)
        alone.__dict__.update(case.__dict__)
        alone.N, alone.W, alone.x = 1, w_in, case.x[n:n + 1, :, :, :w_in].contiguous()
        one = R.Reference(alone)
        w2 = (w_in - 1) // 2 + 1
        assert one.cat.shape == (1, H2, w2, 2 * case.C1)
        assert torch.equal(ref.cat[n, :, :w2], one.cat[0]) and torch.equal(ref.bound[n, :, :w2], one.bound[0])
        assert float(ref.cat[n, :, w2:].abs().max()) == 0.0 if w2 < W2 else True
        assert float(ref.bound[n, :, w2:].abs().max()) == 0.0 if w2 < W2 else True


def test_reference_equals_the_module_definition():
    """StemBlock as the model files write it (nn.Conv2d + ReLU, F.pad (0, 1, 0, 1), max_pool2d(2, 1), cat [pool | stem2b]), in float64"""
    case, _, ref = _problem("C24_odd_narrow")
    nn = torch.nn
    c1, na = case.C1, case.NA
    convs = [nn.Conv2d(3, c1, 3, 2, 1), nn.Conv2d(c1, na, 2, 1, 0), nn.Conv2d(na, c1, 2, 1, 0)]
    for m, w, b in zip(convs, (case.w1, case.w2a, case.w2b), (case.b1, case.b2a, case.b2b)):
        m.double()
        m.weight.data, m.bias.data = w.double(), b.double()
    with torch.no_grad():
        x = torch.relu(convs[0](case.x.double()))
        x = torch.nn.functional.pad(x, (0, 1, 0, 1))
        x2 = torch.relu(convs[1](x))
        x2 = torch.nn.functional.pad(x2, (0, 1, 0, 1))
        x2 = torch.relu(convs[2](x2))
        x1 = torch.nn.functional.max_pool2d(x, 2, 1)
        cat = torch.cat([x1, x2], 1).permute(0, 2, 3, 1)
    assert float((cat - ref.cat).abs().max()) < 1e-13


@pytest.mark.parametrize("c1", R.INSTANCES)
def test_operands_leave_a_real_share_of_relu_zeros(c1):
    _, _, ref = _problem(f"C{c1}_inner_cut_right_bottom")
    b = ref.cat[..., c1:]
    for name, t in (("e", ref.e), ("a", ref.a), ("b", b)):
        share = float((t == 0).double().mean())
        assert 0.15 < share < 0.85, (name, share)
        assert float(t.max()) > 0.1, name


def test_layouts_of_the_entry():
    case = R.Case(1, 4, 4, 24)
    assert float(case.w1_stem()[(1 * 3 + 2) * 3 + 1, 5]) == float(case.w1[5, 1, 1, 2])
    assert float(case.w2a_folded()[3, (1 * 2 + 0) * 24 + 7]) == float(case.w2a[3, 7, 1, 0])
    assert float(case.w2b_folded()[9, (0 * 2 + 1) * 12 + 11]) == float(case.w2b[9, 11, 0, 1])
    assert R.line_table([160, 77, 1]).tolist() == [[160, 80, 40, 0], [77, 39, 20, 20], [1, 1, 1, 30]]


@pytest.mark.parametrize("tag", list(CASES))
def test_emulated_kernel_stays_inside_the_bound(tag):
    """(a): the bound is not too tight for a correct kernel"""
    case, widths, ref = _problem(tag)
    cat = R.emulate(case, widths)
    assert cat.shape == ref.cat.shape
    worst, err = _worst(cat, ref)
    print(f"{tag}: emulated kernel max err {float(err.max()):.3e} worst err/bound {worst:.3f}")
    assert worst <= 1.0, (tag, worst)
    if widths is not None:
        for n, w_in in enumerate(widths):
            assert float(cat[n, :, (w_in - 1) // 2 + 1:].abs().max() if (w_in - 1) // 2 + 1 < cat.shape[2] else 0.0) == 0.0


_BIG = [f"C{c}_inner_cut_right_bottom" for c in R.INSTANCES]
MUTANT_CASES = [
    ("drop_lo_hi_stem1", _BIG),
    ("drop_lo_hi_stem2a", [f"C{c}_coherent_e" for c in R.INSTANCES]),       # (on random operands: 0.9 .. 2.3 of the bound - not a catch)
    ("drop_lo_hi_stem2b", [f"C{c}_coherent_a" for c in R.INSTANCES]),
    ("drop_lo_hi", _BIG + ["C32_grey", "C24_lines"]),
    ("stem2a_tap_shifted", _BIG + ["C24_tiny_3x5"]),
    ("e_map_halo_kept", [f"C{c}_one_exact_tile" for c in R.INSTANCES] + ["C32_odd_narrow", "C48_tiny_1x1", "C32_even_h_odd_w", "C32_odd_h_even_w"]),
    ("line_halo_kept", [f"C{c}_lines" for c in R.INSTANCES]),
    ("a_pad_nonzero_w_pad_nonzero", ["C24_inner_cut_right_bottom", "C24_odd_narrow", "C24_tiny_1x1"]),
    ("n_block_row_stem1", ["C48_inner_cut_right_bottom", "C48_tiny_1x1"]),
    ("n_block_row_stem2b", ["C48_inner_cut_right_bottom", "C48_tiny_1x1"]),
]


@pytest.mark.parametrize("mutant,tag", [(m, t) for m, tags in MUTANT_CASES for t in tags])
def test_wrong_kernel_breaks_the_bound(mutant, tag):
    """(b): each wrong kernel is seen on every case meant to catch it"""
    case, widths, ref = _problem(tag)
    worst, err = _worst(R.emulate(case, widths, mutant), ref)
    print(f"{tag} {mutant}: worst err/bound {worst:.3g}, {int((err > ref.bound).sum())} elements beyond their bound")
    assert worst > 1.0, (mutant, tag, worst)


def test_pad_channels_of_a_alone_cannot_be_seen_in_the_output():
    """C1 = 24: stem2a's lanes 12 .. 15 compute channel 11 again and store 0.0 into the tile's pad channels.  Storing what they computed
    instead changes NO output, because the weight image's pad slots are zero as well (csrc/kernels_stem_fused.hip sf_prepare): the two zeros
    protect each other, and only both gone is a wrong kernel (a_pad_nonzero_w_pad_nonzero above)."""
    case, widths, _ = _problem("C24_inner_cut_right_bottom")
    assert torch.equal(R.emulate(case, widths, "a_pad_nonzero"), R.emulate(case, widths))
