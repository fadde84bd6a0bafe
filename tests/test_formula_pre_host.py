"""CPU: the device formula pre-process's host side.  The numpy restatement of tests/formula_pre_reference.py equals Pillow (whole pipeline
on the fixture crops; reduce, the bicubic resample and the float32 box alone); `rd_formula_preproc_plan` equals the Python arithmetic;
the coefficient tables the device reads (`rd_debug_resample_coeffs`) equal the Python doubles entry by entry; the C surface is declared
in the header, the ctypes table and the library together."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))

import formula_pre_reference as R  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from rapiddoc_amd import build as rd_build
    rd_build.build(verbose=False)
    from rapiddoc_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def cases(golden_dir):
    return R.load_cases(golden_dir)


# ---------------------------------------------------------------------------------------------------------------- numpy against Pillow
def test_fixture_boxes_and_routes(cases):
    """every fixture crop has the box size the list asks for, the host's own box, and the route the plan arithmetic gives it; at least
    the four boxes whose 384 x L intermediate exceeds the bound are `host`, every other one `device`"""
    from rapiddoc_amd import formula_host as FH
    assert len(cases) == len(R.BOX_SIZES)
    for c, box_hw in zip(cases, R.BOX_SIZES):
        x0, y0, x1, y1 = c["box"]
        assert (y1 - y0, x1 - x0) == (box_hw or R.UNIFORM_HW), c["name"]
        assert R.margin_box(c["crop"]) == c["box"]
        pil = FH._crop_margin(Image.fromarray(c["crop"]))
        assert np.array_equal(np.asarray(pil), c["crop"][y0:y1, x0:x1]), c["name"]
        assert c["route"] == ("host" if box_hw in R.HOST_ROUTE_BOXES else "device")
        assert bool(R.plan(x1 - x0, y1 - y0)["served"]) == (c["route"] == "device")
    assert sum(c["route"] == "host" for c in cases) == 4


@pytest.mark.parametrize("i", range(len(R.BOX_SIZES)))
def test_numpy_pipeline_equals_pillow(cases, i):
    """margin box, bilinear resize, thumbnail (reduce + bicubic over the float32 box) and the pad, restated without Pillow, against the
    Pillow-minted bytes; the host-route crops too (the arithmetic has no bound, only the device path has)"""
    from rapiddoc_amd import formula_host as FH
    c = cases[i]
    got = R.decode(c["crop"])
    assert np.array_equal(got, c["u8"]), c["name"]
    assert R.crc(FH.to_network_input(got)) == c["input_crc32"]


def test_margin_threshold_in_integers_is_the_float64_one():
    """(L - mn) * 255 < 200 * (mx - mn) against the reference's float64 (L - mn) / (mx - mn) * 255 < 200, for every (mn, mx, L)"""
    L = np.arange(256, dtype=np.int64)
    for mn in range(255):
        for mx in range(mn + 1, 256):
            v = L[mn: mx + 1]
            f = (v - mn).astype(np.uint8) / np.uint8(mx - mn) * 255 < 200
            assert np.array_equal(f, (v - mn) * 255 < 200 * (mx - mn)), (mn, mx)


@pytest.mark.parametrize("hw,factors", [((128, 257), (3, 3)), ((97, 101), (5, 2)), ((64, 1000), (20, 19)), ((40, 77), (2, 4)), ((33, 50), (7, 1))])
def test_reduce_equals_pillow(hw, factors):
    img = R.make_crop(hw[0] + factors[0], hw)[:hw[0], :hw[1]]
    ref = np.asarray(Image.fromarray(img).reduce(factors))
    assert np.array_equal(R.reduce(img, *factors), ref)


@pytest.mark.parametrize("hw,out_wh", [((128, 854), (384, 58)), ((200, 90), (41, 93)), ((31, 47), (90, 60)), ((77, 300), (300, 20))])
def test_bicubic_equals_pillow(hw, out_wh):
    img = R.make_crop(7, hw)[:hw[0], :hw[1]]
    ref = np.asarray(Image.fromarray(img).resize(out_wh, resample=Image.BICUBIC))
    assert np.array_equal(R.resample(img, R.BICUBIC, out_wh[0], out_wh[1]), ref)


def test_the_box_passes_through_float32():
    """Image.resize(box=...) hands the box to C as float32: the restatement equals Pillow with float32(2560 / 3), and with the double the
    horizontal pass differs (printed: it is the reason the plan states the box as float32)"""
    img = R.make_crop(3, (128, 854))[:128, :854]
    box_w, box_h = 2560 / 3, 384 / 3
    ref = np.asarray(Image.fromarray(img).resize((384, 58), resample=Image.BICUBIC, box=(0, 0, box_w, box_h)))
    got = R.resample(img, R.BICUBIC, 384, 58, float(np.float32(box_w)), float(np.float32(box_h)))
    assert np.array_equal(got, ref)
    dbl = R.resample(img, R.BICUBIC, 384, 58, box_w, box_h)
    cols = int((dbl != ref).any(axis=(0, 2)).sum())
    print(f"\n[float32 box] with the double box {cols} of 384 columns differ from Pillow")
    assert R.plan(400, 60)["box_w"] == np.float32(box_w) and float(R.plan(400, 60)["box_w"]) != box_w


# ---------------------------------------------------------------------------------------------------------------- the plan
def _c_plan(lib, w, h):
    from rapiddoc_amd.engine import FormulaPlan
    p = FormulaPlan()
    assert lib.rd_formula_preproc_plan(w, h, C.byref(p)) == 0
    return p


def test_plan_equals_the_python_arithmetic(lib):
    sizes = sorted(set(range(1, 601, 7)) | {2, 3, 383, 384, 385, 600})
    pairs = [(w, h) for w in sizes for h in sizes]
    pairs += [(b[1], b[0]) for b in R.BOX_SIZES if b] + [(b[0], b[1]) for b in R.BOX_SIZES if b] + [R.UNIFORM_HW[::-1], (16384, 16384), (1, 42), (1, 43), (42, 1), (43, 1)]
    served = 0
    for w, h in pairs:
        want, got = R.plan(w, h), _c_plan(lib, w, h)
        for f in R.PLAN_FIELDS:
            v = getattr(got, f)
            if f.startswith("box_"):
                assert np.float32(v) == want[f], (w, h, f, v, want[f])
            else:
                assert v == want[f], (w, h, f, v, want[f])
        served += got.served
    assert 0 < served < len(pairs)
    for w, h in ((0, 5), (5, 0), (-1, 3), (16385, 4), (4, 16385)):                     # outside the bound: not served, nothing stated
        p = _c_plan(lib, w, h)
        assert p.served == 0 and p.resize_w == 0
    assert lib.rd_formula_preproc_plan(4, 4, None) != 0 and b"NULL" in lib.rd_create_error()
    p = _c_plan(lib, 400, 60)                                                           # a 60 x 400 formula: 384 x 2560, reduced by 3
    assert (p.resize_w, p.resize_h, p.final_w, p.final_h, p.fx, p.fy, p.reduced_w, p.reduced_h, p.pad_x, p.pad_y) == (2560, 384, 384, 58, 3, 3, 854, 128, 0, 163)
    assert _c_plan(lib, 40, 1).served == 1 and _c_plan(lib, 43, 1).served == 0          # 384 x 15360 inside, 384 x 16512 beyond


# ---------------------------------------------------------------------------------------------------------------- the tables
def _c_coeffs(lib, fn_name, args, n_out, cap=512):
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.full((n_out * cap,), -7, np.int32)
    ksize = getattr(lib, fn_name)(*args, bounds.ctypes.data, kk.ctypes.data, kk.size)
    assert 0 < ksize <= cap
    return bounds, kk[: n_out * ksize].reshape(n_out, ksize), ksize


@pytest.mark.parametrize("n_in,n_out", [(400, 2560), (60, 384), (2560, 384), (9, 384), (700, 5), (384, 383)])
def test_bilinear_full_box_tables(lib, n_in, n_out):
    """rd_debug_resample_coeffs(BILINEAR, full box) == the Python doubles == rd_debug_resize_aa_coeffs, entry by entry"""
    sys.path.insert(0, str(ROOT / "tests"))
    import table_path_reference as TP
    b0, k0, ks0 = R.resample_coeffs(R.BILINEAR, n_in, 0.0, float(n_in), n_out)
    b1, k1, ks1 = _c_coeffs(lib, "rd_debug_resample_coeffs", (R.BILINEAR, n_in, 0.0, float(n_in), n_out), n_out)
    b2, k2, ks2 = _c_coeffs(lib, "rd_debug_resize_aa_coeffs", (n_in, n_out), n_out)
    b3, k3, ks3 = TP.aa_coeffs(n_in, n_out)
    assert ks0 == ks1 == ks2 == ks3
    for b, k in ((b1, k1), (b2, k2), (b3, k3)):
        assert np.array_equal(b, b0) and np.array_equal(k, k0)


@pytest.mark.parametrize("n_in,box1,n_out", [(854, float(np.float32(2560 / 3)), 384), (128, 128.0, 58), (768, float(np.float32(15360 / 20)), 384),
                                              (21, float(np.float32(384 / 19)), 10), (391, 391.0, 384), (903, float(np.float32(1806 / 2)), 384)])
def test_bicubic_fractional_box_tables(lib, n_in, box1, n_out):
    b0, k0, ks0 = R.resample_coeffs(R.BICUBIC, n_in, 0.0, box1, n_out)
    b1, k1, ks1 = _c_coeffs(lib, "rd_debug_resample_coeffs", (R.BICUBIC, n_in, 0.0, box1, n_out), n_out)
    assert ks0 == ks1 and np.array_equal(b0, b1) and np.array_equal(k0, k1)
    assert (k0 < 0).any()                                                               # the negative lobes are there (rounded with -0.5)
    assert int(b0[:, 0].min()) >= 0 and int((b0[:, 0] + b0[:, 1]).max()) <= n_in        # no tap outside the source: the kernels rely on it


def test_coefficient_entry_refuses_bad_arguments(lib):
    b, k = np.zeros((8, 2), np.int32), np.zeros(8 * 16, np.int32)
    call = lambda *a, cap=k.size: lib.rd_debug_resample_coeffs(*a, b.ctypes.data, k.ctypes.data, cap)
    assert call(R.BICUBIC, 16, 0.0, 16.0, 8) > 0
    for args in ((1, 16, 0.0, 16.0, 8), (R.BICUBIC, 0, 0.0, 16.0, 8), (R.BICUBIC, 16, 0.0, 16.5, 8), (R.BICUBIC, 16, 4.0, 4.0, 8), (R.BICUBIC, 16, -1.0, 8.0, 8),
                 (R.BICUBIC, 16, 0.0, float("nan"), 8), (R.BICUBIC, 16385, 0.0, 16.0, 8)):
        assert call(*args) == -1, args
    assert call(R.BICUBIC, 16, 0.0, 16.0, 8, cap=8) == -1                               # too little room


# ---------------------------------------------------------------------------------------------------------------- the surface
def test_symbols_are_declared_together(lib):
    from rapiddoc_amd import _lib, build, formula_host
    header = (ROOT / "include" / "rapiddoc_mi355.h").read_text()
    for name in ("rd_formula_margin_boxes", "rd_formula_preproc_plan", "rd_formula_preproc_batch"):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and f"int {name}(" in header
    assert "rd_debug_resample_coeffs" in _lib.DEBUG_SYMBOLS and hasattr(lib, "rd_debug_resample_coeffs") and "rd_debug_resample_coeffs" not in header
    assert _lib.DEBUG_SYMBOLS["rd_debug_resize_aa_coeffs"][1] == [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]      # unchanged
    from rapiddoc_amd.engine import FORMULA_CROP_DTYPE, FormulaPlan
    assert FORMULA_CROP_DTYPE.itemsize == 24 and C.sizeof(FormulaPlan) == 56                 # rd_formula_crop, rd_formula_plan
    assert "kernels_resize_aa.hip" in build.SOURCES
    assert formula_host.FormulaRecognizer.accepts_device_images is True
