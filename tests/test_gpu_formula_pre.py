"""GPU: the formula pre-process on the device (`rd_formula_margin_boxes`, `rd_formula_preproc_batch`, csrc/kernels_resize_aa.hip;
`engine.formula_preprocess`) against the Pillow-minted fixtures of tests/golden/make_golden_formula_pre_device.py.

The arithmetic is integer up to the last step, so everything is asserted EXACTLY: the padded uint8 384 x 384 x 3 image byte for byte, the
float32 network input bit for bit against torch's CPU evaluation of (u8 * f32(1 / 255) - mean) / std and the grey sum, and by crc32 against
the fixture.  Every crop rides as a window of a page whose width is no multiple of 4, at an odd x0 (bases and pitches that are not
4-byte aligned).  Then: margin boxes, batch against alone, a view against its copy, guard rows, the routes of the over-bound crops, and
the callers - `FormulaRecognizer.batch_predict` on device views against numpy, `analyze.recognise_formulas` with the switch on `host` (a
fresh child process), by default, on `device`, and with a stand-in model, which must see numpy arrays."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import formula_pre_reference as R
from rapiddoc_amd import weights as W

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
_CACHE = {}


def _cases(golden_dir):
    if "cases" not in _CACHE:
        _CACHE["cases"] = R.load_cases(golden_dir)
    return _CACHE["cases"]


def _window(crop: np.ndarray, x0: int = 5, y0: int = 2) -> torch.Tensor:
    """the crop as a window of a noise page: odd x0, a page width that is no multiple of 4"""
    h, w = crop.shape[:2]
    pw = w + x0 + 4
    pw += 1 if pw % 4 == 0 else 0
    page = np.random.default_rng(h * 131 + w).integers(0, 256, (h + y0 + 3, pw, 3)).astype(np.uint8)
    page[y0: y0 + h, x0: x0 + w] = crop
    view = torch.from_numpy(page).cuda()[y0: y0 + h, x0: x0 + w]
    assert not view.is_contiguous() or h == 1
    assert (view.data_ptr() % 4 != 0) or (view.stride(0) % 4 != 0) or h == 1
    return view


def _network_input(u8: np.ndarray) -> torch.Tensor:
    """step 5 as torch CPU operations, one rounded operation each: uint8 [..., 384, 384, 3] -> float32 [..., 384, 384]"""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    x = (torch.from_numpy(np.ascontiguousarray(u8)).float() * f32(float(1 / 255.0)) - f32(0.7931)) / f32(0.1738)
    return (f32(0.114) * x[..., 0] + f32(0.587) * x[..., 1]) + f32(0.299) * x[..., 2]


def _device_results(golden_dir):
    """every device-route fixture crop, as page windows, in ONE batch: (cases, x, routes, u8)"""
    if "dev" not in _CACHE:
        from rapiddoc_amd.engine import formula_preprocess
        cases = [c for c in _cases(golden_dir) if c["route"] == "device"]
        x, routes, u8 = formula_preprocess([_window(c["crop"]) for c in cases], return_u8=True)
        torch.cuda.synchronize()
        _CACHE["dev"] = (cases, x.cpu(), routes, u8.cpu().numpy())
    return _CACHE["dev"]


def test_bytes_equal_the_pillow_fixtures(golden_dir):
    cases, x, routes, u8 = _device_results(golden_dir)
    assert len(cases) == len(R.BOX_SIZES) - len(R.HOST_ROUTE_BOXES) and routes == ["device"] * len(cases)
    bad = []
    for i, c in enumerate(cases):
        diff = int((u8[i] != c["u8"]).sum())
        print(f"[formula_pre {c['name']}] bytes differing from Pillow: {diff}")
        if diff:
            bad.append((c["name"], diff))
    assert not bad, bad


def test_floats_are_bit_equal_to_the_cpu_expression_and_the_fixture_crc(golden_dir):
    cases, x, routes, u8 = _device_results(golden_dir)
    assert tuple(x.shape) == (len(cases), 1, 384, 384) and x.dtype == torch.float32
    for i, c in enumerate(cases):
        ref = _network_input(c["u8"])
        assert torch.equal(x[i, 0].view(torch.int32), ref.view(torch.int32)), c["name"]
        assert R.crc(x[i: i + 1].numpy()) == c["input_crc32"], c["name"]


def test_margin_boxes_equal_the_host_boxes(golden_dir):
    from rapiddoc_amd.engine import formula_margin_boxes
    cases = _cases(golden_dir)                                             # the host-route crops and the uniform patch included
    crops, want = [_window(c["crop"]) for c in cases], [tuple(c["box"]) for c in cases]
    for corner in ((0, 0), (0, 58), (36, 0), (36, 58)):                    # one dark pixel in a corner of a light 37 x 59 patch
        a = np.random.default_rng(corner[0] + corner[1]).integers(225, 256, (37, 59, 3)).astype(np.uint8)
        a[corner] = (10, 20, 5)
        assert R.margin_box(a) == (corner[1], corner[0], corner[1] + 1, corner[0] + 1)
        crops.append(_window(a, x0=3, y0=1))
        want.append(R.margin_box(a))
    flat = np.full((70, 300, 3), 255, np.uint8)                            # wider than a wavefront, and a gradient that is not uniform
    flat[:, 150:] = 254
    crops.append(_window(flat))
    want.append(R.margin_box(flat))
    got = formula_margin_boxes(crops).cpu().numpy()
    assert [tuple(int(v) for v in b) for b in got] == want


def test_a_batch_equals_each_crop_alone(golden_dir):
    from rapiddoc_amd.engine import formula_preprocess
    cases = {c["name"]: c for c in _cases(golden_dir)}
    crops = [_window(cases[n]["crop"]) for n in ("box_60x400", "box_301x64", "box_13x17")]
    x, routes, u8 = formula_preprocess(crops, return_u8=True)
    for i, crop in enumerate(crops):
        xa, ra, ua = formula_preprocess([crop], return_u8=True)
        assert ra == ["device"] and torch.equal(xa[0].view(torch.int32), x[i].view(torch.int32)) and torch.equal(ua[0], u8[i])
    x2, _ = formula_preprocess(crops[::-1])                                # another order, no byte output: the same floats
    assert torch.equal(x2.flip(0).view(torch.int32), x.view(torch.int32))


def test_a_view_equals_its_contiguous_copy(golden_dir):
    from rapiddoc_amd.engine import formula_preprocess
    cases = {c["name"]: c for c in _cases(golden_dir)}
    for name in ("box_37x291", "box_640x16", "box_401x400"):
        view = _window(cases[name]["crop"])
        a = formula_preprocess([view], return_u8=True)
        b = formula_preprocess([view.contiguous()], return_u8=True)
        assert a[1] == b[1] == ["device"] and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[2], b[2])
        assert np.array_equal(a[2][0].cpu().numpy(), cases[name]["u8"])


def _call_batch(lib, crops, boxes, out_ptr, u8_ptr):
    from rapiddoc_amd.engine import _formula_descs
    descs = _formula_descs(crops)
    b = np.ascontiguousarray(boxes, dtype=np.int32)
    return lib.rd_formula_preproc_batch(0, descs.ctypes.data, b.ctypes.data, len(crops), out_ptr, u8_ptr, torch.cuda.current_stream().cuda_stream)


def test_guard_rows_stay_untouched(golden_dir):
    from rapiddoc_amd import _lib
    lib = _lib.load()
    cases = {c["name"]: c for c in _cases(golden_dir)}
    picked = [cases[n] for n in ("box_200x90", "box_1x1", "uniform")]
    crops = [_window(c["crop"]) for c in picked]
    n, px = len(crops), 384 * 384
    out = torch.full(((n + 2) * px,), float("nan"), dtype=torch.float32, device="cuda")
    u8 = torch.full(((n + 2) * px * 3,), 0xA5, dtype=torch.uint8, device="cuda")
    assert _call_batch(lib, crops, [c["box"] for c in picked], out.data_ptr() + 4 * px, u8.data_ptr() + 3 * px) == 0
    torch.cuda.synchronize()
    o, b = out.cpu().view(n + 2, px), u8.cpu().view(n + 2, px * 3)
    assert bool(torch.isnan(o[0]).all()) and bool(torch.isnan(o[-1]).all()) and bool((b[0] == 0xA5).all()) and bool((b[-1] == 0xA5).all())
    for i, c in enumerate(picked):
        assert np.array_equal(b[1 + i].numpy().reshape(384, 384, 3), c["u8"]), c["name"]
        assert R.crc(o[1 + i].numpy()) == c["input_crc32"]


def test_bad_arguments_launch_nothing(golden_dir):
    from rapiddoc_amd import _lib
    lib = _lib.load()
    cases = {c["name"]: c for c in _cases(golden_dir)}
    ok, far = cases["box_13x17"], cases["box_5x700"]
    crop, wide = _window(ok["crop"]), _window(far["crop"])
    out = torch.full((2 * 384 * 384,), float("nan"), dtype=torch.float32, device="cuda")
    h, w = ok["crop"].shape[:2]
    for crops, boxes, ptr in (([crop], [ok["box"]], None), ([crop], [(0, 0, w + 1, h)], out.data_ptr()), ([crop], [(3, 0, 3, h)], out.data_ptr()),
                              ([crop], [(-1, 0, w, h)], out.data_ptr()), ([crop, wide], [ok["box"], far["box"]], out.data_ptr())):
        assert _call_batch(lib, crops, boxes, ptr, None) != 0
        assert b"rd_formula_preproc_batch" in lib.rd_create_error()
    assert b"served = 0" in lib.rd_create_error()                          # the last one: the second crop's plan declines, the first did not run
    assert lib.rd_formula_preproc_batch(0, None, None, 1, out.data_ptr(), None, None) != 0
    assert lib.rd_formula_margin_boxes(0, None, 1, None, None) != 0 and b"rd_formula_margin_boxes" in lib.rd_create_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert _call_batch(lib, [crop], [ok["box"]], out.data_ptr(), None) == 0           # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert R.crc(out[: 384 * 384].cpu().numpy()) == ok["input_crc32"] and bool(torch.isnan(out[384 * 384:]).all())


def test_over_bound_crops_take_the_host_route_with_the_host_bits(golden_dir):
    from rapiddoc_amd.engine import formula_preprocess
    cases = {c["name"]: c for c in _cases(golden_dir)}
    names = ["box_5x700", "box_13x17", "box_3x2000"]
    x, routes, u8 = formula_preprocess([_window(cases[n]["crop"]) for n in names], return_u8=True)
    assert routes == ["host", "device", "host"]
    for i, n in enumerate(names):
        assert np.array_equal(u8[i].cpu().numpy(), cases[n]["u8"]) and R.crc(x[i: i + 1].cpu().numpy()) == cases[n]["input_crc32"], n
    grey = torch.from_numpy(cases["box_13x17"]["crop"][..., 1].copy()).cuda()          # H x W: the host path's own case
    xg, rg = formula_preprocess([grey, torch.zeros((0, 5, 3), dtype=torch.uint8, device="cuda")])
    from rapiddoc_amd import formula_host as FH
    assert rg == ["host", "empty"] and np.array_equal(xg[0:1].cpu().numpy(), FH.preprocess([grey.cpu().numpy()])[0]) and not bool(xg[1].any())


# ---------------------------------------------------------------------------------------------------------------- the callers
@pytest.fixture(scope="module")
def recogniser(golden_dir):
    from rapiddoc_amd.formula_host import FormulaRecognizer
    return FormulaRecognizer(W.synth_state_dict(W.load_manifest(golden_dir / "manifest_ppformulanet_plus_m_m8.json"), 0), max_new_tokens=6)


@pytest.fixture()
def device_switch(monkeypatch):
    from rapiddoc_amd import formula_host as FH
    monkeypatch.setattr(FH, "PREPROC_SWITCH", "device")


def test_batch_predict_on_device_views_returns_the_numpy_ids(golden_dir, recogniser, device_switch):
    cases = {c["name"]: c for c in _cases(golden_dir)}
    names = ["box_60x400", "box_5x700", "box_50x51", "uniform", "box_200x90"]
    crops = [cases[n]["crop"] for n in names]
    want = recogniser.batch_predict(crops, batch_size=2)
    assert recogniser.last_routes == ["numpy"] * 5
    got = recogniser.batch_predict([_window(c) for c in crops], batch_size=2)            # chunks of 2, 2, 1; one of them mixed
    assert recogniser.last_routes == ["device", "host", "device", "device", "device"]
    assert got == want and all(isinstance(r, list) for r in got)
    mixed = recogniser.batch_predict([_window(crops[0]), crops[1], _window(crops[2])], batch_size=16)         # device tensors next to numpy
    assert recogniser.last_routes == ["device", "numpy", "device"] and mixed == want[:3]


def _branch_inputs():
    """the pages and detections of tests/test_gpu_parity.py::test_formula_branch_on_given_layout"""
    rng = np.random.default_rng(5)
    pages = rng.integers(0, 255, (2, 400, 600, 3), dtype=np.uint8)
    pages[:, 100:160, 200:420] = 255
    pages[:, 120:140, 230:390] = 30
    mk = lambda cid, x0, y0, x1, y1: {"category_id": cid, "poly": [x0, y0, x1, y0, x1, y1, x0, y1], "score": 0.9}
    return pages, [[mk(14, 200, 100, 420, 160), mk(1, 20, 20, 580, 90), mk(13, 230, 300, 300, 330)], [mk(8, 200, 100, 420, 160)]]


def _branch_latex(rec):
    from rapiddoc_amd.analyze import recognise_formulas
    pages, dets = _branch_inputs()
    assert recognise_formulas(torch.from_numpy(pages).cuda(), dets, rec) == 3
    return [[d.get("latex") for d in page] for page in dets]


def _child_main():
    """run by test_recognise_formulas_is_the_same_on_every_route in a fresh process with RD_FORMULA_PREPROC=host"""
    from rapiddoc_amd import formula_host as FH
    assert FH.PREPROC_SWITCH == "host" and not FH.device_preproc_enabled()
    rec = FH.FormulaRecognizer(W.synth_state_dict(W.load_manifest(ROOT / "tests" / "golden" / "manifest_ppformulanet_plus_m_m8.json"), 0), max_new_tokens=6)
    latex = _branch_latex(rec)
    print("RESULT " + json.dumps({"latex": latex, "routes": rec.last_routes}))


def test_recognise_formulas_is_the_same_on_every_route(golden_dir, recogniser, monkeypatch):
    from rapiddoc_amd import formula_host as FH
    env = dict(os.environ, RD_FORMULA_PREPROC="host")
    code = f"import sys; sys.path[:0] = [{str(ROOT)!r}, {str(ROOT / 'tests')!r}]; import test_gpu_formula_pre as T; T._child_main()"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads(next(line for line in r.stdout.splitlines() if line.startswith("RESULT "))[7:])
    assert child["routes"] == ["numpy"] * 3                                # the host switch: recognise_formulas hands numpy crops over
    by_default = _branch_latex(recogniser)
    default_routes = list(recogniser.last_routes)
    monkeypatch.setattr(FH, "PREPROC_SWITCH", "device")
    on_device = _branch_latex(recogniser)
    assert recogniser.last_routes == ["device"] * 3
    assert default_routes == (["device"] * 3 if FH.DEVICE_BY_DEFAULT else ["numpy"] * 3)
    assert child["latex"] == by_default == on_device
    assert isinstance(on_device[0][0], list) and on_device[0][0] == on_device[1][0] and on_device[0][1] is None

    class StandIn:                                                         # a CustomBaseModel-shaped object: no accepts_device_images
        def __init__(self, inner):
            self.inner, self.seen = inner, []

        def batch_predict(self, images, batch_size=16, **kw):
            self.seen.extend(images)
            return self.inner.batch_predict(images, batch_size=batch_size)
    stand_in = StandIn(recogniser)
    assert _branch_latex(stand_in) == on_device
    assert len(stand_in.seen) == 3 and all(isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim == 3 for a in stand_in.seen)
    pages, dets = _branch_inputs()                                         # a region with polygon_points (they survive only an
    dets[0][0]["polygon_points"] = [[205, 105], [415, 105], [415, 155], [205, 155]]        # unexpanded crop) keeps the host crop
    from rapiddoc_amd.analyze import recognise_formulas
    recognise_formulas(torch.from_numpy(pages).cuda(), dets, recogniser, expand_px=0)
    assert recogniser.last_routes == ["numpy", "device", "device"]
