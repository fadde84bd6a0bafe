"""CPU: the checkbox stage's host side and its yardstick.

tests/checkbox_reference.py restates rapid_doc/utils/checkbox_det_cls.py `checkbox_predict` with OpenCV's published algorithms (cv2 is
not installed; PARITY UNPINNED).  Here: the restatement against scipy.ndimage where scipy has the same operation, the two identities the
kernels of csrc/kernels_checkbox.hip rely on, the CHAIN_APPROX_NONE border follower of csrc/polygon_ops.cpp against hand-written answers
(and CHAIN_APPROX_SIMPLE unchanged), the constants of csrc/checkbox_geom.h, `rd_checkbox_finish` against the restatement, the golden
lists minted from the reference's own file, and PageAnalyzer's route for a `checkbox_fn` that takes the page tensor."""
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import checkbox_reference as R  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]


def random_bitmap(seed, H, W, p_on=0.9):
    """dense enough for runs of 14 / 15 / 16 and for runs of 7 / 8 that touch the frame"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((H, W)) < p_on, 255, 0).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- restatement against scipy
def test_morphology_equals_scipy_with_the_border_conventions():
    ndi = pytest.importorskip("scipy.ndimage")
    for seed, (H, W) in enumerate([(1, 1), (14, 14), (15, 15), (40, 65), (33, 200)]):
        m = random_bitmap(seed, H, W)
        for kh, kw in ((1, 15), (15, 1), (3, 3)):
            st = np.ones((kh, kw), bool)
            assert np.array_equal(R.erode(m, kh, kw) != 0, ndi.binary_erosion(m != 0, st, border_value=1))
            assert np.array_equal(R.dilate(m, kh, kw) != 0, ndi.binary_dilation(m != 0, st, border_value=0))


def test_components_and_boxes_equal_scipy_as_sets():
    ndi = pytest.importorskip("scipy.ndimage")
    for seed, (H, W) in enumerate([(1, 1), (15, 15), (40, 65), (97, 130)]):
        m = random_bitmap(100 + seed, H, W, 0.55)
        n, labels, stats = R.connected_components_with_stats(m)
        lab, n_ref = ndi.label(m != 0, structure=np.ones((3, 3), int))
        assert n - 1 == n_ref
        mine = {frozenset(zip(*np.nonzero(labels == k))) for k in range(1, n)}
        assert mine == {frozenset(zip(*np.nonzero(lab == k))) for k in range(1, n_ref + 1)}
        boxes = {(sl[1].start, sl[0].start, sl[1].stop - sl[1].start, sl[0].stop - sl[0].start) for sl in ndi.find_objects(lab)}
        assert {tuple(int(v) for v in s[:4]) for s in stats[1:]} == boxes
        assert [int(s[4]) for s in stats[1:]] == [int((labels == k).sum()) for k in range(1, n)]
        # label order: the component's first 2 x 2 block in block-raster order
        keys = [R.block_key(stats[k], labels, k) for k in range(1, n)]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_label_order_differs_from_pixel_raster_order():
    m = np.zeros((20, 40), np.uint8)
    m[13:16, 2:5] = 255          # starts one row LOWER, further left
    m[12:15, 20:23] = 255
    _n, _l, stats = R.connected_components_with_stats(m)
    assert [tuple(int(v) for v in s[:2]) for s in stats[1:]] == [(2, 13), (20, 12)]


def test_mean_equals_an_fp64_correlation_away_from_ties():
    ndi = pytest.importorskip("scipy.ndimage")
    k = np.exp(-((np.arange(11) - 5.0) ** 2) / 8.0)
    k /= k.sum()
    rng = np.random.default_rng(5)
    for H, W in ((12, 12), (13, 50), (50, 37)):
        g = rng.integers(0, 256, (H, W)).astype(np.uint8)
        ref = ndi.correlate1d(ndi.correlate1d(g.astype(np.float64), k, axis=1, mode="nearest"), k, axis=0, mode="nearest")
        mine = R.adaptive_mean_gauss11(g)
        clear = np.abs(ref - np.floor(ref) - 0.5) > 1e-3
        assert clear.mean() > 0.99 and np.array_equal(mine[clear], np.rint(ref[clear]).astype(np.uint8))


def test_blur5_equals_an_exact_correlation():
    ndi = pytest.importorskip("scipy.ndimage")
    k = np.array([1, 4, 6, 4, 1], np.int64)
    g = np.random.default_rng(6).integers(0, 256, (17, 23)).astype(np.uint8)
    S = ndi.correlate1d(ndi.correlate1d(g.astype(np.int64), k, axis=1, mode="mirror"), k, axis=0, mode="mirror")
    assert np.array_equal(R.gaussian_blur5_u8(g), ((S + 128) >> 8).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------- the identities the kernels use
def _open_by_runs(m, axis):
    """keep every run whose length, plus 7 for each image edge it touches, is >= 15"""
    m = (m != 0) if axis == 1 else (m != 0).T
    out = np.zeros_like(m)
    for y in range(m.shape[0]):
        x0s, x1s = R._runs_of_row(m[y])
        for x0, x1 in zip(x0s.tolist(), x1s.tolist()):
            if (x1 - x0) + 7 * (x0 == 0) + 7 * (x1 == m.shape[1]) >= 15:
                out[y, x0:x1] = True
    return out if axis == 1 else out.T


def test_the_two_identities_on_200_random_bitmaps():
    rng = np.random.default_rng(7)
    seen_edge = 0
    for i in range(200):
        H, W = int(rng.integers(1, 48)), int(rng.integers(1, 140))
        m = random_bitmap(1000 + i, H, W, float(rng.choice([0.8, 0.9, 0.95])))
        for (kh, kw), axis in (((1, 15), 1), ((15, 1), 0)):
            opened, closed = R.morph_open(m, kh, kw), R.morph_close(m, kh, kw)
            assert np.array_equal(opened & closed, opened)                 # the closings are dead arithmetic
            by_runs = _open_by_runs(m, axis)
            assert np.array_equal(opened != 0, by_runs)
            seen_edge += int(by_runs[:, 0].any() or by_runs[0].any())
    assert seen_edge > 50


# ---------------------------------------------------------------------------------------------------------------- contours
def test_none_contours_known_answers_and_simple_unchanged():
    from rapiddoc_amd import layout_polygon as LP
    m = np.zeros((6, 7), np.uint8)
    m[1:4, 2:6] = 1               # a 4 x 3 rectangle: counter-clockwise in image coordinates, starting at its first pixel
    (c,) = LP.find_external_contours(m, approx_none=True)
    assert c.tolist() == [[2, 1], [2, 2], [2, 3], [3, 3], [4, 3], [5, 3], [5, 2], [5, 1], [4, 1], [3, 1]]
    (s,) = LP.find_external_contours(m)
    assert s.tolist() == [[2, 1], [2, 3], [5, 3], [5, 1]]
    m = np.zeros((3, 6), np.uint8)
    m[1, 1:5] = 1                 # a one-pixel line is walked there and back: inner points twice
    (c,) = LP.find_external_contours(m, approx_none=True)
    assert c.tolist() == [[1, 1], [2, 1], [3, 1], [4, 1], [3, 1], [2, 1]]
    (s,) = LP.find_external_contours(m)
    assert s.tolist() == [[1, 1], [4, 1]]
    m = np.zeros((4, 4), np.uint8)
    m[2, 1] = 1                   # a single pixel
    assert [c.tolist() for c in LP.find_external_contours(m, approx_none=True)] == [[[1, 2]]]
    m = np.zeros((5, 5), np.uint8)
    m[1, 2] = m[2, 1] = m[2, 3] = m[3, 2] = 1        # a diamond: 8-connected, four diagonal steps
    (c,) = LP.find_external_contours(m, approx_none=True)
    assert c.tolist() == [[2, 1], [1, 2], [2, 3], [3, 2]]
    # a ring with something inside its hole: RETR_EXTERNAL leaves the inner component out, in both forms
    m = np.zeros((9, 9), np.uint8)
    m[1:8, 1:8] = 1
    m[2:7, 2:7] = 0
    m[4, 4] = 1
    assert len(LP.find_external_contours(m, approx_none=True)) == 1 and len(LP.find_external_contours(m)) == 1
    assert len(LP.find_external_contours(m, approx_none=True)[0]) == 24
    assert LP.find_external_contours(np.zeros((5, 5), np.uint8), approx_none=True) == []


def test_none_contours_equal_the_restatement_on_random_masks():
    from rapiddoc_amd import layout_polygon as LP
    for seed in range(30):
        rng = np.random.default_rng(seed)
        m = (rng.random((int(rng.integers(1, 30)), int(rng.integers(1, 30)))) < 0.5).astype(np.uint8) * 255
        got = [c.tolist() for c in LP.find_external_contours(m, approx_none=True)]
        assert got == [c.reshape(-1, 2).tolist() for c in R.find_contours_external_none(m)]


# ---------------------------------------------------------------------------------------------------------------- constants, geometry
def test_geometry_header_constants():
    src = (ROOT / "rapiddoc_amd" / "csrc" / "checkbox_geom.h").read_text()
    taps = [float.fromhex(t.rstrip("f")) for t in re.search(r"RD_CB_MEAN_TAPS \{([^}]*)\}", src).group(1).split(", ")]
    assert np.array_equal(np.array(taps, np.float32), R.mean_taps_f32()[5:]) and np.array_equal(np.array(taps), np.array(taps, np.float32).astype(float))


def records_of(trace):
    """the records the device must leave for a page, from the restatement's trace"""
    from rapiddoc_amd import checkbox as CB
    rec = np.zeros(len(trace["cands"]), CB.CAND_DTYPE)
    for i, c in enumerate(trace["cands"]):
        rec[i]["key"], rec[i]["tick"] = c["key"], c["tick"]
        rec[i]["x"], rec[i]["y"], rec[i]["w"], rec[i]["h"] = c["box"]
        rec[i]["rx"], rec[i]["ry"], rec[i]["rw"], rec[i]["rh"] = c["roi_rect"]
        rows = R.pack_words(c["roi"])
        assert rows.shape[1] == 1
        rec[i]["roi"][:rows.shape[0]] = rows[:, 0]
    return rec


@pytest.fixture(scope="module")
def golden(golden_dir):
    pages = dict(np.load(golden_dir / "checkbox_pages.npz"))
    return pages, json.loads((golden_dir / "checkbox_expected.json").read_text())


def test_restatement_reproduces_the_minted_lists(golden):
    """the lists come from the reference's own checkbox_det_cls.py (tests/golden/make_golden_checkbox.py)"""
    pages, exp = golden
    assert set(pages) == set(exp["small"]) == {"outcomes", "filter_edges", "first_dropped"}
    for name, bgr in pages.items():
        assert R.checkbox_predict(bgr) == exp["small"][name]
    labels = [r["label"] for r in exp["small"]["outcomes"]]
    assert "Ticked" in labels and "Unticked" in labels


def test_finish_equals_the_restatement(golden):
    from rapiddoc_amd import checkbox as CB
    pages, exp = golden
    n_rejected = 0
    for name, bgr in pages.items():
        t = R.checkbox_trace(bgr)
        rec = records_of(t)
        n_rejected += sum(not c["keeps"] for c in t["cands"])
        assert CB.finish(rec, *bgr.shape[:2]) == exp["small"][name]
        assert CB.finish(rec[::-1], *bgr.shape[:2]) == exp["small"][name]            # the order comes from the keys
    assert n_rejected >= 1
    assert CB.finish(np.zeros(0, CB.CAND_DTYPE), 10, 10) == []
    # ROI rectangles over every size the filter lets through, at the page's corners too
    for w in range(12, 51):
        for h in range(12, 51):
            for x, y, W, H in ((0, 0, 60, 60), (3, 7, 1191, 1684), (1191 - w, 1684 - h, 1191, 1684), (16384 - w, 16384 - h, 16384, 16384)):
                rx, ry, rw, rh = R.roi_rect(np.int32(x), np.int32(y), np.int32(w), np.int32(h), W, H)
                assert 1 <= rw <= 60 and 1 <= rh <= 70 and rx + rw <= W and ry + rh <= H


def test_finish_random_pages_and_refuses_a_wrong_record():
    from rapiddoc_amd import checkbox as CB
    from rapiddoc_amd.engine import EngineError
    page = np.ascontiguousarray(R.form_page(3, 300, 420)[:, :, ::-1])
    t = R.checkbox_trace(page)
    rec = records_of(t)
    assert len(rec) >= 3 and CB.finish(rec, 300, 420) == t["result"]
    bad = rec.copy()
    bad[0]["rw"] += 1
    with pytest.raises(EngineError, match="disagrees"):
        CB.finish(bad, 300, 420)
    bad = rec.copy()
    bad[0]["w"] = 11
    with pytest.raises(EngineError, match="disagrees"):
        CB.finish(bad, 300, 420)
    with pytest.raises(EngineError, match="rd_checkbox_finish"):
        CB.finish(rec, 0, 420)


def test_device_entry_guards_launch_nothing_without_a_gpu_too():
    from rapiddoc_amd import _lib
    lib = _lib.load()
    assert lib.rd_checkbox_workspace(1, 0, 10, 100, 10, None) == 0 and lib.rd_checkbox_workspace(1, 16385, 10, 100, 10, None) == 0
    assert lib.rd_checkbox_workspace(1, 10, 16385, 100, 10, None) == 0 and lib.rd_checkbox_workspace(0, 10, 10, 100, 10, None) == 0
    assert lib.rd_checkbox_workspace(2, 16384, 16384, 100, 10, None) > 0
    for args in ((None, 1, 10, 10), (1, 1, 0, 10), (1, 1, 10, 16385), (1, 0, 10, 10)):
        pages, P, H, W = args
        assert lib.rd_checkbox_detect_device(0, pages, P, H, W, 0, 100, 10, 1, 1 << 30, 1, 1, None) == 1
        assert b"rd_checkbox_detect_device" in lib.rd_create_error()
    assert lib.rd_checkbox_detect_device(0, 1, 1, 10, 10, 0, 100, 10, 1, 16, 1, 1, None) == 1 and b"workspace holds 16 bytes" in lib.rd_create_error()


# ---------------------------------------------------------------------------------------------------------------- PageAnalyzer
def _run_seed7(golden_dir, checkbox_fn, log):
    import test_analyze_trace as T
    from rapiddoc_amd import analyze
    from rapiddoc_amd.pages import synth_page
    fx = json.loads((golden_dir / "analyze_trace_seed7.json").read_text())
    pages = torch.from_numpy(np.stack([synth_page(i)[0] for i in fx["page_ids"]]))
    det_calls = iter(fx["trace"]["det_calls"])

    def det_raw_fn(canvases, batch_size):
        return [np.asarray(b, dtype=np.float32).reshape(-1, 4, 2) for b in next(det_calls)["boxes"]]

    pa = analyze.PageAnalyzer(T.ReplayLayout(fx["layout_dets"], []), T.ReplayPipe([]),
                              formula_model=T.ReplayFormula([]) if fx["formula_enable"] else None, layout_batch_size=fx["layout_batch_num"],
                              formula_level=fx["formula_level"], formula_batch_size=fx["formula_batch_num"],
                              det_batch_num=fx["ocr_config"]["Det.rec_batch_num"], det_raw_fn=det_raw_fn,
                              seal_enable=fx["ocr_config"].get("seal_enable", True), checkbox_fn=checkbox_fn, checkbox_enable=True)
    return fx, pages, pa(pages)


def _hits(fx, k):                     # == make_golden_analyze.checkbox_predict
    first = next(d for d in fx["layout_dets"][k] if d["category_id"] in (0, 1, 2, 4, 6, 7, 9))
    x0, y0 = int(first["poly"][0]) + 12, int(first["poly"][1]) + 6
    return [{"bbox": [x0, y0, x0 + 14, y0 + 14], "text": "checked" if k == 0 else "unchecked", "score": 0.97},
            {"bbox": [3, 3, 15, 15], "text": "unchecked", "score": 0.5}]


def test_page_analyzer_hands_the_tensor_to_a_device_checkbox_fn(golden_dir):
    fx0 = json.loads((golden_dir / "analyze_trace_seed7.json").read_text())
    log = {"calls": [], "callable": 0}

    class DeviceStub:
        accepts_device_pages = True

        def detect_pages(self, pages):
            log["calls"].append(pages)
            return [_hits(fx0, k) for k in range(pages.shape[0])]

        def __call__(self, bgr):
            raise AssertionError("a checkbox_fn that accepts device pages is never called page by page")

    def plain(bgr):
        assert isinstance(bgr, np.ndarray)
        log["callable"] += 1
        return _hits(fx0, log["callable"] - 1)

    fx, pages, out_dev = _run_seed7(golden_dir, DeviceStub(), log)
    assert len(log["calls"]) == 1 and log["calls"][0] is pages            # the tensor itself, once, no numpy copy
    _fx, _pages, out_plain = _run_seed7(golden_dir, plain, log)
    assert log["callable"] == 2
    assert out_dev == out_plain == fx["output"]
    assert sum(1 for page in out_dev for d in page if d["category_id"] == 200) == 4


def test_checkbox_enable_without_a_function_names_the_class():
    import test_analyze_trace as T
    from rapiddoc_amd import analyze
    with pytest.raises(ValueError, match="checkbox_fn.*Mi355Checkbox"):
        analyze.PageAnalyzer(T.ReplayLayout([], []), T.ReplayPipe([]), checkbox_enable=True)
    from rapiddoc_amd import checkbox as CB
    assert CB.Mi355Checkbox.accepts_device_pages is True and CB.CAND_DTYPE.itemsize == 584 and CB.PAGE_DTYPE.itemsize == 32
