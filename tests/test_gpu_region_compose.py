"""GPU: region composition on the device (csrc/kernels_region.hip, rd_region_canvases; engine.region_canvases) BYTE FOR BYTE against the
numpy restatement of tests/region_reference.py - a slice, layout_polygon.polygon_keep_mask, analyze._int_box - and the two routes of
RegionOcr / TableOcr.ocr_result against each other.  Pages are at most 200 x 300, canvases 64 to 256 on a side."""
import ctypes as C

import numpy as np
import pytest
import torch

import region_reference as R
from rapiddoc_amd import _lib, analyze, engine
from rapiddoc_amd import weights as W
from rapiddoc_amd.engine import Region
from test_region_geom_host import FIXED, _cap_polygon

pytestmark = pytest.mark.gpu


def _page(seed, h, w):
    return np.random.default_rng(seed).integers(0, 255, size=(h, w, 3), dtype=np.uint8)        # never 255: white is fill only


@pytest.fixture(scope="module")
def pages():
    """two pages of different sizes; the second is a window of a larger buffer (pitch != 3 W)"""
    a, big = _page(1, 200, 300), _page(2, 190, 280)
    ta, tbig = torch.from_numpy(a).cuda(), torch.from_numpy(big).cuda()
    tb = tbig[12:172, 30:250]
    assert tb.stride(0) == 840 != 3 * tb.shape[1]
    return [(a, ta), (big[12:172, 30:250], tb)]


def _check(pages, specs, gh, gw, want_masked=True):
    """specs: (page index, rect, paste, polygon, float boxes) -> one launch, compared canvas by canvas; returns the canvases"""
    regions, want = [], []
    for p, rect, paste, poly, fboxes in specs:
        boxes = [ib for ib in (analyze._int_box(b, gh, gw) for b in fboxes) if ib]
        regions.append(Region(pages[p][1], rect, paste, poly, boxes))
        want.append(R.compose(pages[p][0], rect, paste, poly, boxes, gh, gw))
    canv, det = engine.region_canvases(regions, (gh, gw), want_masked)
    torch.cuda.synchronize()
    assert (det is not None) == want_masked
    for k, (c, d) in enumerate(want):
        assert np.array_equal(canv[k].cpu().numpy(), c), ("canvas", k, specs[k][:3])
        if want_masked:
            assert np.array_equal(det[k].cpu().numpy(), d), ("det canvas", k, specs[k][:3])
    return canv, det, want


# inside, over each of the four borders, over a corner, missing the page, 1 x 1, the whole page b
RECTS = [(0, (40, 30, 180, 150)), (0, (-25, 40, 90, 120)), (0, (230, 20, 345, 130)), (0, (60, -30, 200, 70)), (0, (50, 120, 150, 260)),
         (1, (-10, -12, 100, 90)), (1, (150, 100, 260, 200)), (0, (400, 300, 460, 350)), (0, (-80, 10, -5, 60)), (0, (77, 99, 78, 100)),
         (1, (0, 0, 220, 160))]


@pytest.mark.parametrize("paste,gh,gw", [(50, 256, 256), (0, 256, 256), (0, 160, 220), (50, 123, 77), (3, 64, 192)])
def test_rectangles_equal_the_numpy_restatement(pages, paste, gh, gw):
    """256 x 256 / 64 x 192: the 16-byte route; 160 x 220 (660 bytes a row) and 123 x 77: the route for any width.  On the small
    canvases most windows leave the canvas as well - they are cut there."""
    boxes = [(10.5, 12.25, 40.75, 30.5), (30, 20, 60, 50), (-5, -5, 8.5, 9), (52.5, 56.25, 70.75, 75.5), (60, 51, 75, 64.01), (gw - 20.5, gh - 9.5, gw + 30, gh + 2), (0, gh - 1, gw, gh), (500, 500, 600, 600)]
    specs = [(p, rect, (paste, paste), None, boxes if k % 2 == 0 else []) for k, (p, rect) in enumerate(RECTS)]
    _canv, _det, want = _check(pages, specs, gh, gw)
    assert sum(int((c != 255).any()) for c, _d in want) >= 5 and any((c != d).any() for c, d in want)
    _check(pages, specs, gh, gw, want_masked=False)                  # det_canv_dev = NULL: the plain canvases alone


def test_polygons_on_a_clipped_window_equal_the_numpy_restatement(pages):
    """every polygon of tests/test_region_geom_host.py's list (given there in window coordinates), on a region that overhangs the page's
    left and top edges - the raster is that of the polygon translated by the UNclipped corner on a window of the CLIPPED size - and on
    one that overhangs right and bottom"""
    specs = []
    for name, pts in FIXED.items():
        pts = _cap_polygon(engine.REGION_MAX_POLY) if pts is None else np.asarray(pts, np.int32)
        for p, (x0, y0, x1, y1) in ((0, (-9, -7, 39, 33)), (0, (270, 175, 318, 215)), (1, (100, 60, 148, 100))):
            # raster coordinate = page coordinate - the UNclipped corner (fractions: truncated towards zero by the packing)
            page_pts = (pts.astype(np.float64) + [x0 + 0.6, y0 + 0.3]).tolist()
            specs.append((p, (x0, y0, x1, y1), (20, 20), page_pts, [(25.5, 25.5, 40, 40)]))
    _canv, _det, want = _check(pages, specs, 128, 128)
    assert len(specs) == 3 * len(FIXED) and sum(int((c != 255).any()) for c, _d in want) >= len(FIXED)
    _check(pages, specs[:9], 90, 101)                                # the same through the any-width route


def _raw(lib, stage, n, gh, gw, canv_ptr, det_ptr, ws_ptr, ws_bytes, descs_ptr=None, first=0):
    d = stage.descs_ptr + 64 * first if descs_ptr is None else descs_ptr
    return lib.rd_region_canvases(0, d, n, stage.pts_ptr, stage.boxes_ptr, gh, gw, canv_ptr, det_ptr, ws_ptr, ws_bytes, engine._stream_ptr())


def _some_regions(pages, gh=128, gw=192):
    """a polygon region with a box, a region over the top left corner of the window page, one over the right edge with boxes that touch
    the canvas's edges"""
    poly = [[60, 40], [150, 50], [140, 120], [70, 110]]
    return [Region(pages[0][1], (40, 30, 180, 150), (5, 5), poly, [[10, 10, 60, 40]]), Region(pages[1][1], (-10, -12, 100, 90), (0, 0), None, []),
            Region(pages[0][1], (230, 20, 345, 130), (7, 9), None, [[0, 0, gw, 3], [gw - 40, gh - 20, gw, gh]])]


def test_guard_rows_around_both_canvases_stay_untouched(pages):
    lib = _lib.load()
    for gh, gw in ((128, 192), (97, 131)):
        boxes_ok = regions = _some_regions(pages, gh, gw)
        stage = engine.RegionStage([boxes_ok], torch.device("cuda", 0))
        n, row = len(regions), gw * 3
        guard = 16 * row                                             # 16 sentinel rows in front of, between and behind the canvases
        buf = torch.full((3 * guard + 2 * n * gh * row,), 0x5A, dtype=torch.uint8, device="cuda")
        canv_off, det_off = guard, 2 * guard + n * gh * row
        ws = torch.empty(lib.rd_region_canvases_workspace(n, gh, gw), dtype=torch.uint8, device="cuda")
        assert _raw(lib, stage, n, gh, gw, buf.data_ptr() + canv_off, buf.data_ptr() + det_off, ws.data_ptr(), ws.numel()) == 0, lib.rd_create_error()
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        for a, b in ((0, canv_off), (canv_off + n * gh * row, det_off), (det_off + n * gh * row, len(out))):
            assert (out[a:b] == 0x5A).all(), (gh, gw, a, b)
        canv = out[canv_off: canv_off + n * gh * row].reshape(n, gh, gw, 3)
        det = out[det_off: det_off + n * gh * row].reshape(n, gh, gw, 3)
        for k, r in enumerate(boxes_ok):
            c, d = R.compose(pages[0 if k != 1 else 1][0], r.rect, r.paste, r.polygon, r.boxes, gh, gw)
            assert np.array_equal(canv[k], c) and np.array_equal(det[k], d), (gh, gw, k)


def test_bad_arguments_launch_nothing_and_leave_a_message(pages):
    lib = _lib.load()
    gh, gw = 128, 192
    regions = _some_regions(pages)
    n = len(regions)
    stage = engine.RegionStage([regions], torch.device("cuda", 0))
    canv = torch.full((n, gh, gw, 3), 0x5A, dtype=torch.uint8, device="cuda")
    det = torch.full((n, gh, gw, 3), 0x5A, dtype=torch.uint8, device="cuda")
    need = lib.rd_region_canvases_workspace(n, gh, gw)
    assert need >= n * gh * gw and lib.rd_region_canvases_workspace(0, gh, gw) == 0 and lib.rd_region_canvases_workspace(n, 0, gw) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    descs, _pts, _boxes, _f = engine.pack_regions([regions])

    def with_descs(change):
        d = descs.copy()
        change(d)
        return torch.from_numpy(d.view(np.uint8).copy()).cuda()

    def setf(k, field, v):
        def change(d):
            d[field][k] = v
        return change

    over_cap, box_out, box_empty, neg = (with_descs(setf(0, "poly_n", engine.REGION_MAX_POLY + 1)), with_descs(setf(2, "box_off", 0)),
                                         with_descs(setf(0, "box_n", -1)), with_descs(setf(1, "poly_off", -2)))
    # (box_off 0 hands region 2 the boxes [10, 10, 60, 40] - fine - and [0, 0, 192, 3]; on a 64-wide canvas below they leave it)
    cases = {
        "descriptors NULL": lambda: lib.rd_region_canvases(0, None, n, stage.pts_ptr, stage.boxes_ptr, gh, gw, canv.data_ptr(), det.data_ptr(), ws.data_ptr(), need, None),
        "canvases NULL": lambda: _raw(lib, stage, n, gh, gw, None, det.data_ptr(), ws.data_ptr(), need),
        "n = 0": lambda: _raw(lib, stage, 0, gh, gw, canv.data_ptr(), det.data_ptr(), ws.data_ptr(), need),
        "gh = 0": lambda: _raw(lib, stage, n, 0, gw, canv.data_ptr(), det.data_ptr(), ws.data_ptr(), need),
        "gw = -1": lambda: _raw(lib, stage, n, gh, -1, canv.data_ptr(), det.data_ptr(), ws.data_ptr(), need),
        "polygon above the cap": lambda: _raw(lib, stage, n, gh, gw, canv.data_ptr(), det.data_ptr(), ws.data_ptr(), need, over_cap.data_ptr()),
        "negative count": lambda: _raw(lib, stage, n, gh, gw, canv.data_ptr(), det.data_ptr(), ws.data_ptr(), need, box_empty.data_ptr()),
        "negative offset": lambda: _raw(lib, stage, n, gh, gw, canv.data_ptr(), det.data_ptr(), ws.data_ptr(), need, neg.data_ptr()),
        "box outside its canvas": lambda: _raw(lib, stage, n, 64, 64, canv.data_ptr(), det.data_ptr(), ws.data_ptr(), need, box_out.data_ptr()),
        "workspace too small": lambda: _raw(lib, stage, n, gh, gw, canv.data_ptr(), det.data_ptr(), ws.data_ptr(), need - 1),
        "workspace NULL": lambda: _raw(lib, stage, n, gh, gw, canv.data_ptr(), det.data_ptr(), None, 0),
    }
    for name, call in cases.items():
        assert call() == 1, name
        assert len(lib.rd_create_error()) > 20, name
    torch.cuda.synchronize()
    assert bool((canv == 0x5A).all()) and bool((det == 0x5A).all())
    assert b"cap is 64" in (cases["polygon above the cap"](), lib.rd_create_error())[1]
    assert b"leaves the 64 x 64 canvas" in (cases["box outside its canvas"](), lib.rd_create_error())[1]
    with pytest.raises(engine.EngineError):
        engine.region_canvases([Region(pages[0][1], (0, 0, 10, 10), (0, 0), None, [[0, 0, 300, 5]])], (64, 64), True)
    # and the good call on the same buffers does write
    assert _raw(lib, stage, n, gh, gw, canv.data_ptr(), det.data_ptr(), ws.data_ptr(), need) == 0
    torch.cuda.synchronize()
    assert not bool((canv == 0x5A).all())


def test_a_batch_equals_each_region_alone(pages):
    specs = [(p, rect, (50, 50), [[rect[0] + 5, rect[1] + 3], [rect[2] - 4, rect[1] + 9], [rect[2] - 9, rect[3] - 2], [rect[0] + 1, rect[3] - 12]]
              if k % 3 == 0 else None, [(60.5, 60.5, 90, 80)] if k % 2 else []) for k, (p, rect) in enumerate(RECTS)]
    canv, det, _want = _check(pages, specs, 256, 256)
    for k, spec in enumerate(specs):
        c1, d1, _w = _check(pages, [spec], 256, 256)
        assert torch.equal(c1[0], canv[k]) and torch.equal(d1[0], det[k]), k


# ---------------------------------------------------------------------------------------------------------------- the callers
@pytest.fixture(scope="module")
def pipe(golden_dir):
    from rapiddoc_amd.pipeline import PagePipeline
    states = {k: W.synth_state_dict(W.load_manifest(golden_dir / f"manifest_{k}.json"), 0) for k in ("ppocrv6_det", "ppocrv6_rec")}
    return PagePipeline(states, rec_mode="strict", n_rec_streams=2)


def _text(x0, y0, x1, y1, order, polygon=None):
    d = {"category_id": 1, "original_label": "text", "original_order": order, "poly": [x0, y0, x1, y0, x1, y1, x0, y1], "score": 0.9}
    if polygon is not None:
        d["polygon_points"] = polygon
    return d


def _formula(x0, y0, x1, y1):
    return {"category_id": 13, "original_label": "inline_formula", "original_order": 9, "poly": [x0, y0, x1, y0, x1, y1, x0, y1], "score": 0.8}


LINES = [(14, 12, 130, 30), (14, 36, 120, 54), (150, 20, 280, 40), (20, 110, 140, 128), (20, 134, 120, 150)]       # text lines of a page
DETS = [_text(8, 6, 140, 60, 0), _formula(60, 14, 90, 28), _formula(100, 30.5, 135.5, 58), _text(144, 10, 290, 50, 1),
        _text(10, 100, 150, 158, 2, [[12.5, 102], [148, 104], [146, 156], [60, 150.5], [14, 140]]), _text(-6, 160, 70, 196, 3)]


def _run_region_ocr(pipe, pages, dets, route):
    """RegionOcr on one route with text maps drawn from LINES and a spy in the detector seam -> (output, the canvases the detector saw)"""
    from rapiddoc_amd.pipeline import render_text_maps
    seen, held = [], {}
    ocr = analyze.RegionOcr(pipe, compose=route)
    dev = analyze.page_set(pages).device

    def maps_fn(regs, ghw, dhw):
        per_img = []
        for _p, r, useful in regs:
            px, py, x0, y0 = useful[0], useful[1], useful[2], useful[3]
            bb = np.asarray(LINES, dtype=np.float64)
            inside = bb[(bb[:, 0] >= x0) & (bb[:, 2] <= r["poly"][4]) & (bb[:, 1] >= y0) & (bb[:, 3] <= r["poly"][5])]
            per_img.append(inside - [x0 - px, y0 - py, x0 - px, y0 - py])
        held["maps"] = render_text_maps(per_img, ghw, dhw, dev)
        return held["maps"]

    def det_raw_fn(canvases, batch_size):
        assert canvases.is_cuda
        seen.append(canvases.cpu().numpy().copy())
        return ocr._detect_group(canvases, held["maps"], pipe)

    ocr.det_raw_fn = det_raw_fn
    out = ocr(pages, dets, det_maps_fn=maps_fn)
    torch.cuda.synchronize()
    return out, seen


def test_region_ocr_device_route_equals_the_host_route(pipe):
    pages = torch.from_numpy(np.stack([_page(21, 200, 300), _page(22, 200, 300)])).cuda()
    dets = [DETS, DETS[3:] + DETS[:1]]
    out_h, seen_h = _run_region_ocr(pipe, pages, dets, "host")
    out_d, seen_d = _run_region_ocr(pipe, pages, dets, "device")
    assert len(seen_h) == len(seen_d) >= 2 and all(np.array_equal(a, b) for a, b in zip(seen_h, seen_d))
    assert out_h == out_d
    assert sum(1 for pg in out_d for d in pg if d["category_id"] in (15, 16)) >= 6
    assert any((c != 255).any() for c in seen_d)


def test_a_cuda_list_of_two_page_sizes_equals_the_white_padded_tensor_on_the_host_route(pipe):
    a, b = _page(23, 200, 300), _page(24, 170, 130)
    padded = np.full((2, 200, 300, 3), 255, np.uint8)
    padded[0], padded[1, :170, :130] = a, b
    dets = [DETS, [_text(8, 6, 140, 60, 0), _formula(60, 14, 90, 28), _text(20, 110, 140, 128 + 50, 1)]]     # page b: both regions overhang it
    out_t, seen_t = _run_region_ocr(pipe, torch.from_numpy(padded).cuda(), dets, "host")
    out_l, seen_l = _run_region_ocr(pipe, [torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()], dets, "device")
    assert len(seen_t) == len(seen_l) and all(np.array_equal(x, y) for x, y in zip(seen_t, seen_l))
    assert out_t == out_l


def test_table_ocr_result_device_route_equals_the_host_route(pipe):
    from rapiddoc_amd import ocr_host
    from rapiddoc_amd.pipeline import render_text_maps
    page = torch.from_numpy(_page(25, 200, 300)).cuda()
    table = page[20:143, 40:117]                                                  # 123 x 77: an odd width, a window of the page
    adjusted = [{"bbox": [10.5, 8.25, 30.75, 20.5]}, {"bbox": [25, 15, 50, 40]}, {"bbox": [60, 100, 90, 130]}, {"bbox": [-20, -20, -5, -5]}]
    maps = render_text_maps([[(6, 50, 70, 66), (6, 72, 60, 88)]], (123, 77), ocr_host.det_resize_shape(123, 77, 960, "max"), page.device)
    res = {}
    for route in ("host", "device"):
        seen = []
        tocr = analyze.TableOcr(pipe, compose=route, use_word_box=False)

        def det_raw_fn(canvases, batch_size, tocr=tocr, seen=seen):
            seen.append(canvases.cpu().numpy().copy())
            return tocr.det._detect_group(canvases.contiguous(), maps, pipe)

        tocr.det.det_raw_fn = det_raw_fn
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res[route] = (tocr.ocr_result(table, adjusted), seen, tocr.ocr_result(table, None), tocr.ocr_result(table, []))
    torch.cuda.synchronize()
    (rh, sh, nh, eh), (rd, sd, nd, ed) = res["host"], res["device"]
    assert len(sh) == len(sd) == 3 and all(np.array_equal(a, b) for a, b in zip(sh, sd))
    assert (sd[0] != sd[1]).any() and np.array_equal(sd[1], table.cpu().numpy()[None])        # boxes whited out of the first call only
    for a, b in ((rh, rd), (nh, nd), (eh, ed)):
        assert len(a) == len(b) == 3 and len(a[0]) >= 1
        assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1] and a[2] == b[2]
