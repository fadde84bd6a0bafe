"""CPU: a page batch handed to the page driver as a LIST of pages of their own sizes (the reference takes a list of page images,
batch_analyze.py:78-111) - PageAnalyzer / RegionOcr / TableOcr / recognise_formulas / crop_region with stand-ins for every network, as
tests/test_analyze_trace.py does - and the descriptor packing of the device composition route (engine.pack_regions) against a numpy
restatement (tests/region_reference.py) and the host route's own canvases.  No GPU."""
import copy
import zlib

import numpy as np
import pytest
import torch

import region_reference as R
from rapiddoc_amd import analyze, engine
from test_analyze_trace import ReplayFormula, ReplayPipe


def text(x0, y0, x1, y1, order, polygon=None):
    d = {"category_id": 1, "original_label": "text", "original_order": order, "poly": [x0, y0, x1, y0, x1, y1, x0, y1], "score": 0.9}
    if polygon is not None:
        d["polygon_points"] = polygon
    return d


def formula(x0, y0, x1, y1, order):
    return {"category_id": 13, "original_label": "inline_formula", "original_order": order, "poly": [x0, y0, x1, y0, x1, y1, x0, y1], "score": 0.8}


def table(x0, y0, x1, y1, order):
    return {"category_id": 5, "original_label": "table", "original_order": order, "poly": [x0, y0, x1, y0, x1, y1, x0, y1], "score": 0.85}


class FixedLayout:
    def __init__(self, dets):
        self.dets, self.shapes = dets, []

    def batch_predict(self, images, batch_size):
        self.shapes.append([tuple(i.shape) for i in images])
        return copy.deepcopy(self.dets)


class TableModel:
    def __init__(self):
        self.crops = []

    def predict(self, img, ocr_result, fill, adjusted, skip_text_in_image, use_img2table, skip_table_orientation=True):
        self.crops.append((img.shape, zlib.crc32(np.ascontiguousarray(img).tobytes()), len(ocr_result[0]) if ocr_result else 0))
        return f"<html><table><tr><td>{img.shape[0]}x{img.shape[1]}</td></tr></table></html>"


def det_boxes(gh, gw):
    """the detector stand-in's answer for a canvas of gh x gw: two lines inside the 50-px margin"""
    out = [[[60, 58], [min(gw - 55, 190), 58], [min(gw - 55, 190), 74], [60, 74]]]
    if gh >= 150:
        out.append([[62, 84], [120, 84], [120, 98], [62, 98]])
    return np.asarray(out, dtype=np.float32)


def run(pages, dets, **kw):
    """one PageAnalyzer pass with every network stood in for -> (output, log of everything the stand-ins were handed)"""
    log = {"det": [], "table_det": [], "formula": [], "rec": []}

    def det_raw_fn(canvases, batch_size):
        log["det"].append(canvases.numpy().copy())
        return [det_boxes(*canvases.shape[1:3]) for _ in range(canvases.shape[0])]

    def table_det_raw_fn(canvas, batch_size):
        log["table_det"].append(canvas.numpy().copy())
        return [np.asarray([[[4, 4], [40, 4], [40, 16], [4, 16]]], dtype=np.float32)]

    layout, tables = FixedLayout(dets), TableModel()
    pa = analyze.PageAnalyzer(layout, ReplayPipe(log["rec"]), formula_model=ReplayFormula(log["formula"]), table_model=tables, layout_batch_size=2,
                              det_raw_fn=det_raw_fn, table_det_raw_fn=table_det_raw_fn, table_rec_fn=lambda c, q: [("cell", 0.9)] * len(q),
                              table_use_word_box=False, seal_enable=False, **kw)
    out = pa(pages)
    log["layout"], log["tables"], log["labels"] = layout.shapes, tables.crops, pa.last_rotate_labels
    return out, log


def same_log(a, b, keys=("det", "table_det", "formula", "rec", "tables")):
    for k in keys:
        assert len(a[k]) == len(b[k]), k
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, k


def page(seed, h, w):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 255, size=(h, w, 3), dtype=np.uint8))       # (never 255: white is padding only)


POLY = [[20.7, 118.2], [150.1, 112.9], [171.3, 160.0], [90.5, 171.8], [24.0, 165.5]]
# per page: rectangles, a polygon region, a formula inside a text region (whited out of the det copy), a table with a formula inside
DETS_A = [text(12, 10, 180, 60, 0), formula(40, 22, 90, 44, 1), text(15, 110, 175, 175, 2, POLY), table(200, 20, 290, 95, 3),
          formula(220, 40, 250, 60, 4), text(205, 120, 292, 180, 5)]
DETS_B = [text(-8, -6, 120, 70, 0),                       # overhangs the page's left and top edges
          text(100, 150, 260, 245, 1),                    # overhangs the SMALLER page's right and bottom edges (220 x 240)
          formula(30, 90, 80, 112, 2), text(10, 84, 200, 120, 3)]


def test_a_list_of_equal_pages_equals_the_stacked_tensor():
    a, b = page(1, 200, 300), page(2, 200, 300)
    out_t, log_t = run(torch.stack([a, b]), [DETS_A, DETS_A])
    out_l, log_l = run([a, b], [DETS_A, DETS_A])
    assert out_l == out_t and log_l["layout"] == log_t["layout"]
    same_log(log_l, log_t)
    assert len(log_t["det"]) >= 2 and len(log_t["tables"]) == 2 and len(log_t["formula"]) == 1 and sum(len(p) for p in out_t) > 16


def test_a_list_of_two_sizes_equals_the_white_padded_tensor():
    """White padding equals the canvas fill, so every canvas is the same - also for the region that overhangs the smaller page."""
    a, b = page(3, 200, 300), page(4, 240, 220)
    padded = torch.full((2, 240, 300, 3), 255, dtype=torch.uint8)
    padded[0, :200, :300], padded[1, :240, :220] = a, b
    out_t, log_t = run(padded, [DETS_A, DETS_B])
    out_l, log_l = run([a, b], [DETS_A, DETS_B])
    assert log_l["layout"] == [[(200, 300, 3), (240, 220, 3)]] and log_t["layout"] == [[(240, 300, 3)] * 2]
    assert out_l == out_t
    same_log(log_l, log_t)
    # the overhanging region reached the detector with page pixels and white where it leaves the page
    big = [c for c in log_l["det"] if c.shape[1:3] == (256, 320)]
    assert len(big) == 1 and (big[0][0, 50 + 90:, 50 + 120:] == 255).all() and (big[0][0, 50: 50 + 90, 50: 50 + 120] != 255).any()


class Orientation:
    def __init__(self, labels):
        self.labels, self.k = labels, 0

    def predict(self, img):
        self.k += 1
        return self.labels[self.k - 1]


@pytest.mark.parametrize("labels", [["0", "90"], ["270", "180"]])
def test_a_list_may_mix_upright_and_sideways_pages(labels):
    a, b = page(5, 200, 300), page(6, 220, 240)
    turn = {"90": 1, "270": -1}
    upright = [torch.rot90(t, turn[lb], dims=(0, 1)).contiguous() if lb in turn else t for t, lb in zip((a, b), labels)]
    dets = [DETS_A if tuple(upright[0].shape[:2]) == (200, 300) else DETS_B, DETS_B]
    want, log_w = run(upright, dets)
    for t, lb, pg in zip((a, b), labels, want):
        for d in pg:
            d["rotate_label"] = lb
            if lb in turn:
                d["poly"] = analyze.restore_poly(d["poly"], lb, int(t.shape[1]), int(t.shape[0]))
    got, log_g = run([a, b], dets, orientation_model=Orientation(labels), use_doc_orientation_classify=True)
    assert got == want and log_g["labels"] == labels
    assert log_g["layout"] == log_w["layout"] == [[tuple(u.shape) for u in upright]]
    same_log(log_g, log_w)
    # the tensor form still refuses the mix (and only the mix)
    if labels == ["0", "90"]:
        with pytest.raises(NotImplementedError):
            run(torch.stack([a, a]), [DETS_A, DETS_A], orientation_model=Orientation(labels), use_doc_orientation_classify=True)


def test_crop_region_and_formula_crops_use_the_page_s_own_size():
    a, b = page(7, 200, 300), page(8, 120, 100)
    crop = analyze.crop_region([a, b], 1, text(60, 90, 130, 140, 0))           # overhangs page b (120 x 100) only
    assert crop.shape == (50, 70, 3) and (crop[:30, :40] == b.numpy()[90:120, 60:100]).all() and (crop[30:] == 255).all() and (crop[:, 40:] == 255).all()
    log = []
    n = analyze.recognise_formulas([a, b], [[formula(250, 150, 299, 199, 0)], [formula(60, 100, 99, 119, 0)]], ReplayFormula(log))
    # grown by 2 px and stopped at each page's OWN far edges: 248 .. 300 x 148 .. 200 on page a, 58 .. 100 x 98 .. 120 on page b
    assert n == 2 and log[0]["shapes"] == [[52, 52], [22, 42]]


# ---------------------------------------------------------------------------------------------------------------- descriptor packing
def _ocr_regions(pages, dets_per_page, mask_boxes):
    """RegionOcr.__call__'s region list and size groups"""
    from rapiddoc_amd import layout_host, ocr_host
    regions = []
    for p, dets in enumerate(dets_per_page):
        for r in dets:
            useful = layout_host.crop_geometry(r, analyze.PASTE, analyze.PASTE)
            regions.append((p, r, useful, analyze._formula_boxes_in_crop(mask_boxes[p], useful)))
    groups = ocr_host.det_buckets([(u[7], u[6]) for _, _, u, _ in regions], ["ch"] * len(regions), det_batch_num=len(regions))
    return regions, groups


def test_descriptor_packing_against_the_numpy_restatement_and_the_host_route():
    big = page(9, 230, 330)
    pages = [page(10, 200, 300), big[10:190, 20:260]]                               # the second page: a window of a larger buffer
    dets = [[text(20, 30, 120, 90, 0), text(-30, 40, 60, 100, 1), text(250, 20, 340, 80, 2), text(30, -25, 140, 35, 3), text(40, 170, 150, 230, 4),
             text(400, 300, 470, 360, 5), text(100, 100, 101, 101, 6), text(15, 110, 175, 175, 7, POLY), text(-20, 100, 120, 190, 8, POLY)],
            [text(5, 5, 100, 60, 0), text(150, 100, 260, 200, 1, [[140, 90], [250, 120], [230, 210], [160, 170]])]]
    masks = [[{"bbox": [30.4, 35.2, 60.7, 50.1]}, {"bbox": [50, 40, 80, 70]}, {"bbox": [-45.5, 20, 21.5, 95]}, {"bbox": [100, 60, 130, 95.5]},
              {"bbox": [500, 500, 520, 520]}],
             [{"bbox": [0, 0, 30, 20]}]]
    ps = analyze.page_set(pages)
    regions, groups = _ocr_regions(ps, dets, masks)
    chosen, lists = analyze.RegionOcr._device_groups(ps, regions, groups)
    assert chosen == list(range(len(groups))) and len(groups) >= 2
    descs, pts, boxes, firsts = engine.pack_regions(lists)
    assert descs.dtype.itemsize == 64 and len(descs) == len(regions) and firsts == [sum(len(g) for g in lists[:i]) for i in range(len(lists))]
    assert int(descs["poly_n"].sum()) == len(pts) == 5 + 5 + 4 and int(descs["box_n"].sum()) == len(boxes) and len(boxes) > 4
    page_of = {int(t.data_ptr()): t.numpy() for t in pages}
    assert set(descs["pitch"].tolist()) == {900, 990}
    seen = 0
    for gi, (_lang, (gh, gw), members, _bs) in enumerate(groups):
        canv, det = analyze.RegionOcr._compose_host(ps, regions, members, gh, gw)
        mine = R.compose_descs(descs[firsts[gi]: firsts[gi] + len(members)], pts, boxes, page_of, gh, gw)
        for k, (c, d) in enumerate(mine):
            assert np.array_equal(c, canv[k].numpy()) and np.array_equal(d, det[k].numpy()), (gi, k)
            seen += int((c != 255).any()) + 2 * int((c != d).any())
    assert seen >= 3 * 4                                                          # pixels and whited-out boxes really took part
    # the fields of one clipped region, spelled out: page 0's region 1 overhangs the left edge by 30
    k = [i for i, r in enumerate(r for g in lists for r in g) if r.rect == (-30, 40, 60, 100)][0]
    d = descs[k]
    assert (int(d["x0"]), int(d["y0"]), int(d["x1"]), int(d["y1"]), int(d["paste_x"]), int(d["paste_y"]), int(d["page_w"]), int(d["page_h"])) == \
        (-30, 40, 60, 100, 50, 50, 300, 200)


def test_a_polygon_above_the_cap_keeps_its_whole_group_on_the_host():
    ps = analyze.page_set([page(11, 200, 300)])
    many = [[20 + (i % 40), 30 + (i // 2)] for i in range(engine.REGION_MAX_POLY + 1)]
    dets = [[text(20, 30, 120, 90, 0, many), text(22, 32, 122, 92, 1), text(20, 30, 250, 190, 2, many[: engine.REGION_MAX_POLY])]]
    regions, groups = _ocr_regions(ps, dets, [[]])
    chosen, lists = analyze.RegionOcr._device_groups(ps, regions, groups)
    assert len(groups) == 2 and chosen == [1] and len(lists) == 1 and len(lists[0][0].polygon) == engine.REGION_MAX_POLY


def test_the_switch_and_its_override():
    assert analyze.compose_route("host") == "host" and analyze.compose_route("device") == "device"
    assert analyze.compose_route(None) in ("host", "device")
    with pytest.raises(ValueError):
        analyze.compose_route("gpu")
    assert analyze.RegionOcr(None, compose="host").compose == "host" and analyze.TableOcr(None, compose="device").det.compose == "device"
