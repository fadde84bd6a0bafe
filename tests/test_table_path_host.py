"""CPU: the host side of the table path - the new C entry in the header / symbol table / source list, the numpy restatement of Pillow's
antialiased resample against every resample fixture (and against Pillow itself where it imports), the library's own coefficient tables
against that restatement, `table_match` against every matcher / predict fixture recorded from the reference, the `None` cases, the CJK
cell-text rules on hand-written cases and the two unsupported switches."""
import ctypes as C
import copy
import json
from pathlib import Path

import numpy as np
import pytest

import table_path_reference as TP
from rapiddoc_amd import table_match as TM
from rapiddoc_amd import table_unitable as TU
from rapiddoc_amd import weights as W

ROOT = Path(__file__).resolve().parents[1]
BIG = ("table_path_resample_448_600x1000.npz", "table_path_resample_448_120x300.npz")


def _cases(golden_dir):
    out = TP.resample_cases(golden_dir)
    for fn in BIG:
        z = np.load(golden_dir / fn)
        name = str(z["names"][0])
        seed, h, w = (int(v) for v in z[name + "_recipe"])
        out.append((name, W.synth_table_crop(seed, h, w), 448, 448, z[name + "_exp"]))
    return out


def test_new_entry_is_in_the_header_the_symbol_table_and_the_sources():
    from rapiddoc_amd import _lib, build
    header = (ROOT / "include" / "rapiddoc_mi355.h").read_text()
    assert "int rd_preproc_resize_aa_norm(int device_id, const uint8_t* hwc_u8_dev, int H, int W, int OH, int OW" in header
    assert "#define RD_RESIZE_AA_MAX_SIDE 16384" in header
    res, args = _lib.SYMBOLS["rd_preproc_resize_aa_norm"]
    assert res is C.c_int and len(args) == 12
    assert "kernels_resize_aa.hip" in build.SOURCES and (build.CSRC / "kernels_resize_aa.hip").exists()


def test_fixture_set_holds_the_cases_the_kernel_can_go_wrong_at(golden_dir):
    shapes = {(src.shape[0], src.shape[1], oh, ow) for _n, src, oh, ow, _e in _cases(golden_dir)}
    assert shapes == {(53, 131, 24, 40), (9, 11, 24, 40), (24, 97, 24, 40), (61, 40, 24, 40), (24, 40, 24, 40), (5, 400, 24, 40), (1, 1, 24, 40),
                      (600, 1000, 448, 448), (120, 300, 448, 448)}


def test_numpy_restatement_equals_every_resample_fixture(golden_dir):
    for name, src, oh, ow, exp in _cases(golden_dir):
        got = TP.resize_aa_u8(src, oh, ow)
        assert got.shape == exp.shape and np.array_equal(got, exp), name
    ident = [c for c in _cases(golden_dir) if c[0] == "identity"][0]
    assert np.array_equal(ident[1], ident[4])


def test_numpy_restatement_equals_pillow_on_ten_shapes():
    Image = pytest.importorskip("PIL.Image")
    for i, (h, w) in enumerate(TP.PIL_SHAPES):
        a = W.synth_table_crop(3 + i, h, w) if i % 2 else (W.synth_table_crop(3 + i, h, w) ^ TP.lcg_bytes(i, (1, 1, 3)))
        ref = np.asarray(Image.fromarray(a).resize((448, 448), Image.BILINEAR))
        assert np.array_equal(TP.resize_aa_u8(a, 448, 448), ref), (h, w)


@pytest.mark.parametrize("n_in,n_out", [(1000, 448), (600, 448), (131, 40), (53, 24), (11, 40), (9, 24), (400, 40), (5, 24), (1, 40), (2011, 448), (7, 448),
                                        (16384, 3), (3, 1000)])
def test_library_tables_equal_the_restatement(n_in, n_out):
    """the tables the device reads (host code of kernels_resize_aa.hip, developer entry rd_debug_resize_aa_coeffs) against the Python doubles"""
    from rapiddoc_amd import _lib
    lib = _lib.load()
    fn = lib.rd_debug_resize_aa_coeffs
    bounds, kk, ksize = TP.aa_coeffs(n_in, n_out)
    b = np.full((n_out, 2), -1, dtype=np.int32)
    k = np.full((n_out, ksize), -1, dtype=np.int32)
    assert fn(n_in, n_out, b.ctypes.data, k.ctypes.data, k.size) == ksize
    assert np.array_equal(b, bounds) and np.array_equal(k, kk)
    assert int(b[:, 0].min()) >= 0 and int((b[:, 0] + b[:, 1]).max()) <= n_in and int(b[:, 1].max()) <= ksize and int(b[:, 1].min()) >= 1
    assert fn(n_in, n_out, b.ctypes.data, k.ctypes.data, k.size - 1) == -1
    assert fn(0, n_out, b.ctypes.data, k.ctypes.data, k.size) == -1 and fn(n_in, 16385, b.ctypes.data, k.ctypes.data, k.size) == -1


# ------------------------------------------------------------------------------------------------------------------ matcher
def _match(golden_dir):
    return json.loads((golden_dir / "table_path_match.json").read_text())


def test_matcher_fixture_set(golden_dir):
    cases = _match(golden_dir)["cases"]
    assert set(cases) == {"spans_8pt", "several_in_one_cell_bold", "above_first_cell_and_under_iou", "equal_iou_decided_by_distance", "more_than_256_boxes",
                          "four_point_cells_int_boxes"}
    assert len(cases["more_than_256_boxes"]["ocr_result"][0]) > TM.MATCH_CHUNK == 256 and TM.MIN_IOU == 0.1 ** 8
    assert len(cases["spans_8pt"]["cell_bboxes"][0]) == 8 and len(cases["four_point_cells_int_boxes"]["cell_bboxes"][0]) == 4
    assert all(c["html"].count("<td") > 0 for c in cases.values())


@pytest.mark.parametrize("name", ["spans_8pt", "several_in_one_cell_bold", "above_first_cell_and_under_iou", "equal_iou_decided_by_distance",
                                  "more_than_256_boxes", "four_point_cells_int_boxes"])
def test_matcher_reproduces_the_reference(golden_dir, name):
    c = _match(golden_dir)["cases"][name]
    dt, rec = TM.format_ocr_results(c["ocr_result"], *c["img_hw"])
    assert np.asarray(dt).tolist() == c["dt_boxes"]
    struct = [(c["structure"], 1.0)]
    html = TM.match_tables(struct, [np.array(c["cell_bboxes"], dtype=np.float32)], [dt], [rec])
    assert html == [c["html"]]
    assert [p.tolist() for p in TM.decode_logic_points(struct)] == [c["logic_points"]]


def test_tie_order_and_threshold_by_hand():
    cells = np.array([[0, 0, 100, 50], [100, 5, 200, 55], [0, 60, 100, 110], [100, 60, 200, 110]], dtype=np.float32)
    dt = np.array([[80, 10, 120, 40], [80, 70, 120, 100], [500, 500, 600, 600]], dtype=np.float64)
    assert TM.match_result(cells, dt) == {1: [0], 2: [1]}           # equal IoU: the nearer cell; equal distance too: the lowest index; no overlap: none
    assert TM.match_result(cells, np.zeros((0, 4))) == {} and TM.match_result(np.zeros((0, 4)), dt) == {}
    assert TM.match_tables([(["<tr>", "<td></td>", "</tr>"], 1.0)], [cells[:1]], [None], [None]) == [None]


@pytest.mark.parametrize("name", ["plain", "fill_skip", "fill_keep", "formulas", "fill_and_formulas"])
def test_predict_list_preparation_reproduces_the_reference(golden_dir, name):
    c = _match(golden_dir)["predict_prep"][name]
    rgb = np.empty((*c["image_hw"], 3), dtype=np.uint8)
    rgb[:] = c["image_rgb"]
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])
    kw = c["kwargs"]
    ocr = TM.prepare_ocr_list(bgr, copy.deepcopy(c["ocr_in"]), kw.get("fill_image_res"), kw.get("mfd_res"), kw.get("skip_text_in_image", True))
    assert json.loads(json.dumps(ocr, default=lambda a: np.asarray(a).tolist())) == c["ocr_out"]
    white = np.argwhere((bgr == 255).all(axis=2))
    assert len(white) == c["white_pixels"] and bgr[0, 0].tolist() == c["bgr_corner"]
    if c["white_box_yx"]:
        assert [white.min(axis=0).tolist(), white.max(axis=0).tolist()] == c["white_box_yx"]


def test_fill_white_has_both_corner_pixels_inside():
    img = np.zeros((10, 12, 3), dtype=np.uint8)
    TM.fill_white(img, [3.9, 2.2, 6.7, 4.0])
    ys, xs = np.nonzero(img[:, :, 0])
    assert (ys.min(), ys.max(), xs.min(), xs.max()) == (2, 4, 3, 6) and int((img == 255).all(axis=2).sum()) == 12
    TM.fill_white(img, [20, 20, 30, 30])                    # outside: nothing
    assert int((img == 255).all(axis=2).sum()) == 12
    TM.fill_white(img, [11, 9, 8, 8])                       # corners in the other order, clipped at the border
    assert img[8:10, 8:12].min() == 255


def test_ocr_text_normalisation():
    assert [TM.normalize_table_ocr_text(t) for t in (None, 7, " a & b ", "香", "哦樂", "5號", "10號", "第6號", "<b>x</b>")] == \
        ["", "7", "a &amp; b", "否", "哦", "5", "10號", "第6號", "&lt;b&gt;x&lt;/b&gt;"]


def test_cjk_cell_text_rules_by_hand():
    n = TM.normalize_table_cell_text
    assert n("plain text stays") == "plain text stays" and n("") == "" and n(None) is None
    assert n("合 计 金 额") == "合计金额"
    assert n("金额 ， 共 5 元") == "金额，共5元"
    assert n("第 3 季度 Q3 报告") == "第3季度Q3报告"
    assert n("A b 中") == "A b中"                               # Latin next to Latin keeps its blank
    assert n("价格 $ 5") == "价格$ 5"
    html, toks = TM.get_pred_html(["<tr>", "<td></td>", "<td", ' colspan="2"', ">", "</td>", "</tr>"], {0: [0, 1], 1: [2]},
                                  [("合 计", 1.0), ("金 额", 1.0), ("a b", 1.0)], cell_text=n)
    assert html == '<tr><td>合计金额</td><td colspan="2">a b</td></tr>'


# ------------------------------------------------------------------------------------------------------------------ the predict-shaped class
class _Structure:
    """a structure model of the class's shape that needs no GPU: returns a prepared (structure, boxes)"""
    resize = "pil"

    def __init__(self, tokens, boxes):
        self.tokens, self.boxes, self.calls = tokens, boxes, 0

    def __call__(self, imgs):
        self.calls += 1
        self.seen = [np.array(i) for i in imgs]
        return [(TU.wrap_with_html_struct(list(self.tokens)), 1.0) for _ in imgs], [np.array(self.boxes, dtype=np.float32) for _ in imgs]


def test_class_runs_the_matcher_behind_the_structure_model(golden_dir):
    c = _match(golden_dir)["cases"]["several_in_one_cell_bold"]
    st = _Structure(c["structure"][3:-3], c["cell_bboxes"])
    model = TU.Mi355RapidTable(st)
    rgb = np.full((*c["img_hw"], 3), 200, dtype=np.uint8)
    out = model([rgb], [copy.deepcopy(c["ocr_result"])])
    assert out.pred_htmls == [c["html"]] and [p.tolist() for p in out.logic_points] == [c["logic_points"]] and len(out.cell_bboxes) == 1
    assert model.predict(rgb, copy.deepcopy(c["ocr_result"])) == c["html"]
    assert model.batch_predict([rgb, rgb], copy.deepcopy(c["ocr_result"])) == [c["html"]] * 2


def test_predict_whites_out_fill_boxes_in_the_bgr_image_it_hands_on():
    st = _Structure(["<tr>", "<td></td>", "</tr>"], [[0, 0, 60, 40]])
    model = TU.Mi355RapidTable(st)
    rgb = np.empty((40, 60, 3), dtype=np.uint8)
    rgb[:] = (7, 90, 180)
    ocr = [[[[2.0, 2.0], [20.0, 2.0], [20.0, 10.0], [2.0, 10.0]]], ["a"], [0.9]]
    html = model.predict(rgb, ocr, fill_image_res=[{"ocr_bbox": [[20, 10], [35, 10], [35, 30], [20, 30]], "uuid": "u1"}])
    assert html == "<html><body><table><tr><td>a u1</td></tr></table></body></html>"
    assert st.seen[0][0, 0].tolist() == [180, 90, 7] and st.seen[0][10:31, 20:36].min() == 255 and st.seen[0][9, 20].tolist() == [180, 90, 7]
    assert rgb.max() == 180 and ocr[1] == ["a", "u1"]           # the caller's image stays, the caller's list grows as in the reference


def test_none_cases():
    st = _Structure([], np.zeros((0,), dtype=np.float32))           # a structure without a cell: the matcher raises, predict returns None
    model = TU.Mi355RapidTable(st)
    rgb = np.zeros((40, 60, 3), dtype=np.uint8)
    ocr = [[[[2.0, 2.0], [20.0, 2.0], [20.0, 10.0], [2.0, 10.0]]], ["a"], [0.9]]
    assert model.predict(rgb, copy.deepcopy(ocr)) is None and st.calls == 1
    with pytest.raises((ValueError, IndexError)):
        TM.filter_ocr_result(np.zeros((0, 8), dtype=np.float32), [np.zeros(4)], [("a", 1.0)])
    for empty in (None, [], ()):
        assert model.predict(rgb, empty) is None
    assert st.calls == 1                                            # nothing ran for an empty OCR list


def test_unsupported_switches_raise():
    model = TU.Mi355RapidTable(_Structure([], []))
    rgb = np.zeros((100, 50, 3), dtype=np.uint8)                    # portrait: 2.0 > 1.2
    ocr = [[[[2.0, 2.0], [20.0, 2.0], [20.0, 10.0], [2.0, 10.0]]], ["a"], [0.9]]
    with pytest.raises(NotImplementedError, match="img2table"):
        model.predict(rgb, ocr, use_img2table=True)
    with pytest.raises(NotImplementedError, match="rotation"):
        model.predict(rgb, ocr, skip_table_orientation=False)
    with pytest.raises(NotImplementedError, match="rotation"):
        model.predict(rgb, None)                                    # no OCR list: the reference would look at the orientation first
    with pytest.raises(ValueError, match="pil"):
        st = _Structure([], [])
        st.resize = "linear"
        TU.Mi355RapidTable(st)


def test_class_pil_expectation_is_consistent(golden_dir):
    exp = TP.load_summary(golden_dir)["class_pil"]
    ids = TU.STAND_IN_IDS
    assert exp["ids"][0] == ids.prefix and exp["ids"][-1] == ids.eos and 22 <= len(exp["ids"]) <= 62 and exp["crop_hw"] == [600, 1000]
    boxes, html = TU.decode_tokens(exp["ids"], TU.stand_in_tokens())
    assert html == exp["html"] and TU.wrap_with_html_struct(html) == exp["wrapped"]
    assert (TU.rescale_bboxes(600, 1000, boxes).tolist() if len(boxes) else boxes.tolist()) == exp["boxes"]
    assert tuple(exp["rule"]) in ((0.25, 0.05), (0.1, 0.02))
