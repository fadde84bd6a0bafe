"""CPU: what the refilled-slot table decode (rd_table_decode_stream) and the pooled table route need no GPU for - the new symbols, the
constructor checks and the window split of `Mi355UniTableStructure`, `Mi355RapidTable.predict_many` against the `predict` loop on a
stand-in structure model, and `TableOcr(pooled=True)` against the per-table route with stand-in detector, recogniser and table model."""
import copy
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from rapiddoc_amd import table_unitable as TU

ROOT = Path(__file__).resolve().parents[1]
IDS = TU.STAND_IN_IDS


def test_new_symbols_exist_everywhere():
    from rapiddoc_amd import _lib, build as rd_build, engine
    rd_build.build(verbose=False)
    lib = _lib.load()
    header = (ROOT / "include" / "rapiddoc_mi355.h").read_text()
    assert re.search(r"\bint rd_table_decode_stream\s*\(", header) and "typedef struct rd_table_stream_stats" in header
    assert int(re.search(r"#define RD_TABLE_STREAM_MAX_TOKENS (\d+)", header).group(1)) == engine.TABLE_STREAM_MAX_TOKENS == 65536
    assert int(re.search(r"#define RD_TABLE_STREAM_MAX_SLOTS (\d+)", header).group(1)) == engine.TABLE_STREAM_MAX_SLOTS == TU.MAX_SLOTS == 8
    assert "rd_table_decode_stream" in _lib.SYMBOLS and "rd_debug_table_decode_stream" in _lib.DEBUG_SYMBOLS
    assert len(_lib.SYMBOLS["rd_table_decode_stream"][1]) == 11 and len(_lib.DEBUG_SYMBOLS["rd_debug_table_decode_stream"][1]) == 15
    assert hasattr(lib, "rd_table_decode_stream") and hasattr(lib, "rd_debug_table_decode_stream")
    assert "rd_debug_table_decode_stream" in (ROOT / "rapiddoc_amd" / "csrc" / "api_debug.cpp").read_text()
    assert "rd_debug_table_decode_stream" in (ROOT / "tools" / "README.md").read_text()
    assert C.sizeof(engine.TableStreamStats) == 16
    assert lib.rd_table_decode_stream(None, None, 1, 1, 1, 1, None, None, None, None, None) != 0          # no handle: refused, nothing touched
    assert callable(engine.RdEngine.table_decode_stream)


def test_constructor_checks_its_arguments():
    toks = TU.stand_in_tokens()
    with pytest.raises(ValueError, match="batching"):
        TU.Mi355UniTableStructure({}, {}, IDS, toks, batching="rows")
    for bad in (0, 9, -1, 2.5, "3", None, True):
        with pytest.raises(ValueError, match="slots"):
            TU.Mi355UniTableStructure({}, {}, IDS, toks, batching="stream", slots=bad)
    with pytest.raises(ValueError, match="slots"):                  # checked whatever the batching is
        TU.Mi355UniTableStructure({}, {}, IDS, toks, slots=0)
    with pytest.raises(ValueError, match="resize"):
        TU.Mi355UniTableStructure({}, {}, IDS, toks, resize="cubic", batching="stream")


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_valid_arguments_reach_the_engine_and_fail_loudly_without_a_gpu():
    from rapiddoc_amd.engine import EngineError
    with pytest.raises(EngineError):
        TU.Mi355UniTableStructure({}, {}, IDS, TU.stand_in_tokens(), batching="stream", slots=np.int64(3))


def test_window_split_for_the_token_limit():
    from rapiddoc_amd.engine import TABLE_STREAM_MAX_TOKENS as T
    assert TU.stream_windows(0, 784, T) == []
    assert TU.stream_windows(5, 784, T) == [(0, 5)]
    per = T // 784
    assert per == 83 and per * 784 <= T < (per + 1) * 784
    assert TU.stream_windows(per, 784, T) == [(0, per)] and TU.stream_windows(per + 1, 784, T) == [(0, per), (per, per + 1)]
    w = TU.stream_windows(3 * per + 2, 784, T)
    assert w == [(0, per), (per, 2 * per), (2 * per, 3 * per), (3 * per, 3 * per + 2)] and all((e - b) * 784 <= T for b, e in w)
    assert TU.stream_windows(7, 1024, T) == [(0, 7)] and TU.stream_windows(65, 1024, T) == [(0, 64), (64, 65)]
    assert TU.stream_windows(7, 3, 7) == [(0, 2), (2, 4), (4, 6), (6, 7)]
    with pytest.raises(ValueError):
        TU.stream_windows(1, T + 1, T)


# ---------------------------------------------------------------------------------------------------------------- predict_many
class _Structure:
    """a structure model of the class's shape that needs no GPU: `decode_ids` returns prepared contexts and counts its calls"""
    resize = "pil"

    def __init__(self, ids, fail_pooled=False):
        self.ids, self.calls, self.fail_pooled = ids, [], fail_pooled
        self.id_to_token = TU.stand_in_tokens()

    def preprocess(self, imgs):
        return torch.zeros((len(imgs), 3, 4, 4)), [tuple(int(v) for v in im.shape[:2]) for im in imgs]

    def decode_ids(self, x):
        self.calls.append(int(x.shape[0]))
        if self.fail_pooled and x.shape[0] > 1:
            raise RuntimeError("the pooled structure call")
        return [list(self.ids) for _ in range(x.shape[0])]

    finish = TU.Mi355UniTableStructure.finish

    def __call__(self, imgs):
        x, shapes = self.preprocess(imgs)
        return self.finish(self.decode_ids(x), shapes)


def _items(golden_dir):
    """five tables on the recorded ids of tests/golden/table_path_match.json; table 1 has no OCR rows, table 3's first text is RAISE"""
    import json
    inj = json.loads((golden_dir / "table_path_match.json").read_text())["engine_inject"]
    oh, ow = inj["ori_hw"]
    items = []
    for k, (h, w) in enumerate([(120, 300), (90, 200), (150, 260), (100, 240), (64, 330)]):
        quads, texts, scores = copy.deepcopy(inj["ocr_result"])
        quads = [[[px * w / ow, py * h / oh] for px, py in q] for q in quads]
        texts = [f"{t} #{k}" for t in texts]
        if k == 3:
            texts[0] = "RAISE"
        rgb = np.full((h, w, 3), 200 + k, dtype=np.uint8)
        items.append((rgb, [] if k == 1 else [quads, texts, scores], [], [], True, False, True))
    return inj, items


@pytest.mark.parametrize("fail_pooled", [False, True])
def test_predict_many_equals_the_predict_loop(golden_dir, monkeypatch, fail_pooled):
    from rapiddoc_amd import table_match as TM
    inj, items = _items(golden_dir)
    real_match = TM.match_tables

    def match_tables(pred_structures, cell_bboxes, dt_boxes, rec_res, **kw):
        if any(t == "RAISE" for res in rec_res for t, _s in res):
            raise RuntimeError("the matcher of table 3")
        return real_match(pred_structures, cell_bboxes, dt_boxes, rec_res, **kw)
    monkeypatch.setattr(TM, "match_tables", match_tables)
    loop_st, many_st = _Structure(inj["ids"]), _Structure(inj["ids"], fail_pooled)
    loop_items, many_items = copy.deepcopy(items), copy.deepcopy(items)
    want = [TU.Mi355RapidTable(loop_st).predict(*it) for it in loop_items]
    got = TU.Mi355RapidTable(many_st).predict_many(many_items)
    assert got == want and got[1] is None and got[3] is None
    assert all(isinstance(got[k], str) and f"#{k}" in got[k] for k in (0, 2, 4)) and len({got[0], got[2], got[4]}) == 3
    assert loop_st.calls == [1, 1, 1, 1]
    assert many_st.calls == ([4, 1, 1, 1, 1] if fail_pooled else [4])      # ONE structure call; if it raises, the loop
    for a, b in zip(loop_items, many_items):                               # the caller's OCR lists grow as `predict` grows them, once
        assert a[1] == b[1]
    assert TU.Mi355RapidTable(many_st).predict_many([]) == [] and TU.Mi355RapidTable(many_st).predict_many([items[1]]) == [None]
    with pytest.raises(NotImplementedError, match="img2table"):
        TU.Mi355RapidTable(many_st).predict_many([items[0][:5] + (True, True)])
    with pytest.raises(NotImplementedError, match="rotation"):
        TU.Mi355RapidTable(many_st).predict_many([(np.zeros((100, 50, 3), np.uint8), None)])


# ---------------------------------------------------------------------------------------------------------------- TableOcr(pooled=True)
class _TableModel:
    """records its calls; the answer names the crop's size and its OCR texts"""

    def __init__(self):
        self.predict_calls, self.many_calls = [], []

    def predict(self, image, ocr_result, fill, mfd, skip_text_in_image, use_img2table, skip_table_orientation=None):
        rows = [[np.asarray(q).tolist() for q in ocr_result[0]], list(ocr_result[1]), [float(v) for v in ocr_result[2]]] if ocr_result else []
        self.predict_calls.append((image.shape, int(image.sum()), rows, copy.deepcopy(fill), copy.deepcopy(mfd), skip_text_in_image, use_img2table,
                                   skip_table_orientation))
        if not ocr_result:
            return None
        return f"<html><body><table><tr><td>{image.shape[0]}x{image.shape[1]} {' '.join(ocr_result[1])}</td></tr></table></body></html>"


class _PooledTableModel(_TableModel):
    def predict_many(self, items):
        self.many_calls.append(len(items))
        return [self.predict(*it) for it in items]


def _pages_and_dets():
    rng = np.random.default_rng(5)
    pages = torch.from_numpy(rng.integers(0, 256, (2, 400, 600, 3), dtype=np.uint8))
    box = lambda x0, y0, x1, y1: [x0, y0, x1, y0, x1, y1, x0, y1]
    dets = [[{"category_id": 5, "poly": box(20, 30, 300, 180), "score": 0.9,
              "layout_image_list": [{"category_id": 3, "poly": box(40, 50, 90, 100), "score": 0.8}]},
             {"category_id": 13, "poly": box(100, 60, 160, 90), "score": 0.9, "latex": "x^2"},
             {"category_id": 5, "poly": box(310, 200, 590, 390), "score": 0.9},
             {"category_id": 1, "poly": box(10, 5, 200, 25), "score": 0.9}],
            [{"category_id": 5, "poly": box(0, 0, 600, 400), "score": 0.9},
             {"category_id": 5, "poly": box(50, 50, 50, 90), "score": 0.9},                  # an empty box: skipped
             {"category_id": 5, "poly": box(300, 300, 420, 380), "score": 0.9}]]
    return pages, dets


def _run(model, pooled):
    from rapiddoc_amd.analyze import TableOcr
    pages, dets = _pages_and_dets()
    n_det = [0]

    def det_raw_fn(canvas, n):
        n_det[0] += 1
        h, w = int(canvas.shape[1]), int(canvas.shape[2])
        if (h, w) == (80, 120):
            return [np.zeros((0, 4, 2), np.float32)]                 # nothing detected on the small table: an empty OCR list
        return [np.array([[[5, 5], [w // 2, 5], [w // 2, 25], [5, 25]], [[5, 40], [w - 10, 40], [w - 10, 60], [5, 60]]], np.float32)]

    rec_fn = lambda canvas, quads: [(f"t{int(canvas.shape[2])}_{i}", 0.9 - 0.1 * i) for i in range(len(quads))]
    ocr = TableOcr(None, det_raw_fn=det_raw_fn, rec_fn=rec_fn, use_word_box=False, pooled=pooled)
    n = ocr(pages, dets, model, page_scales=[2.0, 1.0])
    return n, dets, n_det[0]


def test_pooled_table_ocr_writes_what_the_per_table_route_writes():
    loop_model, pooled_model = _PooledTableModel(), _PooledTableModel()
    n0, want, det0 = _run(loop_model, pooled=False)
    n1, got, det1 = _run(pooled_model, pooled=True)
    assert n0 == n1 == 4 and det0 == det1 == 4
    assert loop_model.many_calls == [] and pooled_model.many_calls == [4], "one predict_many call per page batch"
    assert pooled_model.predict_calls == loop_model.predict_calls          # the same arguments, in page / layout order
    assert got == want
    tables = [d for page in got for d in page if d["category_id"] == 5]
    assert [("html" in t) for t in tables] == [True, True, True, False, False]
    assert tables[0]["html"].startswith("<table><tr><td>150x280 t280_0 t280_1") and tables[0]["html"].endswith("</table>")
    assert tables[0]["formula_boxes"] == [[50, 30, 80, 45]] and tables[0]["img_boxes"] == [[20, 25, 45, 50]]
    assert "formula_boxes" not in tables[2] and all("layout_image_list" not in t for t in tables)
    assert loop_model.predict_calls[0][4] == [{"bbox": [80, 30, 140, 60], "latex": "x^2"}] and loop_model.predict_calls[0][7] is True


def test_a_model_without_predict_many_takes_the_per_table_loop():
    plain = _TableModel()
    n, got, _ = _run(plain, pooled=True)
    _n, want, _ = _run(_PooledTableModel(), pooled=False)
    assert n == 4 and len(plain.predict_calls) == 4 and got == want


def test_page_analyzer_hands_table_pooled_to_its_table_stage():
    from rapiddoc_amd.analyze import PageAnalyzer, TableOcr
    import inspect
    assert inspect.signature(TableOcr.__init__).parameters["pooled"].default is False
    assert inspect.signature(PageAnalyzer.__init__).parameters["table_pooled"].default is False
    assert PageAnalyzer(None, None, table_pooled=True).table_ocr.pooled is True and PageAnalyzer(None, None).table_ocr.pooled is False
