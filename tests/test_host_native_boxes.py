"""CPU: `rd_text_boxes_order_merge` (box ordering + same-line merge of a whole batch in one library call) returns exactly what the
Python restatement `merge_det_boxes(sorted_boxes(.))` returns on the same records: the same count and the same float32 bits."""
import json
from pathlib import Path

import numpy as np
import pytest

from rapiddoc_amd import ocr_host as H

GOLDEN = Path(__file__).resolve().parent / "golden"


def records_of(pages, max_in=None):
    """pages: per page an array [k, 4, 2] -> (TEXT_BOX_DTYPE records [B, max_in], counts); the slots behind a page's count hold junk."""
    max_in = max_in or max([len(p) for p in pages] + [1])
    rec = np.zeros((len(pages), max_in), H.TEXT_BOX_DTYPE)
    rec["pts"] = 12345.0
    rec["score"] = -1.0
    for b, p in enumerate(pages):
        rec["pts"][b, :len(p)] = np.asarray(p, np.float32).reshape(-1, 8)
    return rec, np.array([len(p) for p in pages], np.int32)


def python_path(rec, counts):
    """What PagePipeline.boxes_from_maps_device does with RD_HOST_NATIVE=0."""
    out = []
    for b, k in enumerate(counts.tolist()):
        boxes = rec["pts"][b, :k].reshape(k, 4, 2).astype(np.int32)
        q = H.merge_det_boxes(H.sorted_boxes(boxes.astype(np.float32))) if k else []
        out.append(np.asarray(q, dtype=np.float32).reshape(-1, 4, 2))
    return out


def assert_same(pages, max_in=None):
    rec, counts = records_of(pages, max_in)
    want = python_path(rec, counts)
    got = H.order_merge_boxes_native(rec, counts)
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and g.shape == w.shape, (b, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (b, g.tolist(), w.tolist())
    return got


def quad(x, y, w, h, s=0):
    """tl (x, y), bl (x, y + h), right side shifted down by s: mean side height h, diagonal's vertical extent h + s."""
    return [[x, y], [x + w, y + s], [x + w, y + s + h], [x, y + h]]


def branch_page(rng):
    """Integer boxes in rows, sized to sit ON the thresholds of the two functions: top-left y 9 / 10 / 11 apart (the `< 10` row rule),
    equal x (sort ties), heights that are multiples of 5 with the diagonal extent at exactly 0.8 x / 1.2 x the height and one pixel
    beyond (tilt test), neighbours overlapping in y by exactly 0.6 of the smaller height and one pixel either side, boxes and lines
    exactly 4 x as wide as high, x intervals that touch, overlap, nest and miss by one pixel."""
    quads = []
    y = int(rng.integers(0, 40))
    for _ in range(int(rng.integers(0, 9))):
        h = int(rng.choice([5, 10, 15, 20, 25, 40]))
        x = int(rng.choice([0, 5, 50]))
        for _ in range(int(rng.integers(1, 6))):
            w = int(rng.choice([4 * h, 4 * h - 1, 4 * h + 1, h, 2 * h, 3 * h, 30, 100, 250]))
            hh = int(rng.choice([h, h, h, h + 5, max(5, h - 5)]))
            f = hh // 5                                    # 0.2 x the height
            s = int(rng.choice([0, 0, 0, 0, 0, 0, -f, f, -f - 1, f + 1, -f + 1, f - 1, 3 * f]))
            ov = 3 * min(h, hh) // 5                       # 0.6 x the smaller height of two boxes of this row
            dy = int(rng.choice([0, 0, 0, 1, h - ov, h - ov - 1, h - ov + 1, 9, 10, 11]))
            quads.append(quad(x, y + dy, w, hh, s))
            x += int(rng.choice([w, w + 1, w - 5, w + 10, 0, w // 2, w + 40]))       # touch, miss by one, overlap, gap, x tie, nest
        y += int(rng.choice([9, 10, 11, 0, 3, h, h + 6, 2 * h + 13]))
    quads = np.asarray(quads, np.float32).reshape(-1, 4, 2)
    return quads[rng.permutation(len(quads))]


@pytest.mark.parametrize("seed", range(5))
def test_golden_inputs(seed):
    """The inputs the restatement itself is pinned to the reference with (fractional coordinates: the truncation toward zero counts)."""
    g = json.loads((GOLDEN / f"boxes_seed{seed}.json").read_text())
    quads = np.array(g["quads"], dtype=np.float32).reshape(-1, 4, 2)
    got = assert_same([quads, -quads, quads[::-1] + 0.75])[0]
    assert len(got) > 0


def test_empty_page_one_box_and_a_batch_with_both():
    got = assert_same([np.zeros((0, 4, 2)), [quad(10, 20, 200, 20)], np.zeros((0, 4, 2)), [quad(10, 20, 200, 20, 9)]], max_in=7)
    assert [g.shape for g in got] == [(0, 4, 2), (1, 4, 2), (0, 4, 2), (1, 4, 2)]
    assert H.order_merge_boxes_native(np.zeros((0, 4), H.TEXT_BOX_DTYPE), np.zeros(0, np.int32)) == []


def test_a_thousand_boxes_on_one_page():
    rng = np.random.default_rng(7)
    quads = [quad(int(rng.integers(0, 1100)), int(rng.integers(0, 1600)), int(rng.integers(5, 300)), int(rng.choice([10, 20, 30])),
                  int(rng.choice([0, 0, 0, 2, 7]))) for _ in range(1000)]
    got = assert_same([quads], max_in=1000)[0]
    assert 0 < len(got) <= 1000


def test_random_pages_on_the_thresholds():
    rng = np.random.default_rng(2024)
    pages = [branch_page(rng) for _ in range(240)]
    got = assert_same(pages)
    # the generator reaches every branch: merged lines, unmerged lines, tilted boxes, rows re-ordered by the swap pass
    n_in, n_out = sum(len(p) for p in pages), sum(len(g) for g in got)
    assert n_in > 2000 and 0.3 * n_in < n_out < n_in
    tilted = sum(H.quad_is_tilted(q) for p in pages for q in p)
    assert 0.05 * n_in < tilted < 0.6 * n_in
    for fn in (lambda q: (q[2][1] - q[0][1]) * 5 == 4 * (q[3][1] - q[0][1]), lambda q: (q[2][1] - q[0][1]) * 5 == 6 * (q[3][1] - q[0][1]),
               lambda q: q[1][0] - q[0][0] == 4 * (q[3][1] - q[0][1])):
        assert sum(bool(fn(q)) for p in pages for q in p) > 20          # boxes exactly on 0.8 x, 1.2 x and 4 x


def test_bad_counts_are_refused():
    from rapiddoc_amd import _lib
    lib = _lib.load()
    rec, _counts = records_of([[quad(0, 0, 10, 10)]], max_in=2)
    out, n = np.zeros((1, 2, 4, 2), np.float32), np.zeros(1, np.int32)
    for bad in (-1, 3):
        c = np.array([bad], np.int32)
        assert lib.rd_text_boxes_order_merge(rec.ctypes.data, c.ctypes.data, 1, 2, out.ctypes.data, n.ctypes.data) == 1
