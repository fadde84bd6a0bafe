"""CPU: `rd_rec_plan_lines` (reference widths, chunk ratios and launches of the strict mode in one library call) returns exactly what
the Python loops of `rec_batches_lines` return - `native=False`, the path RD_HOST_NATIVE=0 selects."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from rapiddoc_amd import ocr_host as H

ROOT = Path(__file__).resolve().parents[1]


def assert_same(ratios, **kw):
    want = H.rec_batches_lines(ratios, with_ratio=True, native=False, **kw)
    got = H.rec_batches_lines(ratios, with_ratio=True, native=True, **kw)
    assert len(got[0]) == len(want[0])
    for (gi, gw), (wi, ww) in zip(got[0], want[0]):
        assert np.array_equal(gi, wi) and type(gw) is int and gw == ww
    for g, w in zip(got[1:], want[1:]):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
    two = H.rec_batches_lines(ratios, native=True, **kw)             # without the ratios: the same first two
    assert len(two) == 2 and np.array_equal(two[1], want[1]) and [w for _c, w in two[0]] == [w for _c, w in want[0]]
    return got


@pytest.mark.parametrize("n", [0, 1, 5, 6, 7, 1440])
def test_sizes_around_the_reference_chunk(n):
    rng = np.random.default_rng(n)
    batches, line_w, line_ratio = assert_same((rng.random(n) * 30 + 0.2).tolist())
    assert sum(len(c) for c, _w in batches) == n == len(line_w) == len(line_ratio)


def test_ratios_below_the_default_width_keep_it():
    batches, line_w, line_ratio = assert_same([0.5, 6.6, 1.0, 320 / 48, 3.25, 6.666, 2.0])
    assert line_w.tolist() == [320] * 7 and line_ratio.tolist() == [320 / 48] * 7 and [w for _c, w in batches] == [320]
    # the last chunk alone above it; another chunk size, line height and launch multiple
    assert_same([0.5, 6.6, 1.0, 320 / 48, 3.25, 6.666, 2.0, 6.7, 6.7000001], rec_batch_num=4)
    assert_same([0.5, 9.1, 1.0, 7.77, 3.25, 6.666, 2.0], rec_batch_num=3, img_h=32, img_w=100, launch_multiple=8)


def test_equal_ratios_across_a_chunk_border():
    """Ties at a chunk border may land in either chunk - wherever np.argsort's default kind puts them; both paths take that one order."""
    rng = np.random.default_rng(5)
    ratios = np.repeat(rng.random(40) * 20 + 5, rng.integers(1, 14, size=40))
    ratios = ratios[rng.permutation(len(ratios))].tolist()
    batches, _line_w, _line_ratio = assert_same(ratios)
    order = np.concatenate([c for c, _w in batches])
    assert np.array_equal(order, np.argsort(np.array(ratios)))
    assert_same(ratios, rec_batch_num=5, n_min=4, n_max=40, n_step=3)
    # the library call on an order of its own: ties reversed against the stable order, the widths follow the order it is given
    import ctypes as C

    from rapiddoc_amd import _lib
    r = np.array([7.0, 9.0, 9.0, 9.0, 7.0, 12.5, 9.0])
    order = np.array([4, 0, 6, 3, 2, 1, 5], np.int64)
    n = len(r)
    lw, lr, sz, wd, k = np.zeros(n, np.int64), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32), C.c_int32(0)
    args = (2, 48, 320, 32, 16, 160, 2, 256, lw.ctypes.data, lr.ctypes.data, sz.ctypes.data, wd.ctypes.data, n, C.byref(k))
    assert _lib.load().rd_rec_plan_lines(r.ctypes.data, order.ctypes.data, n, *args) == 0
    assert lw.tolist() == [336, 336, 432, 432, 432, 432, 600] and lr.tolist() == [7.0, 7.0, 9.0, 9.0, 9.0, 9.0, 12.5]
    assert sz[: k.value].sum() == n and wd[k.value - 1] == 608
    order[3] = 7                                                        # an index outside the list is refused, not read
    assert _lib.load().rd_rec_plan_lines(r.ctypes.data, order.ctypes.data, n, *args) == 1


def test_the_benchmarks_own_lines():
    """The 32 x 45 lines of bench.py's page batch, from its det records (tests/golden/bench_det_records.npz, written by
    tools/host_boundary.py --write-fixture) to the launches."""
    spec = importlib.util.spec_from_file_location("host_boundary", ROOT / "tools" / "host_boundary.py")
    hb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hb)
    records, counts = hb.fixture_inputs()
    quads = H.order_merge_boxes_native(records, counts)
    assert all(np.array_equal(a, b) for a, b in zip(quads, hb.boxes_python(records, counts)))
    ratios, _q = hb.line_ratios(quads)
    assert len(ratios) == 1440
    batches, line_w, _r = assert_same(ratios)
    assert line_w.min() >= 320 and all(w % 32 == 0 for _c, w in batches)
