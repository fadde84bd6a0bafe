"""CPU: csrc/region_geom.h - the per-pixel form of cv2.fillPoly's raster that the device evaluates (kernels_region.hip) - against
rd_fill_poly (polygon_ops.cpp), element for element.  rd_debug_region_keep_mask runs the header's functions on the host, no HIP call."""
import numpy as np
import pytest

from rapiddoc_amd import layout_polygon


@pytest.fixture(scope="module")
def lib():
    from rapiddoc_amd import build as rd_build
    rd_build.build(verbose=False)
    from rapiddoc_amd import _lib
    return _lib.load()


def _header_mask(lib, h, w, pts):
    p = np.ascontiguousarray(np.asarray(pts, dtype=np.int32).reshape(-1, 2))
    out = np.full((h, w), 7, np.uint8)
    assert lib.rd_debug_region_keep_mask(h, w, p.ctypes.data if len(p) else None, len(p), out.ctypes.data) == 0
    return out


def _fill_poly_mask(h, w, pts):
    return layout_polygon.fill_poly(np.zeros((h, w), np.uint8), np.asarray(pts, dtype=np.int32).reshape(-1, 2), 1)


def _max_poly():
    from rapiddoc_amd.engine import REGION_MAX_POLY
    return REGION_MAX_POLY


def test_random_polygons_equal_fill_poly(lib):
    rng = np.random.default_rng(20250)
    bad = []
    for case in range(2000):
        n = int(rng.integers(3, 17))
        h, w = int(rng.integers(1, 49)), int(rng.integers(1, 49))
        pts = rng.integers(-16, 64, size=(n, 2)).astype(np.int32)
        if not np.array_equal(_header_mask(lib, h, w, pts), _fill_poly_mask(h, w, pts)):
            bad.append((case, h, w, pts.tolist()))
    assert not bad, f"{len(bad)} of 2000 differ, first: {bad[0]}"


def _cap_polygon(n):
    """a star of n vertices, alternating radii: self-touching spikes, many edges per row"""
    k = np.arange(n)
    r = np.where(k % 2 == 0, 22.0, 9.0)
    return np.stack([24 + r * np.cos(2 * np.pi * k / n), 20 + r * np.sin(2 * np.pi * k / n)], axis=1).astype(np.int32)


FIXED = {
    "one point": [(5, 7)],
    "one point outside": [(-3, 2)],
    "two points": [(2, 3), (30, 17)],
    "two points steep": [(20, 1), (14, 30)],
    "two points, horizontal": [(-5, 9), (70, 9)],
    "all points equal": [(11, 11)] * 5,
    "horizontal and vertical edges": [(4, 4), (40, 4), (40, 30), (4, 30)],
    "rectangle over the window": [(-10, -10), (60, -10), (60, 50), (-10, 50)],
    "vertex exactly on a row": [(5, 5), (25, 15), (45, 5), (45, 25), (25, 15), (5, 25)],
    "vertex on a row, diamond": [(20, 2), (38, 20), (20, 38), (2, 20)],
    "bow-tie": [(3, 3), (44, 36), (44, 3), (3, 36)],
    "concave L": [(4, 4), (20, 4), (20, 24), (42, 24), (42, 36), (4, 36)],
    "wholly outside": [(60, 60), (90, 62), (75, 95)],
    "wholly above": [(2, -30), (30, -28), (12, -3)],
    "thin sliver": [(0, 0), (47, 1), (47, 2)],
    "collinear": [(1, 1), (10, 10), (30, 30)],
    "the cap itself": None,
}


@pytest.mark.parametrize("name", list(FIXED))
def test_fixed_cases_equal_fill_poly(lib, name):
    pts = _cap_polygon(_max_poly()) if FIXED[name] is None else np.asarray(FIXED[name], np.int32)
    for h, w in ((40, 48), (17, 23), (1, 1), (48, 5)):
        got, want = _header_mask(lib, h, w, pts), _fill_poly_mask(h, w, pts)
        assert np.array_equal(got, want), (name, h, w, np.argwhere(got != want)[:5].tolist())
    if name in ("wholly outside", "wholly above", "one point outside"):
        assert not _header_mask(lib, 40, 48, pts).any()
    else:
        assert _header_mask(lib, 40, 48, pts).any()


def test_no_points_sets_nothing_and_the_cap_is_refused(lib):
    assert not _header_mask(lib, 9, 13, np.zeros((0, 2), np.int32)).any()
    cap = _max_poly()
    assert cap >= 32
    over = np.ascontiguousarray(_cap_polygon(cap + 1))
    out = np.zeros((8, 8), np.uint8)
    assert lib.rd_debug_region_keep_mask(8, 8, over.ctypes.data, len(over), out.ctypes.data) == -1
    assert lib.rd_debug_region_keep_mask(0, 8, over.ctypes.data, 3, out.ctypes.data) == -1
    assert lib.rd_debug_region_keep_mask(8, 8, over.ctypes.data, 3, None) == -1
