"""Numpy restatement of what rd_region_canvases writes (include/rapiddoc_mi355.h), from the calls the host route is made of: a slice of
the page, layout_polygon.polygon_keep_mask for the polygon, integer mask boxes.  Shared by tests/test_analyze_pages_list_host.py (the
descriptor packing) and tests/test_gpu_region_compose.py (the kernel)."""
import numpy as np

from rapiddoc_amd import layout_polygon


def compose(page: np.ndarray, rect, paste, polygon, boxes, gh: int, gw: int):
    """(canvas, detector canvas) [gh, gw, 3] u8 of one region.  page [H, W, 3]; rect = UNclipped (x0, y0, x1, y1) in page coordinates;
    paste = canvas position of (x0, y0); polygon = points in page coordinates or None; boxes = integer (x0, y0, x1, y1) in canvas
    coordinates.  A part of the window that leaves the canvas is dropped, as nothing may be written outside it."""
    H, W = page.shape[:2]
    x0, y0, x1, y1 = (int(v) for v in rect)
    canv = np.full((gh, gw, 3), 255, np.uint8)
    x0c, y0c, x1c, y1c = max(0, x0), max(0, y0), min(W, x1), min(H, y1)
    if x1c > x0c and y1c > y0c:
        part = page[y0c:y1c, x0c:x1c].copy()
        if polygon is not None and len(polygon):
            part[~layout_polygon.polygon_keep_mask(part.shape[:2], polygon, x0, y0)] = 255
        cx, cy = int(paste[0]) + (x0c - x0), int(paste[1]) + (y0c - y0)
        # the window on the canvas, clipped to the canvas
        ax, ay, bx, by = max(0, cx), max(0, cy), min(gw, cx + part.shape[1]), min(gh, cy + part.shape[0])
        if bx > ax and by > ay:
            canv[ay:by, ax:bx] = part[ay - cy: by - cy, ax - cx: bx - cx]
    det = canv.copy()
    for b in boxes:
        det[b[1]:b[3], b[0]:b[2]] = 255
    return canv, det


def compose_descs(descs, pts, boxes, page_of, gh: int, gw: int):
    """the same from packed descriptors (engine.REGION_DESC_DTYPE rows + their vertex and box lists); page_of: address -> numpy page"""
    out = []
    for d in descs:
        page = page_of[int(d["page"])]
        assert page.shape[:2] == (int(d["page_h"]), int(d["page_w"])) and int(d["pitch"]) == page.strides[0]
        poly = pts[int(d["poly_off"]): int(d["poly_off"]) + int(d["poly_n"])] if int(d["poly_n"]) else None
        bx = boxes[int(d["box_off"]): int(d["box_off"]) + int(d["box_n"])]
        out.append(compose(page, [int(d[k]) for k in ("x0", "y0", "x1", "y1")], (int(d["paste_x"]), int(d["paste_y"])), poly, bx, gh, gw))
    return out
