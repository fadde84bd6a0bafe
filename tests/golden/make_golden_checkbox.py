#!/usr/bin/env python3
"""Golden vectors of the checkbox stage, minted by the reference's own code (build container only).

    python tests/golden/make_golden_checkbox.py      # writes tests/golden/checkbox_pages.npz and tests/golden/checkbox_expected.json

What runs is rapid_doc/utils/checkbox_det_cls.py, loaded by file path, unmodified: `checkbox_predict` = detect_checkboxes +
classify_checkboxes with their default arguments.  The module imports `cv2`, which is not installed here; it is stood in for by
tests/checkbox_reference.py fake_cv2(), whose functions restate the OpenCV calls - so the vectors pin every line the reference wrote
around those calls (stats[2:], the size filter, the ROI arithmetic, the Counter ranking, the tick share, the result dicts) and NOT the
arithmetic inside OpenCV (docs/notebook/checkbox.md lists what stays unpinned).
Small pages are stored as pixels (BGR, .npz); the two 1684 x 1191 form pages are stored as their expected lists only - the test
regenerates their pixels from the integer hash of checkbox_reference.form_page.  The mint asserts that the fixtures hold every outcome
the stage can have."""
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
sys.path.insert(0, str(HERE.parent))
import checkbox_reference as R  # noqa: E402


def page_outcomes():
    """260 wide, 200 high: ticked and empty boxes, a faint tick, a rule right under a box, and two boxes whose interiors start at
    y = 13 (left) and y = 12 (right)"""
    g = np.full((200, 260), 255, np.uint8)
    R.draw_box(g, 20, 10, 24, 24)              # interior starts at y = 12 ... dilated frame: rows 13 .. 30 -> y = 13
    R.draw_box(g, 120, 9, 24, 24)              # one row higher -> y = 12
    R.draw_box(g, 20, 60, 26, 26)
    R.draw_tick(g, 20, 60, 26, 3)              # a bold cross
    R.draw_box(g, 80, 60, 26, 26)
    g[72:75, 90:94] = 20                       # a small blot: some tick share, below 0.2
    R.draw_box(g, 140, 60, 30, 30)
    R.draw_tick(g, 140, 60, 30, 2)
    R.draw_box(g, 20, 120, 24, 24)
    g[146:148, 135 - 100:165 - 100] = 30       # a rule right under the box: its left end lies inside the ROI's lower extension
    R.draw_box(g, 100, 120, 24, 24)            # the same box without the rule
    g[170:172, 150:158] = 40                   # a dash shorter than 15: no line
    return g


def page_filter_edges():
    """component sizes 11, 12, 50, 51 (squares) and 18, 17, 22, 23 wide on 20 high; the frame is 2 thick and the dilation takes one
    more pixel from each side: outer = component + 6"""
    g = np.full((200, 260), 255, np.uint8)
    x = 8
    for side in (11, 12, 50, 51):
        R.draw_box(g, x, 8, side + 6, side + 6)
        x += side + 6 + 9
    x = 8
    for w in (18, 17, 22, 23):
        R.draw_box(g, x, 90, w + 6, 26)
        x += w + 6 + 12
    return g


def page_first_dropped():
    """a dark band across the top with a box-sized window in it: the window is the FIRST component in label order, so stats[2:] drops
    it although it has a checkbox's size; the same window lower down is kept"""
    g = np.full((100, 120), 255, np.uint8)
    g[0:30, :] = 30
    g[6:26, 10:30] = 255
    R.draw_box(g, 60, 50, 26, 26)
    return g


def grey_to_bgr(g, seed):
    """three channels with a little hashed colour so that the grey conversion has work to do (light pixels stay above 150)"""
    H, W = g.shape
    n = (R._hash32(np.arange(H * W * 3, dtype=np.uint64) + np.uint64(seed << 32)) % 5).astype(np.int16).reshape(H, W, 3)
    return np.clip(g[:, :, None].astype(np.int16) - n, 0, 255).astype(np.uint8)


def main():
    sys.modules["cv2"] = R.fake_cv2()
    spec = importlib.util.spec_from_file_location("ref_checkbox_det_cls", REF / "rapid_doc/utils/checkbox_det_cls.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    small = {"outcomes": grey_to_bgr(page_outcomes(), 1), "filter_edges": grey_to_bgr(page_filter_edges(), 2),
             "first_dropped": grey_to_bgr(page_first_dropped(), 3)}
    expected = {name: ref.checkbox_predict(bgr) for name, bgr in small.items()}
    traces = {name: R.checkbox_trace(bgr) for name, bgr in small.items()}
    for name in small:
        assert traces[name]["result"] == expected[name], name         # the restatement's own driver agrees with the reference's
        print(name, small[name].shape, [(r["bbox"], r["label"]) for r in expected[name]])

    # ---- every outcome is present
    t = traces["outcomes"]
    labels = {r["label"] for r in expected["outcomes"]}
    assert labels == {"Ticked", "Unticked"}
    assert any(not c["keeps"] for c in t["cands"]), "no reject by the contour rule"
    assert [25, 123, 43, 141] not in [r["bbox"] for r in expected["outcomes"]] and any(c["box"][:2] == (23, 123) and not c["keeps"] for c in t["cands"])
    shares = [c["tick"] / (c["box"][2] * c["box"][3]) for c in t["cands"] if c["keeps"]]
    assert any(0 < s <= 0.2 for s in shares) and any(s > 0.2 for s in shares), shares
    # the y = 12 / y = 13 swap: label order puts the LEFT box (y = 13) first, pixel-raster order would put the right one (y = 12) first
    first_two = [r["bbox"] for r in expected["outcomes"][:2]]
    assert first_two[0][1] == 13 and first_two[1][1] == 12 and first_two[0][0] < first_two[1][0], first_two
    raster = sorted(first_two, key=lambda b: (b[1], b[0]))
    assert raster != first_two
    t = traces["filter_edges"]
    sizes = {(c[3], c[4]) for c in t["comps"]}
    assert {(11, 11), (12, 12), (50, 50), (51, 51), (18, 20), (17, 20), (22, 20), (23, 20)} <= sizes, sizes
    kept = {(r["bbox"][2] - r["bbox"][0], r["bbox"][3] - r["bbox"][1]) for r in expected["filter_edges"]}
    assert kept == {(12, 12), (50, 50), (18, 20), (22, 20)}, kept
    t = traces["first_dropped"]
    first = t["comps"][0]
    assert first[3:] == (18, 18) and 12 <= first[3] <= 50, first                      # candidate-sized, and first in label order
    assert [r["bbox"] for r in expected["first_dropped"]] == [[63, 53, 83, 73]], expected["first_dropped"]

    forms = {}
    for seed in (11, 12):
        bgr = np.ascontiguousarray(R.form_page(seed)[:, :, ::-1])
        forms[str(seed)] = ref.checkbox_predict(bgr)
        n_t = sum(r["label"] == "Ticked" for r in forms[str(seed)])
        print("form page", seed, bgr.shape, len(forms[str(seed)]), "boxes,", n_t, "ticked")
        assert len(forms[str(seed)]) >= 20 and 3 <= n_t < len(forms[str(seed)])

    np.savez_compressed(HERE / "checkbox_pages.npz", **small)
    (HERE / "checkbox_expected.json").write_text(json.dumps({"small": expected, "forms": forms, "form_shape": [1684, 1191]}, ensure_ascii=False, indent=0))


if __name__ == "__main__":
    main()
