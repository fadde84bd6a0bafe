"""GPU: checkbox detection on the device (`rd_checkbox_detect_device`, csrc/kernels_checkbox.hip; `rd_checkbox_finish`; rapiddoc_amd/
checkbox.py) against the numpy restatement of tests/checkbox_reference.py, BIT FOR BIT: the three mask planes word for word, every
component's box and label-order key, per candidate the ROI rectangle, the ROI rows and the tick count, and the final dicts.  Every device
buffer of these tests lies between guard bytes that must come back untouched."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import checkbox_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 256
SHAPES = [(1, 1), (14, 14), (15, 15), (40, 63), (40, 64), (40, 65), (33, 200), (97, 130)]


def noisy_page(seed, H, W, p_dark=0.9):
    """RGB: a dense random bitmap (runs of 14 / 15 / 16 inside, of 7 / 8 at the frame) with grey levels on both sides of 150, 150 and
    151 included"""
    rng = np.random.default_rng(seed)
    dark = rng.random((H, W)) < p_dark
    level = np.where(dark, rng.integers(120, 151, (H, W)), rng.integers(151, 200, (H, W)))
    return np.clip(level[:, :, None] + rng.integers(-3, 4, (H, W, 3)), 0, 255).astype(np.uint8)


def form_like(seed, H, W):
    """boxes where the page has room for them (one ticked, one in the page's corner: its ROI is clipped), sparse noise otherwise"""
    if H < 97:
        return noisy_page(seed, H, W, 0.3)
    g = np.full((H, W), 255, np.uint8)
    R.draw_box(g, 10, 8, 26, 26)
    R.draw_tick(g, 10, 8, 26, 3)
    R.draw_box(g, 60, 40, 30, 30)
    R.draw_box(g, W - 24, H - 24, 24, 24)
    R.draw_box(g, 0, H - 30, 22, 22)
    return np.ascontiguousarray(np.stack([g, np.maximum(g, 2) - 2, np.maximum(g, 5) - 5], axis=-1))


def guarded(nbytes, dev):
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + nbytes]


def device_trace(pages_rgb, max_runs=None, max_cand=64, bgr=False):
    """run the kernels on guarded buffers -> (headers, per page a dict of what the device computed)"""
    from rapiddoc_amd import checkbox as CB
    pages = torch.from_numpy(np.ascontiguousarray(pages_rgb)).cuda()
    P, H, W, _ = pages.shape
    max_runs = max_runs or CB.default_max_runs(H, W)
    nbytes, offs = CB.workspace(P, H, W, max_runs, max_cand)
    bufs = [guarded(n, pages.device) for n in (nbytes, P * CB.PAGE_DTYPE.itemsize, P * max_cand * CB.CAND_DTYPE.itemsize)]
    CB.run_device(pages, bgr, max_runs, max_cand, ws=bufs[0][1], hdr=bufs[1][1], cands=bufs[2][1])
    torch.cuda.synchronize()
    for whole, _v in bufs:
        w = whole.cpu().numpy()
        assert (w[:GUARD] == 0xA5).all() and (w[-GUARD:] == 0xA5).all(), "guard bytes around a device buffer were written"
    ws = bufs[0][1].cpu().numpy()
    hdr = bufs[1][1].cpu().numpy().view(CB.PAGE_DTYPE)
    cands = bufs[2][1].cpu().numpy().view(CB.CAND_DTYPE)
    WW = (W + 63) // 64
    plane = lambda name: ws[offs[name]:offs[name] + P * H * WW * 8].view("<u8").reshape(P, H, WW)
    ints = lambda name: ws[offs[name]:offs[name] + P * max_runs * 4].view("<i4").reshape(P, max_runs)
    out = []
    for p in range(P):
        d = {"bin": plane("bin")[p], "lines": plane("lines")[p], "final": plane("final")[p], "hdr": hdr[p]}
        if not hdr[p]["flags"] & CB.RUNS_OVERFLOW:
            n = int(hdr[p]["n_runs"])
            roots = np.flatnonzero(ints("parent")[p, :n] == np.arange(n))
            k, x0, x1, y0, y1 = (ints(nm)[p, roots] for nm in ("key", "minx", "maxx", "miny", "maxy"))
            d["comps"] = sorted(zip(k.tolist(), x0.tolist(), y0.tolist(), (x1 - x0 + 1).tolist(), (y1 - y0 + 1).tolist()))
            rec = cands[hdr[p]["cand_off"]:hdr[p]["cand_off"] + min(int(hdr[p]["n_cand"]), max_cand)]
            d["records"] = rec[np.argsort(rec["key"], kind="stable")]
        out.append(d)
    return hdr, out


def assert_page_equals_restatement(dev, rgb):
    from rapiddoc_amd import checkbox as CB
    t = R.checkbox_trace(np.ascontiguousarray(rgb[:, :, ::-1]))
    H, W = rgb.shape[:2]
    for name in ("bin", "lines", "final"):
        assert np.array_equal(dev[name], R.pack_words(t[name])), name
    assert dev["hdr"]["flags"] == 0 and dev["hdr"]["n_comp"] == len(t["comps"])
    assert dev["comps"] == sorted(t["comps"]) and [c[0] for c in t["comps"]] == sorted(c[0] for c in t["comps"])
    assert dev["hdr"]["first_key"] == (t["comps"][0][0] if t["comps"] else -1)
    rec = dev["records"]
    assert len(rec) == len(t["cands"]) == dev["hdr"]["n_cand"]
    for r, c in zip(rec, t["cands"]):
        assert (int(r["key"]), (int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"]))) == (c["key"], c["box"])
        assert (int(r["rx"]), int(r["ry"]), int(r["rw"]), int(r["rh"])) == c["roi_rect"]
        rows = np.zeros(CB.ROI_ROWS, "<u8")
        rows[:c["roi"].shape[0]] = R.pack_words(c["roi"])[:, 0]
        assert np.array_equal(r["roi"], rows)                                    # the ROI bytes, as bits
        assert int(r["tick"]) == c["tick"]
    assert CB.finish(rec, H, W) == t["result"]
    return t


@pytest.mark.parametrize("H,W", SHAPES)
def test_device_equals_the_restatement_bit_for_bit(H, W):
    pages = np.stack([noisy_page(10 * H + W, H, W), noisy_page(7 * H + W, H, W, 0.97), form_like(H + W, H, W)])
    _hdr, dev = device_trace(pages)
    traces = [assert_page_equals_restatement(dev[p], pages[p]) for p in range(3)]
    if (H, W) == (97, 130):
        assert any(t["cands"] for t in traces)                                   # the tick chain ran


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(golden_dir / "checkbox_pages.npz")), json.loads((golden_dir / "checkbox_expected.json").read_text())


@pytest.fixture(scope="module")
def box():
    from rapiddoc_amd.checkbox import Mi355Checkbox
    return Mi355Checkbox(0)


def test_golden_pages(golden, box):
    pages, exp = golden
    for name, bgr in pages.items():
        rgb = np.ascontiguousarray(bgr[:, :, ::-1])
        _hdr, dev = device_trace(rgb[None])
        assert_page_equals_restatement(dev[0], rgb)
        assert box.detect_pages(torch.from_numpy(rgb[None]).cuda()) == [exp["small"][name]]
        assert box(bgr) == exp["small"][name]                                    # the BGR call, uploaded


def test_a_batch_equals_its_pages_alone_and_bgr_equals_rgb(golden, box):
    bgr = [golden[0]["outcomes"], golden[0]["filter_edges"], np.ascontiguousarray(noisy_page(1, 200, 260)[:, :, ::-1])]
    rgb = np.stack([b[:, :, ::-1] for b in bgr])
    together = box.detect_pages(torch.from_numpy(np.ascontiguousarray(rgb)).cuda())
    records = [r.copy() for r in box.last_records]
    for p in range(3):
        assert box.detect_pages(torch.from_numpy(np.ascontiguousarray(rgb[p:p + 1])).cuda()) == [together[p]]
        assert np.array_equal(box.last_records[0], records[p])
        assert box(bgr[p]) == together[p]
    assert together[0] == golden[1]["small"]["outcomes"] and together[1] == golden[1]["small"]["filter_edges"]


def test_overflow_is_reported_and_recovered(golden):
    from rapiddoc_amd import checkbox as CB
    bgr = golden[0]["outcomes"]
    rgb = torch.from_numpy(np.ascontiguousarray(bgr[:, :, ::-1])[None]).cuda()
    hdr, dev = device_trace(rgb.cpu().numpy(), max_runs=8)
    assert hdr[0]["flags"] & CB.RUNS_OVERFLOW and hdr[0]["n_runs"] > 8 and hdr[0]["n_cand"] == 0
    hdr, dev = device_trace(rgb.cpu().numpy(), max_cand=2)
    assert hdr[0]["flags"] == CB.CANDS_OVERFLOW and hdr[0]["n_cand"] > 2
    for kw in ({"max_runs": 8}, {"max_cand": 2}, {"max_runs": 8, "max_cand": 1}):
        small = CB.Mi355Checkbox(0, **kw)
        assert small.detect_pages(rgb) == [golden[1]["small"]["outcomes"]]
        assert small.last_headers[0]["flags"] != 0                               # never silent: the first pass said so


def test_guards_on_the_device_entry(box):
    from rapiddoc_amd import _lib
    lib = _lib.load()
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    for args in ((0, 1, 8, 8), (p, 1, 0, 8), (p, 1, 8, 16385), (p, 0, 8, 8), (p, 1025, 8, 8)):
        assert lib.rd_checkbox_detect_device(0, args[0], args[1], args[2], args[3], 0, 16, 4, p, 4096, p, p, None) != 0
        assert b"rd_checkbox_detect_device" in lib.rd_create_error()
    assert lib.rd_checkbox_detect_device(0, p, 1, 8, 8, 0, 16, 4, p, 64, p, p, None) != 0 and b"workspace" in lib.rd_create_error()
    torch.cuda.synchronize()
    assert int(t.sum()) == 0                                                     # nothing was launched


def test_full_size_form_pages(golden, box):
    exp = golden[1]
    H, W = exp["form_shape"]
    pages = torch.from_numpy(np.stack([R.form_page(seed, H, W) for seed in (11, 12)])).cuda()
    got = box.detect_pages(pages)
    assert got == [exp["forms"]["11"], exp["forms"]["12"]]
    assert (box.last_headers["flags"] == 0).all()
    assert 0 < box.last_d2h_bytes < 0.01 * pages.numel(), box.last_d2h_bytes
