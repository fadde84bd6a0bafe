#!/usr/bin/env python3
"""Microbenchmark of region composition in the OCR stage of the page driver (`analyze.RegionOcr`): the "host" route - torch calls per
region, polygon masks rasterised on the host and uploaded, a clone per masked group - against the "device" route
(`engine.region_canvases`: one staging upload per batch, one launch per size group), at a realistic region count.

Workload: 32 `pages.synth_page` pages; per page about 20 text regions, each two of the generator's own text lines, the last of them with
`polygon_points` (a hexagon inside its rectangle), and three formula boxes that lie on text lines.  The detector's maps are drawn from the
line boxes (random weights find no text), once, outside the timed part.

Both routes run in ONE process, alternated round by round after the warm-up; the host route takes part twice ("host a", "host b"), so
that the spread of the host route against itself is known.  Timed:
  compose     the composition of every size group alone, between two device events (the host work between the launches is inside);
  whole call  one `RegionOcr.__call__` - composition, detector, DB post-process, line crops, recogniser - host clock around a synchronise.
Reported: medians and min .. max, the bytes the composition moves (pages read + canvases written) and bytes/s over the compose time,
crc32 of every canvas (the routes must agree), and which route the rule of docs/notebook/region_compose.md makes the default.

    python tools/mb_region_compose.py [--pages 32] [--steps 7] [--warmup 2] > profiles/mb_region_compose.txt
"""
import argparse
import sys
import time
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def make_batch(n_pages: int):
    """pages uint8 [n, H, W, 3], per page the layout detections and the text-line boxes"""
    from rapiddoc_amd.pages import synth_page
    pages, dets, lines = [], [], []
    for p in range(n_pages):
        page, boxes = synth_page(p)
        pages.append(page)
        lines.append(boxes)
        page_dets = []
        pairs = [boxes[i: i + 2] for i in range(0, len(boxes) - 1, 2)][:21]
        for k, pair in enumerate(pairs):
            x0, y0 = int(pair[:, 0].min()) - 6, int(pair[:, 1].min()) - 3
            x1, y1 = int(pair[:, 2].max()) + 6, int(pair[:, 3].max()) + 3
            d = {"category_id": 1, "original_label": "text", "original_order": k, "poly": [x0, y0, x1, y0, x1, y1, x0, y1], "score": 0.9}
            if k == len(pairs) - 1:           # a hexagon that keeps the lines and cuts the rectangle's corners
                d["polygon_points"] = [[x0 + 12.5, y0], [x1 - 12.5, y0], [x1, (y0 + y1) / 2], [x1 - 12.5, y1], [x0 + 12.5, y1], [x0, (y0 + y1) / 2]]
            page_dets.append(d)
        for k in (0, 5, 10):                 # three formula boxes, each on the first line of a region
            bx0, by0, _bx1, by1 = (float(v) for v in pairs[k][0])
            f = [bx0 + 120.5, by0 + 1, bx0 + 200.25, by1 - 1]
            page_dets.append({"category_id": 13, "original_label": "inline_formula", "original_order": 100 + k,
                              "poly": [f[0], f[1], f[2], f[1], f[2], f[3], f[0], f[3]], "score": 0.8})
        dets.append(page_dets)
    return np.stack(pages), dets, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert args.steps >= 7, "medians of at least 7 repetitions"
    import copy

    import torch
    from rapiddoc_amd import analyze, layout_host, ocr_host
    from rapiddoc_amd import weights as W
    from rapiddoc_amd.engine import region_canvases
    from rapiddoc_amd.pipeline import PagePipeline, render_text_maps

    g = ROOT / "tests" / "golden"
    pipe = PagePipeline({k: W.synth_state_dict(W.load_manifest(g / f"manifest_{k}.json"), 0) for k in ("ppocrv6_det", "ppocrv6_rec")}, device=0)
    pages_np, dets0, lines = make_batch(args.pages)
    pages = torch.from_numpy(pages_np).cuda()
    ps = analyze.page_set(pages)
    maps_cache = {}

    def maps_fn(regs, ghw, dhw):
        key = (ghw, len(regs), regs[0][0], tuple(regs[0][2]))
        if key not in maps_cache:
            per_img = []
            for p, r, useful in regs:
                px, py, x0, y0 = useful[0], useful[1], useful[2], useful[3]
                bb = np.asarray(lines[p], dtype=np.float64).reshape(-1, 4)
                inside = bb[(bb[:, 0] >= x0) & (bb[:, 2] <= r["poly"][4]) & (bb[:, 1] >= y0) & (bb[:, 3] <= r["poly"][5])]
                per_img.append(inside - [x0 - px, y0 - py, x0 - px, y0 - py])
            maps_cache[key] = render_text_maps(per_img, ghw, dhw, pages.device)
        return maps_cache[key]

    # the region list and the size groups exactly as RegionOcr.__call__ makes them
    regions = []
    for p, dets in enumerate(dets0):
        ocr_regions, _t, formulas = layout_host.split_regions(copy.deepcopy(dets))
        for r in ocr_regions:
            useful = layout_host.crop_geometry(r, analyze.PASTE, analyze.PASTE)
            regions.append((p, r, useful, analyze._formula_boxes_in_crop(formulas, useful)))
    groups = ocr_host.det_buckets([(u[7], u[6]) for _, _, u, _ in regions], ["ch"] * len(regions), det_batch_num=len(regions))
    canvas_bytes = read_bytes = 0
    for _lang, (gh, gw), members, _bs in groups:
        masked = any(regions[i][3] for i in members)
        canvas_bytes += len(members) * gh * gw * 3 * (2 if masked else 1)
        for i in members:
            _p, _r, (_px, _py, x0, y0, x1, y1, _nw, _nh), _f = regions[i]
            read_bytes += max(0, min(pages.shape[2], x1) - max(0, x0)) * max(0, min(pages.shape[1], y1) - max(0, y0)) * 3

    def compose_only(route):
        """every group's canvases on `route` -> (ms between two device events, crc32 of all canvases)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = []
        staged = analyze.RegionOcr._stage_groups(ps, regions, groups) if route == "device" else {}
        for gi, (_lang, (gh, gw), members, _bs) in enumerate(groups):
            if gi in staged:
                stage, at = staged[gi]
                canv, det = region_canvases(stage.groups[at], (gh, gw), any(r.boxes for r in stage.groups[at]), stage, at)
            else:
                canv, det = analyze.RegionOcr._compose_host(ps, regions, members, gh, gw)
            out.append((canv, det))
        e1.record()
        torch.cuda.synchronize()
        crc = 0
        for canv, det in out:
            crc = zlib.crc32(canv.cpu().numpy().tobytes(), crc)
            if det is not None and det is not canv:
                crc = zlib.crc32(det.cpu().numpy().tobytes(), crc)
        return e0.elapsed_time(e1), crc

    def whole_call(route):
        ocr = analyze.RegionOcr(pipe, compose=route)
        dets = copy.deepcopy(dets0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ocr(pages, dets, det_maps_fn=maps_fn)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        spans = [(d["poly"], d["text"], d["score"]) for page in out for d in page if d["category_id"] in (15, 16)]
        return ms, zlib.crc32(repr(spans).encode()), len(spans)

    parts = [("host a", "host"), ("device", "device"), ("host b", "host")]
    print(f"# tools/mb_region_compose.py {' '.join(sys.argv[1:])}: {args.pages} pages of {pages.shape[1]} x {pages.shape[2]}, {len(regions)} text regions "
          f"({sum(1 for r in regions if r[1].get('polygon_points'))} with a polygon, {sum(len(r[3]) for r in regions)} formula boxes inside them) in "
          f"{len(groups)} size groups; {args.warmup} warm-up + {args.steps} timed rounds, routes alternating in one process")
    print(f"# the composition reads {read_bytes / 1e6:.1f} MB of page pixels and writes {canvas_bytes / 1e6:.1f} MB of canvases")
    comp = {name: [] for name, _ in parts}
    whole = {name: [] for name, _ in parts}
    crcs = {}
    for r in range(args.warmup + args.steps):
        row = []
        for name, route in parts:
            c_ms, c_crc = compose_only(route)
            w_ms, w_crc, n_spans = whole_call(route)
            crcs.setdefault("canvases", c_crc)
            crcs.setdefault("spans", w_crc)
            assert c_crc == crcs["canvases"], (name, "the canvases differ between the routes")
            assert w_crc == crcs["spans"], (name, "the spans differ between the routes")
            row += [c_ms, w_ms]
            if r >= args.warmup:
                comp[name].append(c_ms)
                whole[name].append(w_ms)
        print(f"round {r:2d}{' (warm-up)' if r < args.warmup else '          '}  " +
              "  ".join(f"{name}: compose {row[2 * i]:8.3f}  call {row[2 * i + 1]:9.2f}" for i, (name, _) in enumerate(parts)) + "  ms", flush=True)
    print(f"canvases crc32 {crcs['canvases']}  spans crc32 {crcs['spans']} ({n_spans} spans): equal on every route and round")
    print(f"{'participant':10s} {'compose median ms':>18s} {'min':>9s} {'max':>9s} {'GB/s':>8s}   {'whole call median ms':>20s} {'min':>9s} {'max':>9s}")
    for name, _ in parts:
        c, w = np.asarray(comp[name]), np.asarray(whole[name])
        print(f"{name:10s} {np.median(c):18.3f} {c.min():9.3f} {c.max():9.3f} {(read_bytes + canvas_bytes) / np.median(c) / 1e6:8.2f}   "
              f"{np.median(w):20.2f} {w.min():9.2f} {w.max():9.2f}")
    host_all = np.asarray(whole["host a"] + whole["host b"])
    spread = abs(float(np.median(whole["host a"])) - float(np.median(whole["host b"])))
    dev, host = float(np.median(whole["device"])), float(np.median(host_all))
    print(f"whole call: host median {host:.2f} ms (both host participants), host-against-host spread {spread:.2f} ms, device median {dev:.2f} ms")
    print(f"rule: device is the default iff {dev:.2f} <= {host:.2f} + {spread:.2f}  ->  {'device' if dev <= host + spread else 'host'}")


if __name__ == "__main__":
    main()
