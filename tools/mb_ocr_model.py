#!/usr/bin/env python3
"""Microbenchmark of the OCR-model seam (`rapiddoc_amd.ocr_model.Mi355RapidOcrModel`, docs/notebook/ocr_model_seam.md) against the routes an
unmodified RapidDoc had before it, on the workload of tools/mb_region_compose.py: 32 `pages.synth_page` pages, about 21 text regions per
page with two text lines each.  Every region is an image of its own (BGR, as the reference's driver holds it), every line a box in it.

  (a) pooled rec   `ocr(crops, det=False)` on ALL line crops as numpy arrays - one upload, the strict planner, GPU-sized launches - against
                   the S2 seam: the reference's chunk-of-6 loop (rapid_ocr.py:404-472) with `Mi355RecSession` as the session.  The S2 side's
                   host resize (`resize_norm_img`, cv2 in the reference) is done BEFORE the timed part with the numpy restatement; its
                   session calls and the host CTC decode are timed.
  (b) detection    `det_batch_predict` per 64-px size group, as `_run_ocr_det_batch` calls it, against the S2 seam: `Mi355DetSession` on
                   chunks of 8 host-preprocessed canvases (pre-process outside the timed part) plus the DB post-process on the host.  Random
                   weights find no text, so BOTH sides post-process maps drawn from the known line boxes: the model through `det_maps_fn`
                   (on the device), the S2 side `ocr_host.db_postprocess` on the host copy of the same maps.
  (c) warp stage   all lines of the workload by ONE `rd_line_warp_sources` launch against the existing route's loop, one
                   `rd_line_warp_batch` launch per source image; device events; the scratch buffers must be equal byte for byte.
  (d) lazy / eager `ocr(LazyLineCrops, det=False)` against `ocr(eager arrays, det=False)`.  What the eager arrays cost the HOST before the
                   call is reported next to it - measured on the numpy restatement of the crop (oracle/cv2_ops.py), a STAND-IN: the real
                   cost is cv2's and is not measured here (cv2 is absent).

All routes run in ONE process, alternated round by round after the warm-up; medians with min .. max.  Rule (docs/notebook/region_compose.md):
a new route is "recommended" iff its median is not above the old route's median plus the old route's own min-to-max spread.

    python tools/mb_ocr_model.py [--pages 32] [--steps 7] [--warmup 2] > profiles/mb_ocr_model.txt
"""
import argparse
import sys
import time
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def make_workload(n_pages: int):
    """-> [(region image BGR uint8 [h, w, 3], line boxes (x0, y0, x1, y1) in it)] - the regions of mb_region_compose.make_batch, cut out"""
    from mb_region_compose import make_batch
    pages, dets, lines = make_batch(n_pages)
    regions = []
    for p, page_dets in enumerate(dets):
        bb = np.asarray(lines[p], dtype=np.float64).reshape(-1, 4)
        for d in page_dets:
            if d["category_id"] != 1:
                continue
            x0, y0, x1, y1 = (int(v) for v in (d["poly"][0], d["poly"][1], d["poly"][4], d["poly"][5]))
            x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, pages.shape[2]), min(y1, pages.shape[1])
            inside = bb[(bb[:, 0] >= x0) & (bb[:, 2] <= x1) & (bb[:, 1] >= y0) & (bb[:, 3] <= y1)] - [x0, y0, x0, y0]
            if len(inside):
                regions.append((np.ascontiguousarray(pages[p, y0:y1, x0:x1]), inside))
    return regions


def quads_of(boxes):
    return [np.float32([[x0, y0], [x1, y0], [x1, y1], [x0, y1]]) for x0, y0, x1, y1 in boxes]


def stats(name, old, new, unit="ms"):
    o, n = np.asarray(old), np.asarray(new)
    spread = float(o.max() - o.min())
    ok = float(np.median(n)) <= float(np.median(o)) + spread
    print(f"{name}\n    old route  median {np.median(o):9.3f} {unit}  ({o.min():.3f} .. {o.max():.3f})\n"
          f"    new route  median {np.median(n):9.3f} {unit}  ({n.min():.3f} .. {n.max():.3f})   x{np.median(o) / np.median(n):.2f}\n"
          f"    rule: {np.median(n):.3f} <= {np.median(o):.3f} + {spread:.3f}  ->  {'recommended' if ok else 'stays opt-in'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert args.steps >= 7, "medians of at least 7 repetitions"
    import torch
    from oracle import cv2_ops
    from rapiddoc_amd import _lib, ocr_host
    from rapiddoc_amd import weights as W
    from rapiddoc_amd.ocr_model import Mi355RapidOcrModel, lazy_crop_function
    from rapiddoc_amd.pipeline import PagePipeline, render_text_maps
    from rapiddoc_amd.rec_plan import LINE_DTYPE, LINE_SOURCE_DTYPE, quads_to_crop_matrices
    from rapiddoc_amd.session import Mi355DetSession, Mi355RecSession

    assert torch.cuda.is_available(), "this tool measures on the GPU"
    lib = _lib.load()
    g = ROOT / "tests" / "golden"
    states = {k: W.synth_state_dict(W.load_manifest(g / f"manifest_{k}.json"), 0) for k in ("ppocrv6_det", "ppocrv6_rec")}
    pipe = PagePipeline(states, device=0)
    model = Mi355RapidOcrModel(pipe, det_db_box_thresh=0.3)
    regions = make_workload(args.pages)
    stream = torch.cuda.current_stream().cuda_stream

    # ---- the lines: per source its quads; descriptors of both warp routes over ONE scratch layout
    src_dev = [torch.from_numpy(img).cuda() for img, _b in regions]
    quads = [quads_of(b) for _img, b in regions]
    n_lines = sum(len(q) for q in quads)
    mats, cw, ch, ok = quads_to_crop_matrices(np.concatenate([np.stack(q) for q in quads]))
    assert ok.all()
    size = (3 * cw.astype(np.int64) * ch.astype(np.int64) + 15) // 16 * 16
    offs = np.cumsum(size) - size
    total = int(size.sum())
    ld = np.zeros(n_lines, LINE_DTYPE)
    ld["crop_w"], ld["crop_h"], ld["scratch_off"], ld["m"] = cw, ch, offs, mats
    sd = np.zeros(n_lines, LINE_SOURCE_DTYPE)
    sd["crop_w"], sd["crop_h"], sd["scratch_off"], sd["m"] = cw, ch, offs, mats
    first = np.cumsum([0] + [len(q) for q in quads])
    for s, t in enumerate(src_dev):
        sl = slice(first[s], first[s + 1])
        sd["src"][sl], sd["pitch"][sl], sd["W"][sl], sd["H"][sl] = t.data_ptr(), 3 * t.shape[1], t.shape[1], t.shape[0]
    ld_dev, sd_dev = torch.from_numpy(ld.view(np.uint8)).cuda(), torch.from_numpy(sd.view(np.uint8)).cuda()
    scratch_old = torch.zeros(total, dtype=torch.uint8, device="cuda")
    scratch_new = torch.zeros(total, dtype=torch.uint8, device="cuda")
    px = (cw * ch).astype(np.int64)

    def warp_old():
        for s, t in enumerate(src_dev):
            a, e = int(first[s]), int(first[s + 1])
            rc = lib.rd_line_warp_batch(0, t.data_ptr(), 1, t.shape[0], t.shape[1], ld_dev.data_ptr() + a * LINE_DTYPE.itemsize, e - a, int(px[a:e].max()),
                                        scratch_old.data_ptr(), stream)
            assert rc == 0

    def warp_new():
        assert lib.rd_line_warp_sources(0, sd.ctypes.data, sd_dev.data_ptr(), n_lines, scratch_new.data_ptr(), total, stream) == 0, lib.rd_create_error()

    def timed_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def timed_host(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    # ---- eager crops (the existing device warp, downloaded: the bytes an unmodified RapidDoc would hold) and lazy crops
    warp_old()
    host = scratch_old.cpu().numpy()
    eager = [host[o: o + 3 * w * h].reshape(h, w, 3).copy() for o, w, h in zip(offs.tolist(), cw.astype(int).tolist(), ch.astype(int).tolist())]
    assert not (ch / cw >= 2).any()
    lazy_fn = lazy_crop_function(lambda img, pts: (_ for _ in ()).throw(RuntimeError("a lazy crop was cut on the host")))
    lazy = [lazy_fn(img, q) for (img, _b), qs in zip(regions, quads) for q in qs]
    t0 = time.perf_counter()
    n_stand_in = min(n_lines, 64)
    k = 0
    for (img, _b), qs in zip(regions, quads):
        for q in qs:
            if k < n_stand_in:
                cv2_ops.get_rotate_crop_image(img, q)
            k += 1
    stand_in_ms = (time.perf_counter() - t0) * 1e3 / n_stand_in * n_lines

    # ---- (a) the S2 loop's inputs, resized on the host before anything is timed
    sess_rec = Mi355RecSession(states["ppocrv6_rec"])
    ratios = np.array([c.shape[1] / float(c.shape[0]) for c in eager])
    indices = np.argsort(ratios)
    chunks = []
    for beg in range(0, n_lines, 6):
        idxs = [int(i) for i in indices[beg: beg + 6]]
        r = max(320 / 48, max(ratios[i] for i in idxs))
        chunks.append((idxs, np.stack([cv2_ops.resize_norm_img(eager[i], r) for i in idxs]).astype(np.float32)))

    def s2_rec():
        out = [None] * n_lines
        for idxs, batch in chunks:
            preds = sess_rec(batch)
            for r, ts in enumerate(ocr_host.ctc_decode(preds.argmax(axis=2), preds.max(axis=2), pipe.characters)):
                out[idxs[r]] = ts
        return out

    # ---- (b) canvases per 64-px size group, their maps, the S2 side's host pre-process
    groups = {}
    for s, (img, boxes) in enumerate(regions):
        key = (-(-img.shape[0] // 64) * 64, -(-img.shape[1] // 64) * 64)
        groups.setdefault(key, []).append(s)
    canvases, maps_dev, maps_host, det_in = {}, {}, {}, {}
    for (gh, gw), members in groups.items():
        arr = np.full((len(members), gh, gw, 3), 255, np.uint8)
        for j, s in enumerate(members):
            img = regions[s][0]
            arr[j, : img.shape[0], : img.shape[1]] = img
        canvases[(gh, gw)] = [a for a in arr]
        dhw = ocr_host.det_resize_shape(gh, gw, 960, "max")
        maps_dev[(gh, gw)] = render_text_maps([regions[s][1] for s in members], (gh, gw), dhw, pipe.tdev)
        maps_host[(gh, gw)] = maps_dev[(gh, gw)].cpu().numpy()
        x = np.stack([cv2_ops.resize_linear_u8(a, dhw) for a in arr]).astype(np.float32) / 255.0          # DetPreProcess, BGR as rapidocr holds it
        x = ((x - np.float32(ocr_host.DET_MEAN)) / np.float32(ocr_host.DET_STD)).transpose(0, 3, 1, 2)
        det_in[(gh, gw)] = np.ascontiguousarray(x, dtype=np.float32)
    model.det_maps_fn = lambda hw, dhw, lo, n: maps_dev[hw][lo: lo + n]
    sess_det = Mi355DetSession(states["ppocrv6_det"])

    def new_det():
        return [model.det_batch_predict(canvases[key], min(len(canvases[key]), 16)) for key in groups]

    def s2_det():
        out = []
        for key, members in groups.items():
            for lo in range(0, len(members), 8):
                sess_det(det_in[key][lo: lo + 8])                                                           # the maps come home ...
                m = maps_host[key][lo: lo + 8]                                                               # ... and the drawn ones are post-processed
                out.append(ocr_host.db_postprocess(m, [key] * len(m), thresh=0.3, box_thresh=0.3, unclip_ratio=1.8))
        return out

    print(f"# tools/mb_ocr_model.py {' '.join(sys.argv[1:])}: {args.pages} pages, {len(regions)} region images in {len(groups)} size groups, {n_lines} text lines, "
          f"{total / 1e6:.1f} MB of line crops; {args.warmup} warm-up + {args.steps} timed rounds, routes alternating in one process")
    t = {name: [] for name in ("s2_rec", "pooled", "s2_det", "det", "warp_old", "warp_new", "eager", "lazy")}
    ref = {}
    for r in range(args.warmup + args.steps):
        row = {}
        row["s2_rec"], a_old = timed_host(s2_rec)
        row["pooled"], a_new = timed_host(lambda: model.ocr(eager, det=False)[0])
        row["s2_det"], _ = timed_host(s2_det)
        row["det"], b_new = timed_host(new_det)
        row["warp_old"] = timed_events(warp_old)
        row["warp_new"] = timed_events(warp_new)
        row["eager"], d_old = timed_host(lambda: model.ocr(eager, det=False)[0])
        row["lazy"], d_new = timed_host(lambda: model.ocr(lazy, det=False)[0])
        launches = (model.stats["warp_source_launches"], model.stats["rec_batches"])
        assert torch.equal(scratch_old, scratch_new), "the two warp routes wrote different bytes"
        assert d_old == d_new == a_new, "lazy and eager crops gave different lines"
        assert [x[0] for x in a_old] == [x[0] for x in a_new], "the pooled call and the chunk loop read different strings"
        crc = zlib.crc32(repr(a_new).encode())
        assert ref.setdefault("crc", crc) == crc
        n_boxes = sum(0 if b is None else len(b) for res in b_new for b, _e in res)
        for name, v in row.items():
            if r >= args.warmup:
                t[name].append(v)
        print(f"round {r:2d}{' (warm-up)' if r < args.warmup else '          '}  " + "  ".join(f"{name} {v:9.3f}" for name, v in row.items()) + "  ms", flush=True)
    score_diff = max(abs(x[1] - y[1]) for x, y in zip(a_old, a_new))
    print(f"lines crc32 {ref['crc']} ({n_lines} lines, strings equal to the chunk loop's on every round, largest score difference {score_diff:.3g}); "
          f"{n_boxes} boxes detected; warp bytes equal on every round; lazy call: {launches[0]} rd_line_warp_sources launches for {launches[1]} rec launches "
          f"and {len(regions)} sources")
    stats("(a) pooled rec: S2 chunk-of-6 loop through Mi355RecSession (old) / ocr(crops, det=False) (new); host clock around a synchronise", t["s2_rec"], t["pooled"])
    stats("(b) detection: Mi355DetSession + host DB post-process (old) / det_batch_predict (new); host clock around a synchronise", t["s2_det"], t["det"])
    stats(f"(c) warp stage: {len(regions)} rd_line_warp_batch launches (old) / 1 rd_line_warp_sources launch (new); device events", t["warp_old"], t["warp_new"])
    stats("(d) ocr(det=False) on eager arrays (old) / on lazy crops (new); host clock around a synchronise; the eager side's crops are NOT in its time", t["eager"], t["lazy"])
    print(f"    the eager arrays cost the host {stand_in_ms:.0f} ms before the call - STAND-IN: the numpy restatement of the crop, extrapolated from "
          f"{n_stand_in} lines; the real cost is cv2's and is not measured here")


if __name__ == "__main__":
    main()
