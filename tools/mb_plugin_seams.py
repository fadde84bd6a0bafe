#!/usr/bin/env python3
"""Microbenchmark of the two model seams as an unmodified RapidDoc drives them - with lists of NUMPY crops in host memory:

  (a) `analyze.RegionTextModel.batch_predict` on the text regions of the tools/mb_region_compose.py workload (32 synthetic pages, 21 regions
      each) handed over as BGR numpy crops, `host_images="copy"` (a torch.full per size group; per region a channel-reversed host copy and a
      synchronous upload) against `"stage"` (one pinned pack, one upload, one `rd_stage_canvases` launch);
  (b) `formula_host.FormulaRecognizer.batch_predict` on the 96 formula crops of tools/mb_formula_pre.py handed over as numpy,
      `host_images="host"` (Pillow per crop) against `"stage"` (one upload, then the device pre-process), decoder capped at 1 token.

One process, routes alternated round by round after the warm-up; the old route takes part twice ("a", "b") so that its spread against
itself is known.  Timed per round: the whole call (host clock around a synchronise) and, for (a), the composition alone between two device
events (the host work between the copies / launches is inside) and the `rd_stage_canvases` launch alone on descriptors that are already on
the device.  Reported: median and min .. max, bytes and bytes/s, crc32 of canvases / strings / ids (the routes must agree), and what the
rule of docs/notebook/region_compose.md says: the new route is recommended iff its median is not above the old route's median by more
than the old route's own min-to-max spread.

    python tools/mb_plugin_seams.py [--steps 7] [--warmup 2] > profiles/mb_plugin_seams.txt
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

HBM_COPY_TBS = 6.3          # what a copy reaches on this part


def region_crops(n_pages: int):
    """the text regions of mb_region_compose.make_batch as the custom-OCR seam gets them: BGR numpy crops without a margin, and per crop
    the text-line boxes inside it in crop coordinates"""
    import mb_region_compose as MB
    pages, dets, lines = MB.make_batch(n_pages)
    crops, boxes = [], []
    for p, page_dets in enumerate(dets):
        for d in page_dets:
            if d["category_id"] != 1:
                continue
            x0, y0, x1, y1 = int(d["poly"][0]), int(d["poly"][1]), int(d["poly"][4]), int(d["poly"][5])
            x0c, y0c, x1c, y1c = max(0, x0), max(0, y0), min(pages.shape[2], x1), min(pages.shape[1], y1)
            crops.append(np.ascontiguousarray(pages[p, y0c:y1c, x0c:x1c, ::-1]))
            bb = np.asarray(lines[p], dtype=np.float64).reshape(-1, 4)
            inside = bb[(bb[:, 0] >= x0) & (bb[:, 2] <= x1) & (bb[:, 1] >= y0) & (bb[:, 3] <= y1)]
            boxes.append(inside - [x0c, y0c, x0c, y0c])
    return crops, boxes


def stats(name, v, extra=""):
    v = np.asarray(v)
    print(f"{name:34s} median {np.median(v):10.3f}  min {v.min():10.3f}  max {v.max():10.3f}  ms{extra}")


def verdict(what, old_a, old_b, new):
    old = np.asarray(list(old_a) + list(old_b))
    med_old, med_new, spread = float(np.median(old)), float(np.median(new)), float(old.max() - old.min())
    ok = med_new <= med_old + spread
    print(f"rule ({what}): stage median {med_new:.2f} ms, old route median {med_old:.2f} ms over both participants, its min-to-max spread "
          f"{spread:.2f} ms -> stage is {'RECOMMENDED' if ok else 'NOT recommended'} ({med_new:.2f} {'<=' if ok else '>'} {med_old + spread:.2f})")


def bench_region(args):
    import torch
    from rapiddoc_amd import _lib, analyze, ocr_host
    from rapiddoc_amd import host_stage as HS
    from rapiddoc_amd import weights as W
    from rapiddoc_amd.pipeline import PagePipeline, render_text_maps

    g = ROOT / "tests" / "golden"
    pipe = PagePipeline({k: W.synth_state_dict(W.load_manifest(g / f"manifest_{k}.json"), 0) for k in ("ppocrv6_det", "ppocrv6_rec")}, device=0)
    crops, boxes = region_crops(args.pages)
    maps_cache = {}

    def maps_fn(ids, ghw, dhw):
        key = (ghw, tuple(ids))
        if key not in maps_cache:
            maps_cache[key] = render_text_maps([boxes[i] for i in ids], ghw, dhw, pipe.tdev)
        return maps_cache[key]

    models = {"copy a": analyze.RegionTextModel(pipe), "stage": analyze.RegionTextModel(pipe, host_images="stage"), "copy b": analyze.RegionTextModel(pipe)}
    shapes = [(c.shape[0], c.shape[1]) for c in crops]
    keep = list(range(len(crops)))
    groups = ocr_host.det_buckets(shapes, ["_"] * len(crops), det_batch_num=len(crops))
    crop_bytes = sum(c.size for c in crops)
    canvas_bytes = sum(len(m) * gh * gw * 3 for _l, (gh, gw), m, _b in groups)
    print(f"# (a) RegionTextModel.batch_predict: {len(crops)} BGR numpy crops ({crop_bytes / 1e6:.1f} MB) of {args.pages} pages in {len(groups)} size groups, "
          f"{canvas_bytes / 1e6:.1f} MB of canvases; {args.warmup} warm-up + {args.steps} timed rounds, routes alternating in one process")

    def compose_only(model):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        canvases = model._canvases(crops, shapes, keep, groups)
        e1.record()
        torch.cuda.synchronize()
        crc = 0
        for c in canvases:
            crc = zlib.crc32(c.cpu().numpy().tobytes(), crc)
        return e0.elapsed_time(e1), crc

    def whole_call(model):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        texts = model.batch_predict(crops, det_maps_fn=maps_fn, batch_size=16)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, zlib.crc32("\x00".join(texts).encode()), sum(1 for t in texts if t)

    # the launch alone: the crops already uploaded, the descriptors already on the device
    lib = _lib.load()
    stage = HS.HostImageStage(pipe.tdev)
    staged = stage.upload(crops)
    canvases = [torch.empty((len(m), gh, gw, 3), dtype=torch.uint8, device=pipe.tdev) for _l, (gh, gw), m, _b in groups]
    descs = HS.pack_stage_descs(staged.base, staged.offsets, staged.shapes, [((gh, gw), m) for _l, (gh, gw), m, _b in groups], [c.data_ptr() for c in canvases])
    descs_dev = torch.from_numpy(descs.view(np.uint8).reshape(-1).copy()).to(pipe.tdev)

    def kernel_only():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        rc = lib.rd_stage_canvases(0, descs.ctypes.data, descs_dev.data_ptr(), len(descs), torch.cuda.current_stream().cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0, lib.rd_create_error()
        return e0.elapsed_time(e1)

    def pack_upload_only():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stage.upload(crops)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3

    comp = {k: [] for k in models}
    whole = {k: [] for k in models}
    kern, pack, upl = [], [], []
    crcs = {}
    for r in range(args.warmup + args.steps):
        row = []
        for name, model in models.items():
            c_ms, c_crc = compose_only(model)
            w_ms, w_crc, n_text = whole_call(model)
            assert crcs.setdefault("canvases", c_crc) == c_crc, (name, "the canvases differ between the routes")
            assert crcs.setdefault("texts", w_crc) == w_crc, (name, "the strings differ between the routes")
            row.append(f"{name}: compose {c_ms:8.3f}  call {w_ms:9.2f}")
            if r >= args.warmup:
                comp[name].append(c_ms)
                whole[name].append(w_ms)
        k_ms = kernel_only()
        p_ms, u_ms = pack_upload_only()
        if r >= args.warmup:
            kern.append(k_ms)
            pack.append(p_ms)
            upl.append(u_ms)
        print(f"round {r:2d}{' (warm-up)' if r < args.warmup else '          '}  " + "  ".join(row) + f"  kernel {k_ms:7.4f}  pack {p_ms:7.3f}  pack+copy {u_ms:7.3f}  ms", flush=True)
    print(f"canvases crc32 {crcs['canvases']}  strings crc32 {crcs['texts']} ({n_text} regions with text): equal on every route and round")
    for name in models:
        stats(f"(a) {name}: composition", comp[name])
    for name in models:
        stats(f"(a) {name}: whole call", whole[name])
    k = float(np.median(kern))
    stats("(a) rd_stage_canvases alone", kern, f"   {crop_bytes + canvas_bytes} bytes read + written -> {(crop_bytes + canvas_bytes) / k / 1e9:.3f} TB/s "
          f"at the median = {(crop_bytes + canvas_bytes) / k / 1e9 / HBM_COPY_TBS:.2f} of the {HBM_COPY_TBS} TB/s a copy reaches (DESIGN.md)")
    stats("(a) rd_stage_pack + enqueue (host)", pack, f"   {crop_bytes / np.median(pack) / 1e6:.2f} GB/s of crop bytes")
    stats("(a) pack + upload, synchronised", upl, f"   {crop_bytes / np.median(upl) / 1e6:.2f} GB/s of crop bytes")
    verdict("a, whole call", whole["copy a"], whole["copy b"], whole["stage"])
    verdict("a, composition", comp["copy a"], comp["copy b"], comp["stage"])


def bench_formula(args):
    import json

    import mb_formula_pre as MF
    import torch
    from rapiddoc_amd import weights as W
    from rapiddoc_amd.formula_host import FormulaRecognizer

    state = W.synth_state_dict(W.load_manifest(ROOT / "tests" / "golden" / "manifest_ppformulanet_plus_m_m8.json"), 0)
    models = {"host a": FormulaRecognizer(state, max_new_tokens=1), "stage": FormulaRecognizer(state, max_new_tokens=1, host_images="stage"),
              "host b": FormulaRecognizer(state, max_new_tokens=1)}
    pages, dets = MF.make_batch()
    crops = []
    for p, page_dets in enumerate(dets):
        for d in page_dets:
            x0, y0, x1, y1 = d["poly"][0], d["poly"][1], d["poly"][4], d["poly"][5]
            crops.append(pages[p, y0:y1, x0:x1])                  # windows of the page array, as the reference slices them
    print(f"# (b) FormulaRecognizer.batch_predict: {len(crops)} numpy crops ({sum(c.size for c in crops) / 1e6:.1f} MB), batch_size 16, max_new_tokens 1; "
          f"{args.warmup} warm-up + {args.steps} timed rounds, routes alternating in one process")
    ms = {k: [] for k in models}
    crc0 = None
    for r in range(args.warmup + args.steps):
        row = []
        for name, model in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids = model.batch_predict(crops, batch_size=16)
            torch.cuda.synchronize()
            t = (time.perf_counter() - t0) * 1e3
            crc = zlib.crc32(json.dumps(ids).encode())
            crc0 = crc if crc0 is None else crc0
            assert crc == crc0, (name, "the ids differ between the routes")
            row.append(f"{name}: {t:9.2f}")
            if r >= args.warmup:
                ms[name].append(t)
        print(f"round {r:2d}{' (warm-up)' if r < args.warmup else '          '}  " + "  ".join(row) + "  ms", flush=True)
    print(f"ids crc32 {crc0}: equal on every route and round")
    for name, model in models.items():
        routes = {k: model.last_routes.count(k) for k in sorted(set(model.last_routes))}
        stats(f"(b) {name}: whole call", ms[name], f"   routes {routes}")
    verdict("b, whole call", ms["host a"], ms["host b"], ms["stage"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["a", "b"], default=None)
    args = ap.parse_args()
    assert args.steps >= 7, "medians of at least 7 repetitions"
    print(f"# tools/mb_plugin_seams.py {' '.join(sys.argv[1:])}")
    if args.only in (None, "a"):
        bench_region(args)
    if args.only in (None, "b"):
        bench_formula(args)


if __name__ == "__main__":
    main()
