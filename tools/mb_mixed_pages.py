#!/usr/bin/env python3
"""Microbenchmark of page batches of mixed page sizes: `rd_preproc_resize_norm_sources` (one launch for sources of any sizes) against
the per-source loop it replaces, at the four places that use it.

  (a) 32 pages of four sizes around 1684 x 1191 on the device: ONE sources launch against 32 `rd_preproc_resize_norm` launches, for the
      det input (linear, every page to its own det shape) and the layout input (cubic, 800 x 800); device events.
  (b) `PagePipeline.run_batch` on a LIST of 24 portrait + 8 landscape 1684 x 1191 pages against two `run_batch` calls on the two size
      groups; host clock around a synchronise.  This compares TIME only: the strings differ by design, because the list call pools the
      lines of all 32 pages into one strict plan and the two group calls pool 24 and 8 (the padded widths differ).
  (c) `LayoutModel.preprocess` on 32 HOST pages of the sizes of (a): `preprocess_loop` (a copy and a launch per page) against
      `preprocess_sources` (one pack, one copy, one launch); host clock around a synchronise.
  (d) the pre-process of `Mi355UniTableStructure(resize="linear")` on 32 host tables of mixed sizes, loop against one launch; host clock.

One MI355X, the routes alternated in one process, 2 warm-up + 7 timed rounds, medians with min .. max.  Rule (docs/notebook/
region_compose.md): the new route is recommended iff its median is not above the old route's median plus the old route's own
min-to-max spread.

    python tools/mb_mixed_pages.py [--steps 7] [--warmup 2] [--only a,b,c,d] > profiles/mb_mixed_pages.txt
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SIZES = [(1684, 1191), (1191, 1684), (1754, 1240), (1650, 1275)]      # A4 at 144 dpi, the same sheet turned, A4 at 150 dpi, Letter at 150 dpi


def report(title, old, new):
    o, n = np.asarray(old), np.asarray(new)
    mo, mn, spread = float(np.median(o)), float(np.median(n)), float(o.max() - o.min())
    print(f"{title}\n    old  median {mo:9.3f} ms  ({o.min():.3f} .. {o.max():.3f})\n    new  median {mn:9.3f} ms  ({n.min():.3f} .. {n.max():.3f})   x{mo / mn:.2f}")
    print(f"    rule: new is recommended iff {mn:.3f} <= {mo:.3f} + {spread:.3f}  ->  {'RECOMMENDED' if mn <= mo + spread else 'not recommended'}", flush=True)


def alternate(old_fn, new_fn, steps, warmup, timer):
    old, new = [], []
    for r in range(warmup + steps):
        a, b = timer(old_fn), timer(new_fn)
        if r >= warmup:
            old.append(a)
            new.append(b)
    return old, new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="a,b,c,d")
    args = ap.parse_args()
    assert args.steps >= 7, "medians of at least 7 repetitions"
    only = set(args.only.split(","))
    import torch
    from rapiddoc_amd import ocr_host
    from rapiddoc_amd import weights as W
    from rapiddoc_amd.engine import preproc_resize_norm, preproc_resize_norm_sources
    from rapiddoc_amd.pages import synth_page
    from rapiddoc_amd.pipeline import PagePipeline, page_det_shape, render_text_maps

    def dev_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def host_clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    print(f"# tools/mb_mixed_pages.py {' '.join(sys.argv[1:])}: {torch.cuda.get_device_name(0)}; {args.warmup} warm-up + {args.steps} timed rounds, "
          f"routes alternating in one process; medians (min .. max)")
    rng = np.random.default_rng(0)
    host_pages = [rng.integers(0, 256, SIZES[i % 4] + (3,), dtype=np.uint8) for i in range(32)]

    if "a" in only:
        pages = [torch.from_numpy(p).cuda() for p in host_pages]
        for name, kw, out_hws in (("det (linear)", dict(mean=ocr_host.DET_MEAN, std=ocr_host.DET_STD, interp=1, swap_rb=True), [page_det_shape(*p.shape[:2]) for p in pages]),
                                  ("layout (cubic)", dict(interp=2), [(800, 800)] * 32)):
            outs = [torch.empty((3,) + hw, dtype=torch.float32, device="cuda") for hw in out_hws]
            outs2 = [torch.empty_like(o) for o in outs]

            def loop():
                for p, hw, o in zip(pages, out_hws, outs):
                    preproc_resize_norm(p, hw, out=o, **kw)
            old, new = alternate(loop, lambda: preproc_resize_norm_sources(pages, out_hws, out=outs2, **kw), args.steps, args.warmup, dev_events)
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs, outs2)), "the routes' bits differ"
            report(f"(a) {name}: 32 device pages of four sizes, 32 rd_preproc_resize_norm launches (old) / 1 rd_preproc_resize_norm_sources launch (new); "
                   f"device events; bits equal", old, new)

    if "b" in only:
        g = ROOT / "tests" / "golden"
        pipe = PagePipeline({k: W.synth_state_dict(W.load_manifest(g / f"manifest_{k}.json"), 0) for k in ("ppocrv6_det", "ppocrv6_rec", "pphgnetv2_b4")}, device=0)
        pages, boxes = [], []
        for i in range(32):
            page, bx = synth_page(i)
            bx = np.asarray(bx, dtype=np.float32).reshape(-1, 4)
            if i % 4 == 3:             # every fourth sheet lies on its side: the top of the page on the left, white on the right
                land = np.full((1191, 1684, 3), 255, np.uint8)
                land[:, :1191] = page[:1191]
                page, bx = land, bx[bx[:, 3] < 1185]
            pages.append(torch.from_numpy(np.ascontiguousarray(page)).cuda())
            boxes.append(bx)
        maps = [render_text_maps([b], tuple(p.shape[:2]), page_det_shape(*p.shape[:2]), p.device) for p, b in zip(pages, boxes)]
        port, land = [i for i in range(32) if i % 4 != 3], [i for i in range(32) if i % 4 == 3]
        t_port, t_land = torch.stack([pages[i] for i in port]), torch.stack([pages[i] for i in land])
        m_port, m_land = torch.cat([maps[i] for i in port]), torch.cat([maps[i] for i in land])
        counts = {}

        def two_calls():
            r = pipe.run_batch(t_port, None, det_maps_override=m_port) + pipe.run_batch(t_land, None, det_maps_override=m_land)
            counts["old"] = sum(len(x.lines) for x in r)

        def one_list():
            r = pipe.run_batch(pages, None, det_maps_override=maps)
            counts["new"] = sum(len(x.lines) for x in r)
        old, new = alternate(two_calls, one_list, args.steps, args.warmup, host_clock)
        report(f"(b) run_batch: 24 portrait + 8 landscape 1684 x 1191 pages, two calls on the size groups (old, {counts['old']} lines) / one call on the list "
               f"(new, {counts['new']} lines, {int(pipe.stats['det_groups'])} det groups, {int(pipe.stats['rec_batches'])} rec launches); host clock.  TIME only: "
               f"the strings differ by design (the list pools all 32 pages' lines into one strict plan)", old, new)

    if "c" in only:
        from rapiddoc_amd.layout_model import LayoutModel, SyntheticBoxSession
        model = LayoutModel(SyntheticBoxSession(["text"], boxes_per_page=2), "pp_doclayoutv3")
        res = {}
        old, new = alternate(lambda: res.__setitem__("old", model.preprocess_loop(host_pages)[0]), lambda: res.__setitem__("new", model.preprocess_sources(host_pages)[0]),
                             args.steps, args.warmup, host_clock)
        assert torch.equal(res["old"].view(torch.int32), res["new"].view(torch.int32)), "the routes' bits differ"
        report("(c) LayoutModel.preprocess: 32 host pages of four sizes, preprocess_loop (old) / preprocess_sources (new); host clock; bits equal", old, new)

    if "d" in only:
        from rapiddoc_amd import table_unitable as TU
        m = object.__new__(TU.Mi355UniTableStructure)          # the pre-process alone: it reads no weights, so no engine is built
        m.resize, m._dev = "linear", torch.device("cuda", 0)
        tables = [W.synth_table_crop(i, 200 + 37 * (i % 7), 300 + 53 * (i % 5)) for i in range(32)]
        res = {}

        def run(route):
            TU.Mi355UniTableStructure.LINEAR_ROUTE = route
            res[route] = m.preprocess(tables)[0]
        keep = TU.Mi355UniTableStructure.LINEAR_ROUTE
        old, new = alternate(lambda: run("loop"), lambda: run("sources"), args.steps, args.warmup, host_clock)
        TU.Mi355UniTableStructure.LINEAR_ROUTE = keep
        assert torch.equal(res["loop"].view(torch.int32), res["sources"].view(torch.int32)), "the routes' bits differ"
        report("(d) Mi355UniTableStructure(resize='linear').preprocess: 32 host tables of mixed sizes, one copy + launch per table (old) / one pack, copy and "
               "launch (new); host clock; bits equal", old, new)


if __name__ == "__main__":
    main()
