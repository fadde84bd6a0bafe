#!/usr/bin/env python3
"""Microbenchmark of the PP-OCRv5 mobile detector (`ppocrv5_det_mobile`; bench.py measures the default v6 path and stays as it is).

  1. the forward at [pages, 3, 960, 704] (the size the page pipeline runs, 32 pages) in the `auto` and `fp32` precision modes: ms per
     launch (HIP events, after warm-up, median of the timed launches), the plan's arena size, and the per-op-kind table of one profiled
     launch (rd_set_profiling: per-op HIP events, so launch gaps are inside the op times); the v6 detector at the same batch, in the same
     run, beside it; with --routes also the forward with every depthwise layer forced on one route (RD_LCV3_DW2D=0 / 1);
  2. every depthwise layer of the backbone alone at its real shape on the direct kernel (csrc/kernels_lcv3.hip) and on the LDS-staged
     kernel (csrc/kernels_lcv3_det.hip): same operands, same run, the routes alternating (rd_debug_lcv3_dw_det, iters > 0, `reps`
     repeats per route).  Per route the median, the repeat spread (max - min) / median of THAT route, GB/s on algorithmic bytes (input
     read once + output written once).  `staged wins` = the staged median is below the direct median by more than the larger of the two
     spreads: the rule that sets lcv3_dw2d_default (csrc/builder_mobile.cpp).

    python tools/mb_det_mobile.py [--steps 7] [--warmup 3] [--pages 32] > profiles/mb_det_mobile.txt
"""
import argparse
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from rapiddoc_amd import _lib  # noqa: E402
from rapiddoc_amd import weights as W  # noqa: E402
from rapiddoc_amd.engine import RdEngine  # noqa: E402

H, W_ = 960, 704
KIND = "ppocrv5_det_mobile"
# (block, k, C of the depthwise layer, stride, level of its input: 1 = H/2 ... 5 = H/32)
DW_LAYERS = [("blocks2.0", 3, 16, 1, 1), ("blocks3.0", 3, 32, 2, 1), ("blocks3.1", 3, 48, 1, 2), ("blocks4.0", 3, 48, 2, 2), ("blocks4.1", 3, 96, 1, 3),
             ("blocks5.0", 3, 96, 2, 3), ("blocks5.1-4", 5, 192, 1, 4), ("blocks6.0", 5, 192, 2, 4), ("blocks6.1-3", 5, 384, 1, 5)]


def ev_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def forward_section(kind, st, x, precision, steps, warmup, table=True, label=""):
    eng = RdEngine(kind, guard="off").load_weights(st).set_precision(precision)
    out = torch.empty((x.shape[0], 1, H, W_), device="cuda")
    for _ in range(warmup):
        eng.det_forward(x, out=out)
    torch.cuda.synchronize()
    ms = [ev_ms(lambda: eng.det_forward(x, out=out)) for _ in range(steps)]
    med = float(np.median(ms))
    arena = eng.workspace_bytes(x.shape[0], H, W_)
    print(f"\n== {kind}{label} forward [{x.shape[0]}, 3, {H}, {W_}] precision {precision}: median {med:.2f} ms (min {min(ms):.2f}, max {max(ms):.2f}; {steps} timed "
          f"launches after {warmup} warm-up) = {x.shape[0] / med * 1e3:.1f} pages/s; arena {arena / 1e9:.2f} GB; range flag {int(eng.range_overflow())}; "
          f"plan stats {eng.plan_stats()}")
    if table:
        eng.set_profiling(True)
        eng.profile_log.clear()
        eng.det_forward(x, out=out)
        eng.set_profiling(False)
        agg = {}
        for r in eng.profile_log:
            t = agg.setdefault((r["kind"], r["cfg"]), [0, 0.0, 0.0, 0.0])
            t[0] += 1; t[1] += r["ms"]; t[2] += r["flops"]; t[3] += r["bytes"]
        tot = sum(t[1] for t in agg.values())
        print(f"per-op-kind table of one profiled launch (sum of op times {tot:.2f} ms, {sum(t[2] for t in agg.values()) / 1e12:.3f} TFLOP)")
        print(f"{'kind':18s} {'cfg':22s} {'ops':>5s} {'ms':>9s} {'share':>6s} {'TFLOP/s':>8s} {'GB/s':>8s}")
        for (k, cfg), t in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            print(f"{k:18s} {cfg:22s} {t[0]:5d} {t[1]:9.3f} {t[1] / tot:6.1%} {t[2] / max(t[1], 1e-9) / 1e9:8.1f} {t[3] / max(t[1], 1e-9) / 1e6:8.0f}")
        if kind == KIND:
            for r in eng.profile_log:
                if r["kind"].startswith("lcv3_dw"):
                    print(f"  dw {r['name'][len('backbone.'):-len('.dw_conv.fold.weight')]:10s} {r['shape']:22s} {r['cfg']:18s} {r['ms']:8.3f} ms {r['bytes'] / r['ms'] / 1e6:7.0f} GB/s")
    eng.close()
    return med


def dw_section(pages, iters, reps):
    lib = _lib.load()
    fn = lib.rd_debug_lcv3_dw_det
    g = torch.Generator(device="cuda").manual_seed(0)
    aff = np.asarray([1.05, 0.02, 0.95, -0.03], np.float32)
    print(f"\n== the depthwise layers alone, {pages} pages, pre-activation on load as in the network: direct (lcv3_dw_kernel) vs LDS-staged (lcv3_dw2d_kernel), "
          f"alternating, {reps} repeats of {iters} launches per route")
    print(f"{'layer':12s} {'shape [N,H,W,C]':22s} {'k':>2s} {'s':>2s} {'lvl':>3s} {'MB':>7s} {'direct ms':>10s} {'spread':>7s} {'GB/s':>7s} {'staged ms':>10s} {'spread':>7s} {'GB/s':>7s} "
          f"{'d / s':>6s} {'max |d|':>9s}  staged wins")
    for name, k, c, s, lvl in DW_LAYERS:
        h, w = H >> lvl, W_ >> lvl
        oh, ow = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
        x = torch.rand((pages, h, w, c), device="cuda", generator=g) * 8 - 4
        wt = (torch.rand((k * k, c), device="cuda", generator=g) - 0.5) * (1.2 / k)
        b = torch.rand((c,), device="cuda", generator=g) - 0.5
        y = [torch.empty((pages, oh, ow, c), device="cuda") for _ in range(2)]
        pre, post = int(name != "blocks2.0"), int(s == 1)
        t = {0: [], 1: []}
        for _rep in range(reps):
            for route in (0, 1):
                ms = fn(pages, h, w, c, k, s, pre, post, route, iters, aff.ctypes.data, x.data_ptr(), wt.data_ptr(), b.data_ptr(), y[route].data_ptr())
                assert ms >= 0
                t[route].append(ms)
        torch.cuda.synchronize()
        mb = 4.0 * (x.numel() + y[0].numel())
        med = [float(np.median(t[r])) for r in (0, 1)]
        spr = [(max(t[r]) - min(t[r])) / med[r] for r in (0, 1)]
        wins = med[1] < med[0] * (1.0 - max(spr))
        print(f"{name:12s} {f'[{pages},{h},{w},{c}]':22s} {k:2d} {s:2d} {lvl:3d} {mb / 1e6:7.1f} {med[0]:10.4f} {spr[0]:7.1%} {mb / med[0] / 1e6:7.0f} {med[1]:10.4f} {spr[1]:7.1%} "
              f"{mb / med[1] / 1e6:7.0f} {med[0] / med[1]:6.2f} {float((y[0] - y[1]).abs().max()):9.2e}  {'yes' if wins else 'no'}")
        del x, y
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--routes", action="store_true", help="also time the forward with RD_LCV3_DW2D=0 and =1")
    a = ap.parse_args()
    gd = ROOT / "tests/golden"
    st = W.synth_state_dict(W.load_manifest(gd / f"manifest_{KIND}.json"), 0, kind=KIND)
    st6 = W.synth_state_dict(W.load_manifest(gd / "manifest_ppocrv6_det.json"), 0)
    x = torch.rand((a.pages, 3, H, W_), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)) * 2 - 1
    print(f"device {torch.cuda.get_device_name(0)}")
    for precision in ("auto", "fp32"):
        forward_section(KIND, st, x, precision, a.steps, a.warmup)
    forward_section("ppocrv6_det", st6, x, "auto", a.steps, a.warmup, table=False)
    if a.routes:
        old = os.environ.get("RD_LCV3_DW2D")
        for route in ("0", "1", "0", "1"):
            os.environ["RD_LCV3_DW2D"] = route          # read per plan: a fresh engine plans under it
            forward_section(KIND, st, x, "auto", a.steps, a.warmup, table=False, label=f" RD_LCV3_DW2D={route}")
        if old is None:
            del os.environ["RD_LCV3_DW2D"]
        else:
            os.environ["RD_LCV3_DW2D"] = old
    del x
    torch.cuda.empty_cache()
    dw_section(a.pages, a.iters, a.reps)


if __name__ == "__main__":
    main()
