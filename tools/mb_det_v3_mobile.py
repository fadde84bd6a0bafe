#!/usr/bin/env python3
"""Microbenchmark of the PP-OCRv3 multilingual detector (`ppocrv3_det_mobile`; bench.py measures the default v6 path and stays as it is).

  1. the forward at [pages, 3, 960, 704] (the size the page pipeline runs, 32 pages) in the `auto` and `fp32` precision modes: ms per
     launch (HIP events, after warm-up, median of the timed launches), the plan's arena size and the per-op-kind table of one profiled
     launch; `ppocrv5_det_mobile` at the same batch, in the same run, beside it;
  2. --routes: the per-block A/B of the inverted-residual blocks that mbv3_block_kernel (csrc/kernels_mbv3.hip) can take.  Two engines
     on the same input and weights, one planned under RD_MBV3_FUSED=0 and one under =1, run profiled launches in turn (`reps` each,
     alternating).  Per block: unfused = the sum of its expand, depthwise and linear ops (block 0: plus the hardswish pass over conv1's
     output that the fused kernel applies on load), fused = its one op.  Per route the median, the spread (max - min) / median of THAT
     route, and GB/s counted on the block's input read once plus its output written once.  `fused wins` = the fused median lies below
     the unfused one by more than the larger of the two spreads: the rule that sets mbv3_fused_default (csrc/builder_mobile.cpp).  Per-op HIP
     events include the launch gap of every op, which the unfused route pays three times: that is part of what a forward pays, too.
     Then the whole forward under either setting, alternating; and the hardswish depthwise layers with C % 16 == 0 alone at their real
     shapes on mbv3_dw_kernel and on the LDS-staged lcv3_dw2d_kernel (csrc/kernels_lcv3_det.hip), alternating, by the same rule: the
     table that sets mbv3_dw2d_default.

    python tools/mb_det_v3_mobile.py [--routes] [--steps 7] [--warmup 3] [--pages 32] > profiles/mb_det_v3_mobile.txt
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
KIND = "ppocrv3_det_mobile"
# (stage, index, k, cin, mid, cout, stride, level of the input map: 1 = H/2 ...)
BLOCKS = [(0, 0, 3, 8, 8, 8, 1, 1), (0, 1, 3, 8, 32, 16, 2, 1), (0, 2, 3, 16, 40, 16, 1, 2), (1, 0, 5, 16, 40, 24, 2, 2), (1, 1, 5, 24, 64, 24, 1, 3),
          (1, 2, 5, 24, 64, 24, 1, 3)]


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
          f"launches after {warmup} warm-up) = {x.shape[0] / med * 1e3:.1f} pages/s; arena {arena / 1e9:.2f} GB; range flag {int(eng.range_overflow())}")
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
        print(f"{'kind':18s} {'cfg':24s} {'ops':>5s} {'ms':>9s} {'share':>6s} {'TFLOP/s':>8s} {'GB/s':>8s}")
        for (k, cfg), t in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            print(f"{k:18s} {cfg:24s} {t[0]:5d} {t[1]:9.3f} {t[1] / tot:6.1%} {t[2] / max(t[1], 1e-9) / 1e9:8.1f} {t[3] / max(t[1], 1e-9) / 1e6:8.0f}")
        if kind == KIND:
            for r in eng.profile_log:
                if r["name"].startswith("backbone.stages.") or r["kind"] in ("stem3x3s2", "lcv3_act"):
                    print(f"  {r['name'][len('backbone.'):] if r['name'].startswith('backbone.') else r['name']:44s} {r['kind']:12s} {r['cfg']:22s} {r['ms']:8.3f} ms "
                          f"{r['bytes'] / r['ms'] / 1e6:7.0f} GB/s")
    eng.close()
    return med


def _planned(st, route, precision):
    os.environ["RD_MBV3_FUSED"] = route            # read per plan: the first forward of a fresh engine plans under it
    return RdEngine(KIND, guard="off").load_weights(st).set_precision(precision)


def routes_section(st, x, reps, precision="auto"):
    old = os.environ.get("RD_MBV3_FUSED")
    engs = {r: _planned(st, r, precision) for r in ("0", "1")}
    out = torch.empty((x.shape[0], 1, H, W_), device="cuda")
    for r in ("0", "1"):
        os.environ["RD_MBV3_FUSED"] = r
        for _ in range(2):
            engs[r].det_forward(x, out=out)
    times = {r: {b[:2]: [] for b in BLOCKS} for r in ("0", "1")}
    bytes_ = {}
    for _rep in range(reps):
        for r in ("0", "1"):
            os.environ["RD_MBV3_FUSED"] = r
            e = engs[r]
            e.set_profiling(True)
            e.profile_log.clear()
            e.det_forward(x, out=out)
            e.set_profiling(False)
            log = list(e.profile_log)
            for s, i, *_ in BLOCKS:
                p = f"backbone.stages.{s}.{i}"
                ops = [q for q in log if q["name"] == p or q["name"].startswith(p + ".")]
                assert len(ops) == (1 if r == "1" else 3), (p, [q["kind"] for q in ops])
                ms = sum(q["ms"] for q in ops)
                if r == "0" and (s, i) == (0, 0):
                    ms += next(q["ms"] for q in log if q["kind"] == "lcv3_act")       # the hardswish pass over conv1's output
                if r == "1":
                    bytes_[(s, i)] = ops[0]["bytes"]
                times[r][(s, i)].append(ms)
    print(f"\n== per-block A/B, {x.shape[0]} pages at {H} x {W_}, precision {precision}: unfused (expand -> mbv3_dw_kernel -> linear) vs fused (mbv3_block_kernel), per-op HIP "
          f"events of profiled launches, the two engines alternating, {reps} launches per route")
    print(f"{'block':6s} {'k':>2s} {'s':>2s} {'cin-mid-cout':>13s} {'lvl':>3s} {'MB in+out':>10s} {'unfused ms':>11s} {'spread':>7s} {'GB/s':>7s} {'fused ms':>9s} {'spread':>7s} {'GB/s':>7s} "
          f"{'u / f':>6s}  fused wins")
    for s, i, k, cin, mid, cout, stride, lvl in BLOCKS:
        t = [times[r][(s, i)] for r in ("0", "1")]
        med = [float(np.median(v)) for v in t]
        spr = [(max(v) - min(v)) / m for v, m in zip(t, med)]
        wins = med[1] < med[0] * (1.0 - max(spr))
        mb = bytes_[(s, i)]
        print(f"{f'{s}.{i}':6s} {k:2d} {stride:2d} {f'{cin}-{mid}-{cout}':>13s} {lvl:3d} {mb / 1e6:10.1f} {med[0]:11.4f} {spr[0]:7.1%} {mb / med[0] / 1e6:7.0f} {med[1]:9.4f} {spr[1]:7.1%} "
              f"{mb / med[1] / 1e6:7.0f} {med[0] / med[1]:6.2f}  {'yes' if wins else 'no'}")
    fw = {r: [] for r in ("0", "1")}
    for _rep in range(reps):
        for r in ("0", "1"):
            os.environ["RD_MBV3_FUSED"] = r
            fw[r].append(ev_ms(lambda: engs[r].det_forward(x, out=out)))
    for r in ("0", "1"):
        m = float(np.median(fw[r]))
        print(f"forward with RD_MBV3_FUSED={r}: median {m:.2f} ms (min {min(fw[r]):.2f}, max {max(fw[r]):.2f})")
    for e in engs.values():
        e.close()
    if old is None:
        del os.environ["RD_MBV3_FUSED"]
    else:
        os.environ["RD_MBV3_FUSED"] = old


# hardswish depthwise layers with C % 16 == 0: (block, k, C, stride, level of the input map)
DW_LAYERS = [("2.2-3", 3, 96, 1, 4), ("2.4", 3, 240, 1, 4), ("2.5", 3, 336, 1, 4), ("3.0", 5, 336, 2, 4), ("3.1-2", 5, 480, 1, 5)]


def dw_section(pages, iters, reps):
    lib = _lib.load()
    direct, staged = lib.rd_debug_mbv3_dw, lib.rd_debug_lcv3_dw_det
    g = torch.Generator(device="cuda").manual_seed(0)
    aff = np.asarray([1.0, 0.0, 1.0, 0.0], np.float32)
    print(f"\n== the hardswish depthwise layers with C % 16 == 0 alone, {pages} pages, hardswish on load and in the epilogue: direct (mbv3_dw_kernel) vs LDS-staged "
          f"(lcv3_dw2d_kernel), alternating, {reps} repeats of {iters} launches per route")
    print(f"{'block':6s} {'shape [N,H,W,C]':22s} {'k':>2s} {'s':>2s} {'lvl':>3s} {'MB':>7s} {'direct ms':>10s} {'spread':>7s} {'GB/s':>7s} {'staged ms':>10s} {'spread':>7s} {'GB/s':>7s} "
          f"{'d / s':>6s} {'max |d|':>9s}  staged wins")
    for name, k, c, s, lvl in DW_LAYERS:
        h, w = H >> lvl, W_ >> lvl
        oh, ow = (h - 1) // s + 1, (w - 1) // s + 1
        x = torch.rand((pages, h, w, c), device="cuda", generator=g) * 8 - 4
        wt = (torch.rand((k * k, c), device="cuda", generator=g) - 0.5) * (1.2 / k)
        b = torch.rand((c,), device="cuda", generator=g) - 0.5
        y = [torch.empty((pages, oh, ow, c), device="cuda") for _ in range(2)]
        t = {0: [], 1: []}
        for _rep in range(reps):
            t[0].append(direct(pages, h, w, c, k, s, 2, 2, c, c, iters, 0, x.data_ptr(), wt.data_ptr(), b.data_ptr(), y[0].data_ptr()))
            t[1].append(staged(pages, h, w, c, k, s, 1, 1, 1, iters, aff.ctypes.data, x.data_ptr(), wt.data_ptr(), b.data_ptr(), y[1].data_ptr()))
            assert t[0][-1] >= 0 and t[1][-1] >= 0
        torch.cuda.synchronize()
        mb = 4.0 * (x.numel() + y[0].numel())
        med = [float(np.median(t[r])) for r in (0, 1)]
        spr = [(max(t[r]) - min(t[r])) / med[r] for r in (0, 1)]
        wins = med[1] < med[0] * (1.0 - max(spr))
        print(f"{name:6s} {f'[{pages},{h},{w},{c}]':22s} {k:2d} {s:2d} {lvl:3d} {mb / 1e6:7.1f} {med[0]:10.4f} {spr[0]:7.1%} {mb / med[0] / 1e6:7.0f} {med[1]:10.4f} {spr[1]:7.1%} "
              f"{mb / med[1] / 1e6:7.0f} {med[0] / med[1]:6.2f} {float((y[0] - y[1]).abs().max()):9.2e}  {'yes' if wins else 'no'}")
        del x, y
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--routes", action="store_true", help="the per-block A/B of the fused kernel against the unfused route")
    a = ap.parse_args()
    gd = ROOT / "tests/golden"
    st = W.synth_state_dict(W.load_manifest(gd / f"manifest_{KIND}.json"), 0, kind=KIND)
    st5 = W.synth_state_dict(W.load_manifest(gd / "manifest_ppocrv5_det_mobile.json"), 0, kind="ppocrv5_det_mobile")
    x = torch.rand((a.pages, 3, H, W_), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)) * 2 - 1
    print(f"device {torch.cuda.get_device_name(0)}")
    for precision in ("auto", "fp32"):
        forward_section(KIND, st, x, precision, a.steps, a.warmup)
    forward_section("ppocrv5_det_mobile", st5, x, "auto", a.steps, a.warmup, table=False)
    if a.routes:
        routes_section(st, x, a.reps)
        del x
        torch.cuda.empty_cache()
        dw_section(a.pages, 40, a.reps)


if __name__ == "__main__":
    main()
