#!/usr/bin/env python3
"""Microbenchmark of the PP-OCRv5 server detector (`ppocrv5_det_server`; bench.py measures the default v6 path and stays as it is).

  1. the forward at [pages, 3, 960, 704] (the size the page pipeline runs, 32 pages) in the `auto` and `fp32` precision modes: ms per
     launch (HIP events, after warm-up, median of the timed launches), the plan's arena size, and the per-op-kind table of one profiled
     launch (rd_set_profiling: per-op HIP events, so launch gaps are inside the op times) with TFLOP/s, the 9x9 layers on their own line;
  2. the four inp_conv (256 -> 64) and four pan_lat_conv (64 -> 64) layers alone at those shapes (1/4 .. 1/32 of the page) on the direct
     9x9 kernel (csrc/kernels_conv9x9_h1.hip) and on the generic k x k split implicit GEMM it displaces, same operands, same run
     (rd_debug_conv, iters > 0), alternating;
  3. the fused local tail (csrc/kernels_det_local.hip) alone at the batch: time on both routes, and the bytes it moves against the
     unfused form's full-resolution 65- and 64-channel tensors.

    python tools/mb_det_server.py [--steps 7] [--warmup 3] [--pages 32] > profiles/mb_det_server.txt
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from rapiddoc_amd import _lib  # noqa: E402
from rapiddoc_amd import weights as W  # noqa: E402
from rapiddoc_amd.engine import RdEngine  # noqa: E402

FP16_PEAK_TFLOPS = 2500.0   # MI355X dense fp16 matrix peak (vendor figure); a split-fp16 product costs 3 MFMAs
H, W_ = 960, 704


def ev_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def forward_section(st, x, precision, steps, warmup):
    eng = RdEngine("ppocrv5_det_server", guard="off").load_weights(st).set_precision(precision)
    out = torch.empty((x.shape[0], 1, H, W_), device="cuda")
    for _ in range(warmup):
        eng.det_forward(x, out=out)
    torch.cuda.synchronize()
    ms = [ev_ms(lambda: eng.det_forward(x, out=out)) for _ in range(steps)]
    med = float(np.median(ms))
    arena = eng.workspace_bytes(x.shape[0], H, W_)
    print(f"\n== forward [{x.shape[0]}, 3, {H}, {W_}] precision {precision}: median {med:.2f} ms (min {min(ms):.2f}, max {max(ms):.2f}; {steps} timed "
          f"launches after {warmup} warm-up) = {x.shape[0] / med * 1e3:.1f} pages/s; arena {arena / 1e9:.2f} GB; range flag {int(eng.range_overflow())}; "
          f"plan stats {eng.plan_stats()}")
    eng.set_profiling(True)
    eng.profile_log.clear()
    eng.det_forward(x, out=out)
    eng.set_profiling(False)
    agg = {}
    for r in eng.profile_log:
        kind = r["kind"]
        if kind == "conv9x9":
            kind = "conv9x9 " + ("inp_conv" if "inp_conv" in r["name"] else "pan_lat_conv")
        t = agg.setdefault((kind, r["cfg"]), [0, 0.0, 0.0, 0.0])
        t[0] += 1; t[1] += r["ms"]; t[2] += r["flops"]; t[3] += r["bytes"]
    tot = sum(t[1] for t in agg.values())
    print(f"per-op-kind table of one profiled launch (sum of op times {tot:.2f} ms, {sum(t[2] for t in agg.values()) / 1e12:.2f} TFLOP)")
    print(f"{'kind':26s} {'cfg':22s} {'ops':>5s} {'ms':>9s} {'share':>6s} {'TFLOP/s':>8s} {'GB/s':>8s}")
    for (kind, cfg), t in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print(f"{kind:26s} {cfg:22s} {t[0]:5d} {t[1]:9.3f} {t[1] / tot:6.1%} {t[2] / max(t[1], 1e-9) / 1e9:8.1f} {t[3] / max(t[1], 1e-9) / 1e6:8.0f}")
    for r in eng.profile_log:
        if r["kind"] == "conv9x9":
            print(f"  9x9 {r['name']:28s} {r['shape']:26s} {r['cfg']:12s} {r['ms']:8.3f} ms {r['flops'] / r['ms'] / 1e9:7.1f} TFLOP/s")
    eng.close()


def conv_section(pages, iters):
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    print(f"\n== the 9x9 layers alone, {pages} pages: direct kernel (conv9x9_h1) vs the generic k x k split implicit GEMM, alternating, {iters} timed launches each")
    print(f"{'layer':16s} {'shape':24s} {'GFLOP':>7s} {'direct ms':>10s} {'TFLOP/s':>8s} {'of peak':>8s} {'generic ms':>11s} {'TFLOP/s':>8s} {'ratio':>6s} {'max |d|':>9s}")
    for name, cin in (("inp_conv", 256), ("pan_lat_conv", 64)):
        for lvl, d in enumerate((4, 8, 16, 32)):
            h, w = H // d, W_ // d
            x = torch.rand((pages, h, w, cin), device="cuda", generator=g) * 2 - 1
            wt = (torch.rand((64, 81 * cin), device="cuda", generator=g) - 0.5) * 0.05
            hi = wt.half()
            lo = ((wt - hi.float()) * 2048.0).half()
            y = [torch.empty((pages, h, w, 64), device="cuda") for _ in range(2)]
            t = {4: [], 0: []}
            tags = {}
            for rep in range(3):
                for route in (4, 0):
                    used = C.c_int(route)
                    ms = lib.rd_debug_conv(pages, h, w, cin, 64, 9, 9, 1, 4, 4, 4, 4, 0, iters, x.data_ptr(), wt.data_ptr(), hi.data_ptr(), lo.data_ptr(), None,
                                           None, y[0 if route == 4 else 1].data_ptr(), C.byref(used))
                    t[route].append(ms)
                    tags[route] = used.value
            torch.cuda.synchronize()
            fl = 2.0 * pages * h * w * 81 * cin * 64
            a, b = float(np.median(t[4])), float(np.median(t[0]))
            print(f"{name + '.' + str(lvl):16s} {f'[{pages},{h},{w},{cin}]':24s} {fl / 1e9:7.1f} {a:10.3f} {fl / a / 1e9:8.1f} {3 * fl / a / 1e9 / FP16_PEAK_TFLOPS:8.1%} "
                  f"{b:11.3f} {fl / b / 1e9:8.1f} {b / a:6.2f} {float((y[0] - y[1]).abs().max()):9.2e}   (route tags {tags[4]} / {tags[0]})")


def tail_section(pages, iters):
    lib = _lib.load()
    fn = lib.rd_debug_det_local
    g = torch.Generator(device="cuda").manual_seed(1)
    f = torch.rand((pages, H // 2, W_ // 2, 64), device="cuda", generator=g)
    shrink = torch.rand((pages, H, W_), device="cuda", generator=g)
    w3 = (torch.rand((64, 65, 3, 3), device="cuda", generator=g) - 0.5) * 0.2
    b3 = torch.rand((64,), device="cuda", generator=g) - 0.5
    w1 = (torch.rand((64,), device="cuda", generator=g) - 0.5) * 0.1
    y = torch.empty((pages, H, W_), device="cuda")
    px = pages * H * W_
    moved = 4.0 * (f.numel() + 2 * px)
    unfused = 4.0 * px * (65 * 2 + 64 * 2)              # the concat and the hidden tensor, each written once and read once
    fl_eff = 2.0 * px * (272 * 64 + 64)                 # what the kernel computes (2x2 per parity + the nine shrink taps)
    fl_ref = 2.0 * px * (65 * 9 * 64 + 64)              # the layers as the reference states them
    print(f"\n== fused local tail alone, {pages} pages [{H} x {W_}]: reads f + shrink, writes maps = {moved / 1e6:.0f} MB ({moved / pages / 1e6:.1f} MB per page); "
          f"the unfused form's two full-resolution tensors alone are {unfused / 1e9:.2f} GB ({unfused / pages / 1e6:.0f} MB per page)")
    for split in (1, 0):
        ms = [fn(pages, H, W_, split, iters, f.data_ptr(), shrink.data_ptr(), w3.data_ptr(), b3.data_ptr(), w1.data_ptr(), 0.1, y.data_ptr(), None) for _ in range(3)]
        m = float(np.median(ms))
        print(f"  {'split-fp16' if split else 'native fp32'}: {m:8.3f} ms  computed {fl_eff / m / 1e9:7.1f} TFLOP/s (as stated by the reference {fl_ref / m / 1e9:7.1f}), "
              f"{moved / m / 1e6:7.0f} GB/s of algorithmic traffic" + (f", {3 * fl_eff / m / 1e9 / FP16_PEAK_TFLOPS:.1%} of the fp16 matrix peak (3 MFMAs per product)" if split else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    st = W.synth_state_dict(W.load_manifest(ROOT / "tests/golden/manifest_ppocrv5_det_server.json"), 0)
    x = torch.rand((a.pages, 3, H, W_), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)) * 2 - 1
    print(f"device {torch.cuda.get_device_name(0)}")
    for precision in ("auto", "fp32"):
        forward_section(st, x, precision, a.steps, a.warmup)
    del x
    torch.cuda.empty_cache()
    conv_section(a.pages, a.iters)
    tail_section(a.pages, a.iters)


if __name__ == "__main__":
    main()
