#!/usr/bin/env python3
"""Microbenchmark of the PP-OCRv4 server models (PPHGNet_small behind `ppocrv5_det_server` / `ppocrv5_rec_server`; bench.py measures the
default v6 path and stays as it is).

  1. route comparison: each of the nine 3x3 shapes of the backbone at the map sizes of the detector ([pages, 3, 960, 704]: the stem at
     1/2, the stages at 1/4 .. 1/32) and of the recogniser ([lines, 3, 48, 1088]) on
       wide     conv3x3_wide_h1 (csrc/kernels_conv3x3_wide.hip),
       generic  what conv_split_route gives the layer without the builder's opt-in (the split implicit GEMM: the parent's only route),
       pieces   conv3x3_h1 launched over pieces of <= 96 output channels (Cin <= 512 only),
     same operands, same run, alternating, medians of three (rd_debug_conv3x3_wide, iters timed launches each).  The operands sit where the
     network has them: x and y are channel slots of one [N, H, W, in + 6 mid] concat buffer (the stem layer: dense maps);
  2. the two forwards in the `auto` and `fp32` precision modes: ms per launch (HIP events, median), pages/s resp. lines/s, the plan's
     arena, the per-op-kind table of one profiled launch, and the new kernel's TFLOP/s against the fp16 matrix peak (3 MFMAs per product).

    python tools/mb_v4_server.py [--steps 7] [--warmup 3] [--pages 32] [--lines 64] > profiles/mb_v4_server.txt
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
REC_H, REC_W = 48, 1088
ROUTES = ((0, "wide"), (1, "generic"), (2, "pieces"))
# (layer, Cin, Cout, concat width or 0 = dense, detector map divisor (h, w), recogniser map (h, w) divisors of 48 x 1088)
LAYERS = (
    ("stem.2", 64, 128, 0, (2, 2), (2, 2)),
    ("s1 first/next", 128, 128, 896, (4, 4), (4, 2)),
    ("s2 first", 256, 160, 1216, (8, 8), (4, 4)),
    ("s2 next", 160, 160, 1216, (8, 8), (4, 4)),
    ("s3 first", 512, 192, 1664, (16, 16), (8, 4)),
    ("s3 next", 192, 192, 1664, (16, 16), (8, 4)),
    ("s3 identity", 768, 192, 1920, (16, 16), (8, 4)),
    ("s4 first", 768, 224, 2112, (32, 32), (16, 4)),
    ("s4 next", 224, 224, 2112, (32, 32), (16, 4)),
)


def ev_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def route_section(title, n, full_hw, which, iters):
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    print(f"\n== the 3x3 layers alone, {title}: alternating, medians of 3 x {iters} timed launches")
    print(f"{'layer':14s} {'x view':26s} {'GFLOP':>7s} {'wide ms':>8s} {'TFLOP/s':>8s} {'of peak':>8s} {'generic ms':>11s} {'TFLOP/s':>8s} {'pieces ms':>10s} {'TFLOP/s':>8s} "
          f"{'fastest':>8s} {'max |d|':>9s}")
    for name, cin, cout, ld, ddiv, rdiv in LAYERS:
        dh, dw = ddiv if which == "det" else rdiv
        h, w = full_hw[0] // dh, full_hw[1] // dw
        if ld:
            buf = torch.rand((n, h, w, ld), device="cuda", generator=g) * 2 - 1
            x, ys = buf[..., :cin], [buf[..., cin: cin + cout], buf[..., cin + cout: cin + 2 * cout], buf[..., cin + 2 * cout: cin + 3 * cout]]
        else:
            x = torch.rand((n, h, w, cin), device="cuda", generator=g) * 2 - 1
            ys = [torch.empty((n, h, w, cout), device="cuda") for _ in range(3)]
        wt = ((torch.rand((cout, 9 * cin), device="cuda", generator=g) - 0.5) * 0.05).contiguous()
        b = torch.rand((cout,), device="cuda", generator=g) - 0.5
        t = {r: [] for r, _ in ROUTES}
        tags = {}
        for rep in range(3):
            for r, _ in ROUTES:
                nm = C.create_string_buffer(32)
                ms = lib.rd_debug_conv3x3_wide(r, n, h, w, cin, cout, 1, x.stride(2), ys[r].stride(2), iters, x.data_ptr(), wt.data_ptr(), b.data_ptr(),
                                               ys[r].data_ptr(), nm, 32, None)
                t[r].append(ms)
                tags[r] = nm.value.decode()
        torch.cuda.synchronize()
        fl = 2.0 * n * h * w * 9 * cin * cout
        med = {r: float(np.median(v)) if min(v) >= 0 else float("nan") for r, v in t.items()}
        served = {r: m for r, m in med.items() if m == m}
        best = min(served, key=served.get)
        d = max(float((ys[r] - ys[0]).abs().max()) for r in served)
        cell = lambda r: f"{med[r]:.3f}" if med[r] == med[r] else "-"
        rate = lambda r: f"{fl / med[r] / 1e9:.1f}" if med[r] == med[r] else "-"
        print(f"{name:14s} {f'[{n},{h},{w},{cin}] ld {x.stride(2)}':26s} {fl / 1e9:7.1f} {cell(0):>8s} {rate(0):>8s} {3 * fl / med[0] / 1e9 / FP16_PEAK_TFLOPS:8.1%} "
              f"{cell(1):>11s} {rate(1):>8s} {cell(2):>10s} {rate(2):>8s} {dict(ROUTES)[best]:>8s} {d:9.2e}   (route tags {tags[0]} / {tags[1]} / {tags[2] or '-'})")
        del x, ys
        torch.cuda.empty_cache()


def forward_section(kind, st, x, precision, steps, warmup, unit):
    eng = RdEngine(kind, guard="off").load_weights(st).set_precision(precision)
    det = kind == "ppocrv5_det_server"
    run = (lambda: eng.det_forward(x)) if det else (lambda: eng.rec_forward(x))
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    ms = [ev_ms(run) for _ in range(steps)]
    med = float(np.median(ms))
    arena = eng.workspace_bytes(x.shape[0], x.shape[2], x.shape[3])
    print(f"\n== {kind} ({eng.backbone}) forward {list(x.shape)} precision {precision}: median {med:.2f} ms (min {min(ms):.2f}, max {max(ms):.2f}; {steps} timed "
          f"launches after {warmup} warm-up) = {x.shape[0] / med * 1e3:.1f} {unit}/s; arena {arena / 1e9:.2f} GB; range flag {int(eng.range_overflow())}")
    eng.set_profiling(True)
    eng.profile_log.clear()
    run()
    eng.set_profiling(False)
    agg = {}
    for r in eng.profile_log:
        t = agg.setdefault((r["kind"], r["cfg"]), [0, 0.0, 0.0, 0.0])
        t[0] += 1; t[1] += r["ms"]; t[2] += r["flops"]; t[3] += r["bytes"]
    tot = sum(t[1] for t in agg.values())
    print(f"per-op-kind table of one profiled launch (sum of op times {tot:.2f} ms, {sum(t[2] for t in agg.values()) / 1e12:.2f} TFLOP)")
    print(f"{'kind':18s} {'cfg':18s} {'ops':>5s} {'ms':>9s} {'share':>6s} {'TFLOP/s':>8s} {'GB/s':>8s}")
    for (k, cfg), t in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print(f"{k:18s} {cfg:18s} {t[0]:5d} {t[1]:9.3f} {t[1] / tot:6.1%} {t[2] / max(t[1], 1e-9) / 1e9:8.1f} {t[3] / max(t[1], 1e-9) / 1e6:8.0f}")
    wide = agg.get(("conv3x3", "c3w/h3"))
    if wide:
        print(f"conv3x3_wide_h1: {wide[0]} layers, {wide[2] / 1e12:.2f} TFLOP in {wide[1]:.2f} ms = {wide[2] / wide[1] / 1e9:.1f} TFLOP/s = "
              f"{3 * wide[2] / wide[1] / 1e9 / FP16_PEAK_TFLOPS:.1%} of the fp16 matrix peak (3 MFMAs per product)")
    for r in eng.profile_log:
        if "downsample" in r["name"] or r["name"] == "maxpool3x3s2":
            print(f"  {r['name']:44s} {r['kind']:8s} {r['cfg']:10s} {r['ms']:8.3f} ms")
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--lines", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--skip-forward", action="store_true")
    a = ap.parse_args()
    print(f"device {torch.cuda.get_device_name(0)}")
    route_section(f"detector maps of {a.pages} pages [{H} x {W_}]", a.pages, (H, W_), "det", a.iters)
    route_section(f"recogniser maps of {a.lines} lines [{REC_H} x {REC_W}]", a.lines, (REC_H, REC_W), "rec", a.iters)
    if a.skip_forward:
        return
    gen = torch.Generator(device="cuda").manual_seed(0)
    golden = ROOT / "tests/golden"
    st = W.synth_state_dict(W.load_manifest(golden / "manifest_ppocrv4_det_server.json"), 0, kind="ppocrv4_server")
    x = torch.rand((a.pages, 3, H, W_), device="cuda", generator=gen) * 2 - 1
    for precision in ("auto", "fp32"):
        forward_section("ppocrv5_det_server", st, x, precision, a.steps, a.warmup, "pages")
    del x
    torch.cuda.empty_cache()
    st = W.synth_state_dict(W.load_manifest(golden / "manifest_ppocrv4_rec_server.json"), 0, kind="ppocrv4_server")
    x = torch.rand((a.lines, 3, REC_H, REC_W), device="cuda", generator=gen) * 2 - 1
    for precision in ("auto", "fp32"):
        forward_section("ppocrv5_rec_server", st, x, precision, a.steps, a.warmup, "lines")


if __name__ == "__main__":
    main()
