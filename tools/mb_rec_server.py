#!/usr/bin/env python3
"""Microbenchmark of the PP-OCRv5 server recogniser (`ppocrv5_rec_server`; bench.py measures the default v6 path and stays as it is).

  1. the bench's line mix - 32 synthetic pages = 1440 text lines per step, every line at the reference width the strict planner gives it
     (ocr_host.rec_batches_lines) - through backbone launches of one width each (ocr_host.rec_batches_equal_width) into one token buffer
     + ONE ragged tail: lines/s and ms per step, HIP-event timed after warm-up, the spread over the timed steps;
  2. the per-kernel table of one step (rd_set_profiling: per-op HIP events, so launch gaps are inside the op times) with TFLOP/s;
  3. the sequence convolution (csrc/kernels_seqconv.hip) alone at the step's token count: fraction of the split-fp16 peak, counted vs
     algorithmic bytes, and - uniform lines only - against the general route it replaces: the k x k implicit-GEMM convolution on a
     materialised [tokens][4096] concat (rd_debug_conv + the torch.cat that builds the concat), same shapes, same run.

    python tools/mb_rec_server.py [--steps 5] [--warmup 2] [--pages 32] > profiles/mb_rec_server.txt
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from rapiddoc_amd import _lib, ocr_host  # noqa: E402
from rapiddoc_amd import weights as W  # noqa: E402
from rapiddoc_amd.engine import RdEngine  # noqa: E402

# MI355X dense fp16 matrix peak (vendor figure, 2.5 PFLOP/s); a split-fp16 product costs 3 MFMAs
FP16_PEAK_TFLOPS = 2500.0


def line_mix(n_pages, n_cu):
    from rapiddoc_amd.pages import synth_batch
    _pages, boxes = synth_batch(0, n_pages)
    ratios = [float((b[2] - b[0]) / max(1.0, (b[3] - b[1]))) for pb in boxes for b in pb]
    batches, line_w = ocr_host.rec_batches_lines(ratios, n_cu=n_cu)
    return ocr_host.rec_batches_equal_width(np.concatenate([c for c, _w in batches]), line_w), np.asarray(line_w)


def ev_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pages", type=int, default=32)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    st = W.synth_state_dict(W.load_manifest(ROOT / "tests/golden/manifest_ppocrv5_rec_server.json"), 0)
    eng = RdEngine("ppocrv5_rec_server").load_weights(st)
    launches, line_w = line_mix(a.pages, n_cu)
    n_lines = int(sum(len(c) for c, _w in launches))
    lens = np.concatenate([np.full(len(c), ocr_host.rec_seq_len(w)) for c, w in launches])
    n_tok = int(lens.sum())
    print(f"lines per step {n_lines}, backbone launches {len(launches)} (widths {sorted(set(int(w) for _c, w in launches))[:4]} .. "
          f"{max(int(w) for _c, w in launches)}), tokens {n_tok}")
    g = torch.Generator(device="cuda").manual_seed(0)
    xs = [torch.rand((len(c), 3, 48, int(w)), device="cuda", generator=g) * 2 - 1 for c, w in launches]
    tokens = torch.zeros((n_tok, eng.rec_token_dim), device="cuda")
    tables = eng.rec_tail_tables(lens, dev)
    offs = np.concatenate([[0], np.cumsum([len(c) * ocr_host.rec_seq_len(w) for c, w in launches])]).astype(np.int64)

    def step():
        for x, lo, hi in zip(xs, offs[:-1], offs[1:]):
            eng.rec_backbone_forward(x, tokens[int(lo): int(hi)])
        eng.rec_tail_forward(tokens, lens, tables)

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    ms = [ev_ms(step, 1) for _ in range(a.steps)]
    med = float(np.median(ms))
    print(f"step: median {med:.2f} ms (min {min(ms):.2f}, max {max(ms):.2f} over {a.steps} steps after {a.warmup} warm-up) = "
          f"{n_lines / med * 1e3:.0f} lines/s; range flag {int(eng.range_overflow())}")

    eng.set_profiling(True)
    eng.profile_log.clear()
    step()
    eng.set_profiling(False)
    agg = {}
    for r in eng.profile_log:
        k = (r["kind"], r["cfg"])
        t = agg.setdefault(k, [0, 0.0, 0.0, 0.0])
        t[0] += 1; t[1] += r["ms"]; t[2] += r["flops"]; t[3] += r["bytes"]
    tot = sum(t[1] for t in agg.values())
    print(f"\nper-kernel table of one profiled step (sum of op times {tot:.2f} ms)")
    print(f"{'kind':22s} {'cfg':26s} {'ops':>5s} {'ms':>9s} {'share':>6s} {'TFLOP/s':>8s} {'GB/s':>8s}")
    for (kind, cfg), t in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print(f"{kind:22s} {cfg:26s} {t[0]:5d} {t[1]:9.3f} {t[1] / tot:6.1%} {t[2] / max(t[1], 1e-9) / 1e9:8.1f} {t[3] / max(t[1], 1e-9) / 1e6:8.0f}")
    sq = [r for r in eng.profile_log if r["kind"] == "seqconv1x3"]
    for r in sq:
        tf = r["flops"] / r["ms"] / 1e9
        print(f"seqconv in the tail: {r['shape']} {r['cfg']}: {r['ms']:.3f} ms, {tf:.1f} TFLOP/s = {3 * tf / FP16_PEAK_TFLOPS:.1%} of the fp16 "
              f"matrix peak counting the 3 MFMAs of a split product")

    # ---- the sequence convolution alone, uniform lines, against the general route
    lib = _lib.load()
    T, B = 40, n_tok // 40
    M, C0, C1, N = B * T, 2048, 2048, 256
    K = 3 * (C0 + C1)
    x0 = torch.rand((M, C0), device="cuda", generator=g) - 0.5
    x1 = torch.rand((M, C1), device="cuda", generator=g) - 0.5
    w = (torch.rand((N, K), device="cuda", generator=g) - 0.5) * 0.02
    b = torch.zeros(N, device="cuda")
    y = torch.empty((M, N), device="cuda")
    it = 10
    ms_seq = lib.rd_debug_seqconv(M, C0, C1, N, T, 3, 1, it, x0.data_ptr(), C0, x1.data_ptr(), C1, w.data_ptr(), b.data_ptr(), None, y.data_ptr(), N, None)
    ms_seq32 = lib.rd_debug_seqconv(M, C0, C1, N, T, 3, 0, 3, x0.data_ptr(), C0, x1.data_ptr(), C1, w.data_ptr(), b.data_ptr(), None, y.data_ptr(), N, None)
    hi = w.half()
    lo = ((w - hi.float()) * 2048.0).half()
    y2 = torch.empty((M, N), device="cuda")
    ms_cat = ev_ms(lambda: torch.cat([x0, x1], dim=1), 5)
    cat = torch.cat([x0, x1], dim=1).contiguous()                 # [B][1][T][4096]: the tensor the general route needs written
    used = C.c_int(0)
    ms_gen = lib.rd_debug_conv(B, 1, T, C0 + C1, N, 1, 3, 1, 0, 1, 0, 1, 3, it, cat.data_ptr(), w.data_ptr(), hi.data_ptr(), lo.data_ptr(), b.data_ptr(),
                               None, y2.data_ptr(), C.byref(used))
    torch.cuda.synchronize()
    flops = 2.0 * M * K * N
    alg = 4.0 * (M * (C0 + C1) + M * N) + 4.0 * N * K            # every operand once
    counted = 4.0 * (3 * M * (C0 + C1) * 4 + M * N) + 4.0 * N * K * ((M + 63) // 64)   # what the kernel requests: 3 taps x 4 wavefronts per row, the weights per 64-row tile
    print(f"\nsequence conv alone, uniform {B} lines x {T} tokens, K = {K}, N = {N} ({flops / 1e9:.0f} GFLOP):")
    print(f"  seqconv split-fp16   {ms_seq:8.3f} ms  {flops / ms_seq / 1e9:7.1f} TFLOP/s = {3 * flops / ms_seq / 1e9 / FP16_PEAK_TFLOPS:.1%} of the fp16 matrix peak (3 MFMAs per product)")
    print(f"  seqconv native fp32  {ms_seq32:8.3f} ms  {flops / ms_seq32 / 1e9:7.1f} TFLOP/s")
    print(f"  general route        {ms_gen:8.3f} ms conv (kernel tag {used.value}) + {ms_cat:.3f} ms concat = {ms_gen + ms_cat:.3f} ms")
    print(f"  bytes: algorithmic {alg / 1e6:.0f} MB, requested by the kernel (L1 / L2 absorb the re-reads) {counted / 1e6:.0f} MB; "
          f"max |seqconv - general| = {float((y - y2).abs().max()):.3e}")


if __name__ == "__main__":
    main()
