#!/usr/bin/env python3
"""Microbenchmark of the checkbox stage (rapiddoc_amd/checkbox.py, csrc/kernels_checkbox.hip) on one GPU: a batch of 32 seeded form pages
of 1684 x 1191 pixels (tests/checkbox_reference.form_page), resident on the device.

Two participants alternate inside one process, `--warmup` rounds, then `--steps` timed ones, wall clock around a synchronised call:
  detect_pages   Mi355Checkbox.detect_pages(pages): every kernel, the two device-to-host copies, the host finish
  pages.cpu()    the copy of the page batch to the host - the floor of the seam the stage replaces (one `pages[p].cpu()` per page before
                 any OpenCV work could start)
Then the threshold kernel alone (rd_debug_time_checkbox_mask: the one pass over the 3 B / pixel pages, 1 bit / pixel out): ms per launch
and bytes moved over that time.  Reported: median and min .. max, the bytes `detect_pages` copied to the host, boxes found, and how a
round splits into the kernels alone and the host finish.

    python tools/mb_checkbox.py [--steps 9] [--warmup 3] [--pages 32] > profiles/mb_checkbox.txt
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
H, W = 1684, 1191


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pages", type=int, default=32)
    args = ap.parse_args()
    import torch

    import checkbox_reference as R
    from rapiddoc_amd import _lib
    from rapiddoc_amd.checkbox import Mi355Checkbox

    distinct = [R.form_page(100 + s, H, W) for s in range(4)]
    pages = torch.from_numpy(np.stack([distinct[p % 4] for p in range(args.pages)])).cuda()
    box = Mi355Checkbox(0)
    found = box.detect_pages(pages)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    parts = {"detect_pages": lambda: box.detect_pages(pages), "pages.cpu()": lambda: pages.cpu()}
    times = {k: [] for k in parts}
    for r in range(args.warmup + args.steps):
        for name, fn in parts.items():
            ms = timed(fn)
            if r >= args.warmup:
                times[name].append(ms)
    print(f"checkbox stage, {args.pages} pages of {H} x {W} ({pages.numel() / 1e6:.1f} MB on the device), {args.steps} alternating rounds after {args.warmup}")
    for name, ts in times.items():
        print(f"  {name:14s} median {statistics.median(ts):8.3f} ms   ({min(ts):.3f} .. {max(ts):.3f})")
    print(f"  detect_pages copied {box.last_d2h_bytes} bytes to the host ({100.0 * box.last_d2h_bytes / pages.numel():.4f} % of the page bytes), "
          f"{sum(len(f) for f in found)} boxes, {sum(r['label'] == 'Ticked' for f in found for r in f)} ticked, "
          f"{sum(len(r) for r in box.last_records)} candidates")
    # where a round goes: the kernels alone (enqueue + synchronise, nothing copied), and the host finish of the last round's records
    from rapiddoc_amd import checkbox as CB
    max_runs = CB.default_max_runs(H, W)
    bufs = CB.run_device(pages, False, max_runs, box.max_cand)
    ks = [timed(lambda: CB.run_device(pages, False, max_runs, box.max_cand, *bufs)) for _ in range(args.warmup + args.steps)][args.warmup:]
    records = box.last_records

    def finish_all():
        for r in records:
            CB.finish(r, H, W)

    fs = [timed(finish_all) for _ in range(args.warmup + args.steps)][args.warmup:]
    print(f"  of which kernels median {statistics.median(ks):8.3f} ms   ({min(ks):.3f} .. {max(ks):.3f}), "
          f"host finish median {statistics.median(fs):8.3f} ms   ({min(fs):.3f} .. {max(fs):.3f})")
    lib = _lib.load()
    WW = (W + 63) // 64
    bin_words = torch.empty(args.pages * H * WW, dtype=torch.int64, device="cuda")
    ms = [lib.rd_debug_time_checkbox_mask(args.pages, H, W, 20, pages.data_ptr(), bin_words.data_ptr()) for _ in range(args.warmup + args.steps)][args.warmup:]
    moved = pages.numel() + bin_words.numel() * 8
    med = statistics.median(ms)
    print(f"  threshold kernel alone: median {med:.4f} ms per launch ({min(ms):.4f} .. {max(ms):.4f}), {moved / 1e6:.1f} MB read + written "
          f"-> {moved / med / 1e6:.0f} GB/s")


if __name__ == "__main__":
    main()
