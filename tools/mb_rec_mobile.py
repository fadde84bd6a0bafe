#!/usr/bin/env python3
"""Microbenchmark of the PP-OCRv5 mobile recogniser (`ppocrv5_rec_mobile`; bench.py measures the default v6 path and stays as it is).

  1. the bench's line mix - 32 synthetic pages = 1440 text lines per step, every line at the reference width the strict planner gives it
     (ocr_host.rec_batches_lines) - through the planner's own GPU-sized backbone launches with a line table
     (rd_rec_backbone_forward_lines) into one token buffer + ONE ragged tail: lines/s and ms per step, HIP-event timed after warm-up, the
     spread over the timed steps.  Beside it: the server kind's strict step on the same workload, 483 ms in 203 launches
     (docs/notebook/v5_server_rec.md);
  2. the per-kernel table of one step (rd_set_profiling: per-op HIP events, so launch gaps are inside the op times);
  3. the same table for one uniform launch of 64 lines at 48 x 1088, the shape at which the fused block kernel is judged;
  4. RD_LCV3_FUSED off / on (two handles, the switch is read when a plan is made), alternating: the three blocks the fused kernel takes,
     per block from the per-op events, the backbone launch at 64 x 48 x 1088 and the strict step.  `--ab-only` runs this section alone
     (the run to put under `rocprofv3 --kernel-trace --stats`).

    python tools/mb_rec_mobile.py [--steps 5] [--warmup 2] [--pages 32] [--ab-only] > profiles/mb_rec_mobile.txt
"""
import argparse
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from rapiddoc_amd import ocr_host  # noqa: E402
from rapiddoc_amd import weights as W  # noqa: E402
from rapiddoc_amd.engine import RdEngine, rec_line_table  # noqa: E402

SERVER_STRICT_MS, SERVER_LAUNCHES = 483.0, 203


def ev_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def table(log, title):
    agg = {}
    for r in log:
        t = agg.setdefault((r["kind"], r["cfg"]), [0, 0.0, 0.0, 0.0])
        t[0] += 1; t[1] += r["ms"]; t[2] += r["flops"]; t[3] += r["bytes"]
    tot = sum(t[1] for t in agg.values())
    print(f"\n{title} (sum of op times {tot:.2f} ms)")
    print(f"{'kind':22s} {'cfg':26s} {'ops':>5s} {'ms':>9s} {'share':>6s} {'TFLOP/s':>8s} {'GB/s':>8s}")
    for (kind, cfg), t in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print(f"{kind:22s} {cfg:26s} {t[0]:5d} {t[1]:9.3f} {t[1] / tot:6.1%} {t[2] / max(t[1], 1e-9) / 1e9:8.1f} {t[3] / max(t[1], 1e-9) / 1e6:8.0f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--ab-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    st = W.synth_state_dict(W.load_manifest(ROOT / "tests/golden/manifest_ppocrv5_rec_mobile.json"), 0)
    eng = RdEngine("ppocrv5_rec_mobile").load_weights(st)

    from rapiddoc_amd.pages import synth_batch
    _pages, boxes = synth_batch(0, a.pages)
    ratios = [float((b[2] - b[0]) / max(1.0, (b[3] - b[1]))) for pb in boxes for b in pb]
    batches, line_w = ocr_host.rec_batches_lines(ratios, n_cu=n_cu)
    line_w = np.asarray(line_w)
    lens = np.array([ocr_host.rec_seq_len(int(w)) for w in line_w])            # line_w: in the order of the concatenated launches
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    n_lines, n_tok = len(line_w), int(lens.sum())
    print(f"lines per step {n_lines}, backbone launches {len(batches)} (launch widths {sorted(set(int(w) for _c, w in batches))}), "
          f"distinct line widths {len(set(line_w.tolist()))}, tokens {n_tok}")
    g = torch.Generator(device="cuda").manual_seed(0)
    xs, tabs, pos = [], [], 0
    for c, w in batches:
        x = torch.zeros((len(c), 3, 48, int(w)), device="cuda")
        for j, lw in enumerate(line_w[pos: pos + len(c)].tolist()):
            x[j, :, :, :lw] = torch.rand((3, 48, lw), device="cuda", generator=g) * 2 - 1
        xs.append(x)
        tabs.append(torch.from_numpy(rec_line_table(line_w[pos: pos + len(c)], first[pos: pos + len(c)])).cuda())
        pos += len(c)
    tokens = torch.zeros((n_tok, eng.rec_token_dim), device="cuda")
    tables = eng.rec_tail_tables(lens, dev)

    def step():
        for x, tab in zip(xs, tabs):
            eng.rec_backbone_forward_lines(x, tab, tokens)
        eng.rec_tail_forward(tokens, lens, tables)

    if a.ab_only:
        return fused_ab(eng, st, xs, tabs, tokens, lens, tables, g, a)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    ms = [ev_ms(step, 1) for _ in range(a.steps)]
    med = float(np.median(ms))
    print(f"strict step: median {med:.2f} ms (min {min(ms):.2f}, max {max(ms):.2f} over {a.steps} steps after {a.warmup} warm-up) = "
          f"{n_lines / med * 1e3:.0f} lines/s in {len(batches)} backbone launches; range flag {int(eng.range_overflow())}")
    print(f"  beside it: ppocrv5_rec_server, same workload, strict: {SERVER_STRICT_MS:.0f} ms in {SERVER_LAUNCHES} launches "
          f"(docs/notebook/v5_server_rec.md) = {SERVER_STRICT_MS / med:.1f} x this step")

    eng.set_profiling(True)
    eng.profile_log.clear()
    step()
    table(eng.profile_log, "per-kernel table of one profiled strict step")
    x = torch.rand((64, 3, 48, 1088), device="cuda", generator=g) * 2 - 1
    eng.set_profiling(False)
    eng.rec_backbone_forward(x)
    torch.cuda.synchronize()
    ms_bb = ev_ms(lambda: eng.rec_backbone_forward(x), 5)
    eng.set_profiling(True)
    eng.profile_log.clear()
    eng.rec_backbone_forward(x)
    eng.set_profiling(False)
    table(eng.profile_log, f"backbone stage of one uniform launch, 64 x 48 x 1088: {ms_bb:.3f} ms per launch; per-kernel table")
    for r in eng.profile_log[:8]:
        print(f"  {r['name']:48s} {r['kind']:12s} {r['cfg']:12s} {r['shape']:28s} {r['ms']:.3f} ms")
    fused_ab(eng, st, xs, tabs, tokens, lens, tables, g, a)


def fused_ab(eng_off, st, xs, tabs, tokens, lens, tables, g, a):
    """RD_LCV3_FUSED off (the handle of the sections above) against on (a second handle whose plans are made under the switch)."""
    x = torch.rand((64, 3, 48, 1088), device="cuda", generator=g) * 2 - 1

    def step(eng):
        for xi, tab in zip(xs, tabs):
            eng.rec_backbone_forward_lines(xi, tab, tokens)
        eng.rec_tail_forward(tokens, lens, tables)

    os.environ["RD_LCV3_FUSED"] = "1"
    try:
        eng_on = RdEngine("ppocrv5_rec_mobile").load_weights(st)
        eng_on.rec_backbone_forward(x)
        step(eng_on)                                   # every plan of the on handle is made here
    finally:
        del os.environ["RD_LCV3_FUSED"]
    eng_off.rec_backbone_forward(x)
    step(eng_off)
    torch.cuda.synchronize()
    print("\nRD_LCV3_FUSED off / on, alternating")
    blocks = ("backbone.blocks2.0.", "backbone.blocks3.0.", "backbone.blocks3.1.")
    for name, eng in (("off", eng_off), ("on", eng_on)):
        eng.set_profiling(True)
        eng.profile_log.clear()
        eng.rec_backbone_forward(x)
        eng.set_profiling(False)
        for blk in blocks:
            rows = [r for r in eng.profile_log if r["name"].startswith(blk)]
            print(f"  {name:3s} {blk:22s} " + " + ".join(f"{r['kind']} {r['ms']:.3f}" for r in rows) + f" = {sum(r['ms'] for r in rows):.3f} ms")
    tok_off = eng_off.rec_backbone_forward(x)
    tok_on = eng_on.rec_backbone_forward(x)
    print(f"  tokens on against off: max-abs difference {float((tok_on - tok_off).abs().max()):.3e} at max |tokens| {float(tok_off.abs().max()):.2f}; "
          f"range flag {int(eng_on.range_overflow())}")
    for rnd in range(3):
        t = {}
        for name, eng in (("off", eng_off), ("on", eng_on)):
            t[name] = (ev_ms(lambda: eng.rec_backbone_forward(x), 10), ev_ms(lambda: step(eng), 2))
        print(f"  round {rnd}: backbone 64 x 48 x 1088 off {t['off'][0]:.3f} ms, on {t['on'][0]:.3f} ms; strict step off {t['off'][1]:.2f} ms, "
              f"on {t['on'][1]:.2f} ms")


if __name__ == "__main__":
    main()
