#!/usr/bin/env python3
"""Microbenchmark of the text-line direction classifier (`ppocr_cls_mobile`; bench.py measures the default page path, which never
classifies, and stays as it is).

  1. the forward at [B, 3, 48, 192] on both routes - RD_CLS_FUSED=0, the chain of separate operators, and RD_CLS_FUSED=1, cls_line_kernel
     (csrc/kernels_mbv3s.hip: the whole network in one launch) - at B = 6 (the reference's cls_batch_num) and B = 1440 (the line count of
     a 32-page bench step).  Two engines on the same input and weights, one planned under each setting, run in turn (alternating) in one
     process: `--warmup` untimed rounds, then `--steps` timed ones of `iters` forwards each between two HIP events (the replayed hipGraph
     of the plan, as the pipeline runs it).  Per route the median ms per forward and the spread (max - min) / median of THAT route;
     `fused wins` = its median lies below the unfused one by more than the larger of the two spreads - the rule that sets
     cls_fused_default (csrc/builder_mobile.cpp).  Then the per-op-kind table of one profiled unfused launch (HIP events around every op, launch
     gaps included: the launch-chain share of the route), and the plans' workspace sizes.
  2. --pipeline: PagePipeline on 32 synthetic pages (1440 lines), use_cls=True against use_cls=False built in the same process, steps
     alternating; median ms per step of either and the added ms per step.

    python tools/mb_cls_mobile.py [--pipeline] [--steps 7] [--warmup 3] > profiles/mb_cls_mobile.txt
"""
import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from rapiddoc_amd import weights as W  # noqa: E402
from rapiddoc_amd.engine import RdEngine  # noqa: E402

KIND = "ppocr_cls_mobile"
GOLDEN = ROOT / "tests" / "golden"


def cls_state():
    return W.synth_state_dict(W.load_manifest(GOLDEN / f"manifest_{KIND}.json"), 0, kind=KIND)


def med_spread(v):
    v = np.asarray(v, dtype=np.float64)
    m = float(np.median(v))
    return m, float((v.max() - v.min()) / m) if m > 0 else 0.0


def engine_on_route(state, fused: str, precision: str, shapes):
    """An engine whose plans for `shapes` are built under RD_CLS_FUSED=`fused` (the switch is read per plan)"""
    old = {k: os.environ.get(k) for k in ("RD_CLS_FUSED", "RD_PRECISION")}
    os.environ["RD_CLS_FUSED"], os.environ["RD_PRECISION"] = fused, precision
    try:
        eng = RdEngine(KIND, guard="off", reuse_outputs=True).load_weights(state)
        for x in shapes:
            for _ in range(3):          # build the plan, let the library capture and replay its graph
                eng.cls_forward(x)
        torch.cuda.synchronize()
        return eng
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def timed(eng, x, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        eng.cls_forward(x)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def forward_ab(args):
    state = cls_state()
    for precision in ("auto", "fp32"):
        xs = {}
        for B in (6, 1440):
            x, _ = W.synth_cls_lines(1, B, 48, 192)
            xs[B] = torch.from_numpy(x).cuda()
        engines = {f: engine_on_route(state, f, precision, list(xs.values())) for f in ("0", "1")}
        print(f"== forward [B, 3, 48, 192], precision {precision}: RD_CLS_FUSED=0 against =1, alternating, {args.warmup} warm-up + {args.steps} timed rounds")
        for B, iters in ((6, 50), (1440, 5)):
            x = xs[B]
            p0, p1 = engines["0"].cls_forward(x).clone(), engines["1"].cls_forward(x).clone()
            diff = float((p0 - p1).abs().max())
            t = {"0": [], "1": []}
            for r in range(args.warmup + args.steps):
                for f in ("0", "1"):
                    ms = timed(engines[f], x, iters)
                    if r >= args.warmup:
                        t[f].append(ms)
            (m0, s0), (m1, s1) = med_spread(t["0"]), med_spread(t["1"])
            wins = m1 < m0 * (1.0 - max(s0, s1))
            print(f"B {B:5d} ({iters} forwards per round)   unfused {m0:8.4f} ms (spread {100 * s0:4.1f} %)   fused {m1:8.4f} ms (spread {100 * s1:4.1f} %)   "
                  f"fused / unfused {m1 / m0:5.2f}   fused wins: {'yes' if wins else 'no'}   max |p_fused - p_unfused| {diff:.2e}")
            print(f"        workspace: unfused {engines['0'].workspace_bytes(B, 48, 192) / 2 ** 20:8.1f} MiB   fused {engines['1'].workspace_bytes(B, 48, 192) / 2 ** 20:8.1f} MiB")
        for B in (6, 1440):
            eng = engines["0"]
            eng.set_profiling(True)
            rounds = []
            for _ in range(args.steps):
                eng.profile_log.clear()
                eng.cls_forward(xs[B])
                rounds.append(list(eng.profile_log))
            eng.set_profiling(False)
            kinds = {}
            for log in rounds:
                per = {}
                for r in log:
                    k = "mbv3s_dw" if r["kind"].startswith("mbv3s_dw") else r["kind"]
                    per.setdefault(k, [0, 0.0])
                    per[k][0] += 1
                    per[k][1] += r["ms"]
                for k, (n, ms) in per.items():
                    kinds.setdefault(k, (n, []))[1].append(ms)
            total = sum(float(np.median(v)) for _n, v in kinds.values())
            print(f"-- unfused route, per op kind, B {B} (profiled launches: HIP events around every op, median of {args.steps}); sum {total:.4f} ms over "
                  f"{sum(n for n, _v in kinds.values())} ops")
            for k, (n, v) in sorted(kinds.items(), key=lambda kv: -np.median(kv[1][1])):
                print(f"   {k:12s} {n:3d} ops   {np.median(v):8.4f} ms   {100 * np.median(v) / total:5.1f} %")
        for e in engines.values():
            e.close()
        print()


def pipeline_ab(args):
    from rapiddoc_amd.pages import synth_batch
    from rapiddoc_amd.pipeline import PagePipeline, boxes_to_quads
    states = {k: W.synth_state_dict(W.load_manifest(GOLDEN / f"manifest_{k}.json"), 0) for k in ("ppocrv6_det", "ppocrv6_rec")}
    pages_np, boxes = synth_batch(0, args.pages)
    pages = torch.from_numpy(pages_np).cuda()
    quads = [boxes_to_quads(b) for b in boxes]
    n_lines = sum(len(q) for q in quads)
    pipes = {"off": PagePipeline(states, n_rec_streams=args.rec_streams),
             "on": PagePipeline({**states, KIND: cls_state()}, n_rec_streams=args.rec_streams, use_cls=True)}
    t = {"off": [], "on": []}
    for r in range(args.warmup + args.steps):
        for name in ("off", "on"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = pipes[name].run_batch(pages, quads_per_page=quads)
            torch.cuda.synchronize()
            if r >= args.warmup:
                t[name].append((time.perf_counter() - t0) * 1e3)
    turned = sum(c[0] for r in res for c in r.cls)
    (m0, s0), (m1, s1) = med_spread(t["off"]), med_spread(t["on"])
    print(f"== PagePipeline, {args.pages} pages, {n_lines} lines, strict rec batching, {args.rec_streams} rec streams, quads given; use_cls=False against "
          f"use_cls=True (cls_thresh 0.9), alternating, {args.warmup} warm-up + {args.steps} timed steps")
    print(f"use_cls=False {m0:8.2f} ms/step (spread {100 * s0:4.1f} %)   use_cls=True {m1:8.2f} ms/step (spread {100 * s1:4.1f} %)   added {m1 - m0:6.2f} ms/step "
          f"({100 * (m1 - m0) / m0:4.1f} %)   lines turned with the stand-in weights: {turned} of {n_lines}   RD_CLS_FUSED={os.environ.get('RD_CLS_FUSED', 'unset')}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pipeline", action="store_true")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--rec-streams", type=int, default=4)
    args = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}; tools/mb_cls_mobile.py {' '.join(sys.argv[1:])}")
    if args.pipeline:
        pipeline_ab(args)
    else:
        forward_ab(args)


if __name__ == "__main__":
    main()
