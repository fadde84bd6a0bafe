#!/usr/bin/env python3
"""Microbenchmark of the table path around the UniTable networks (bench.py measures the default page path, which has no table network,
and stays as it is).  One call, medians of alternating rounds after warm-up rounds, as tools/mb_unitable.py:

  1. preprocess per crop, the engine's linear resize (rd_preproc_resize_norm) against the PIL-exact one (rd_preproc_resize_aa_norm:
     two launches, uint8 intermediate), at 120 x 300, 600 x 1000 and 1500 x 2000 -> 448 x 448; device-resident crops, HIP events
     around `iters` calls on a stream of the tool's own; the PIL-exact call's two kernels are also timed apart (horizontal pass =
     the call on the crop minus the call on a crop that is already 448 wide and as high: vertical pass + normalise only)
  2. how far apart the two normalised tensors are on the two 448-target fixture crops (max-abs, mean-abs), and whether the ids the
     networks decode from them differ (class_pil weights of tests/golden/summary_table_path.json)
  3. ms per decode step at B = 1 and B = 8 (S = 784): rd_debug_table_decode with forced tokens at 16 and at 80 steps, (t80 - t16) / 64
  4. ms per table through Mi355RapidTable.predict on the 600 x 1000 crop (host work and the synchronising decode loop included)

    python tools/mb_table_path.py [--steps 7] [--warmup 3] > profiles/mb_table_path.txt
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from rapiddoc_amd import table_unitable as TU  # noqa: E402
from rapiddoc_amd import weights as W  # noqa: E402
from rapiddoc_amd.engine import RdEngine, preproc_resize_aa_norm, preproc_resize_norm  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
MEAN, STD = TU.NORM_MEAN, TU.NORM_STD


def med_spread(v):
    v = np.asarray(v, dtype=np.float64)
    m = float(np.median(v))
    return m, float((v.max() - v.min()) / m) if m > 0 else 0.0


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def preprocess_timing(args):
    side = torch.cuda.Stream()
    out = torch.empty((3, 448, 448), dtype=torch.float32, device="cuda")
    print(f"== preprocess per crop -> 448 x 448 (device-resident BGR crop, 50 calls per round), alternating, {args.warmup} warm-up + {args.steps} timed rounds")
    for h, w in ((120, 300), (600, 1000), (1500, 2000)):
        crop = torch.from_numpy(W.synth_table_crop(1, h, w)).cuda()
        narrow = torch.from_numpy(W.synth_table_crop(1, h, 448)).cuda()
        fns = {"linear": lambda: preproc_resize_norm(crop, (448, 448), mean=MEAN, std=STD, swap_rb=True, out=out),
               "pil": lambda: preproc_resize_aa_norm(crop, (448, 448), MEAN, STD, swap_rb=True, out=out),
               "pil, vertical + normalise only": lambda: preproc_resize_aa_norm(narrow, (448, 448), MEAN, STD, swap_rb=True, out=out)}
        t = {k: [] for k in fns}
        with torch.cuda.stream(side):
            for fn in fns.values():
                fn()
            for r in range(args.warmup + args.steps):
                for k, fn in fns.items():
                    ms = timed(fn, 50)
                    if r >= args.warmup:
                        t[k].append(ms)
        side.synchronize()
        line = f"{h:4d} x {w:4d}  "
        for k in fns:
            m, s = med_spread(t[k])
            line += f" {k} {1e3 * m:7.1f} us (spread {100 * s:4.1f} %)  "
        print(line)


def class_pil():
    exp = json.loads((GOLDEN / "summary_table_path.json").read_text())["class_pil"]
    enc = W.synth_state_dict(W.load_manifest(GOLDEN / "manifest_unitable_encoder.json"), 0)
    dec = W.synth_state_dict(W.load_manifest(GOLDEN / "manifest_unitable_decoder.json"), 0)
    b = dec["generator.bias"].copy()
    b[TU.STAND_IN_IDS.eos] += np.float32(exp["bias_add"])
    dec["generator.bias"] = b
    return TU.Mi355UniTableStructure(enc, dec, TU.STAND_IN_IDS, TU.stand_in_tokens(), max_new_tokens=64, resize="pil"), exp, dec


def difference(cls):
    print("== linear against PIL-exact on the two 448-target fixture crops (normalised tensors; ids decoded by the class_pil networks, 64 tokens at most)")
    for h, w in ((600, 1000), (120, 300)):
        crop = W.synth_table_crop(1, h, w)
        x = {}
        for mode in ("linear", "pil"):
            cls.resize = mode
            x[mode] = cls.preprocess([crop])[0]
        cls.resize = "pil"
        ids = {m: cls.decode_ids(x[m])[0] for m in x}
        d = (x["linear"] - x["pil"]).abs()
        same = next((i for i, (a, b) in enumerate(zip(ids["linear"], ids["pil"])) if a != b), min(len(ids["linear"]), len(ids["pil"])))
        print(f"{h:4d} x {w:4d}   max-abs {float(d.max()):.3f}   mean-abs {float(d.mean()):.4f}   ids: {len(ids['linear'])} (linear) / {len(ids['pil'])} (pil) tokens, "
              f"equal: {ids['linear'] == ids['pil']}, common prefix {same}")


def decode_timing(args, dstate):
    dec = RdEngine("unitable_decoder").load_weights(dstate)
    side = torch.cuda.Stream()
    rng = np.random.default_rng(0)
    print(f"== decode step at S = 784 (forced tokens, (t80 - t16) / 64), {args.warmup} warm-up + {args.steps} timed rounds")
    for B in (1, 8):
        memory = torch.from_numpy(W.synth_memory(3, B, 784)).cuda()
        forced = torch.from_numpy(rng.integers(12, 510, (B, 80)).astype(np.int32)).cuda()
        t = []
        with torch.cuda.stream(side):
            for r in range(args.warmup + args.steps):
                ms = []
                for n in (16, 80):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    dec.table_decode_debug(memory, TU.STAND_IN_IDS, n, forced=forced[:, :n].contiguous())
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3)
                if r >= args.warmup:
                    t.append((ms[1] - ms[0]) / 64)
        side.synchronize()
        m, s = med_spread(t)
        print(f"B {B}  {m:7.4f} ms/step (spread {100 * s:4.1f} %)   {m / B:7.4f} ms/step/table")
    dec.close()


def predict_timing(args, cls, exp):
    model = TU.Mi355RapidTable(cls)
    rgb = np.ascontiguousarray(W.synth_table_crop(int(exp["crop_seed"]), 600, 1000)[:, :, ::-1])
    t = []
    for r in range(args.warmup + args.steps):
        ocr = json.loads(json.dumps(exp["ocr_result"]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.predict(rgb, ocr)
        torch.cuda.synchronize()
        if r >= args.warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    m, s = med_spread(t)
    print(f"== Mi355RapidTable.predict, 600 x 1000 crop, {len(exp['ids'])} tokens (flip, upload, preprocess, encoder, {len(exp['ids']) - 1} decode steps, host): "
          f"{m:7.2f} ms per table (spread {100 * s:4.1f} %, wall clock)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}; tools/mb_table_path.py {' '.join(sys.argv[1:])}")
    preprocess_timing(args)
    cls, exp, dstate = class_pil()
    difference(cls)
    predict_timing(args, cls, exp)
    decode_timing(args, dstate)


if __name__ == "__main__":
    main()
