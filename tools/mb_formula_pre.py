#!/usr/bin/env python3
"""Microbenchmark of the formula stage's pre-process: `analyze.recognise_formulas` on 96 formula regions, 3 on each of 32 synthetic
pages, with the decoder capped at 1 token so that the pre-process and the encoder dominate (bench.py's value does not contain the
formula stage).  The margin boxes of the regions are drawn from the device-route box sizes of the fixture list
(tests/golden/make_golden_formula_pre_device.py) that fit a third of a page.

Participants, each a worker PROCESS of its own with its own package and library, run in alternation inside one call: `--warmup` rounds,
then `--steps` timed ones; a round is one recognise_formulas call on the whole batch, wall clock, ending in the device-to-host copy of
the ids.  Reported: median and min .. max per participant, how many device-to-host copies (`Tensor.cpu()` of a device tensor) one round
makes, and a crc32 of the token ids (they must agree).

    python tools/mb_formula_pre.py [--steps 7] [--warmup 3] [--parent DIR] > profiles/mb_formula_pre.txt

`--parent DIR`: a checkout of the parent commit with its library built (DIR/rapiddoc_amd/librapiddoc_mi355.so): one more participant
next to this tree with RD_FORMULA_PREPROC=device, =host and unset.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
PAGES, PER_PAGE, PAGE_H, PAGE_W = 32, 3, 1408, 1280
BOXES = [(60, 400), (37, 291), (100, 1000), (23, 157), (301, 64), (200, 90), (50, 51), (13, 17), (50, 50), (401, 400), (1, 1), (1, 40)]   # (h, w)


def make_batch(seed: int = 0):
    """pages uint8 [32, H, W, 3] (light noise, dark strokes inside every region's box) and per page three formula detections whose
    rectangle is the box grown by a margin of 3 .. 8 pixels"""
    rng = np.random.default_rng(seed)
    pages = rng.integers(225, 256, (PAGES, PAGE_H, PAGE_W, 3)).astype(np.uint8)
    dets, band = [], PAGE_H // PER_PAGE
    for p in range(PAGES):
        page_dets = []
        for k in range(PER_PAGE):
            bh, bw = BOXES[int(rng.integers(0, len(BOXES)))]
            m = [int(v) for v in rng.integers(3, 9, 4)]
            y0 = k * band + 10 + int(rng.integers(0, band - bh - 40))
            x0 = 10 + int(rng.integers(0, PAGE_W - bw - 40))
            box = pages[p, y0: y0 + bh, x0: x0 + bw]
            for _ in range(10):
                yy, xx = int(rng.integers(0, bh)), int(rng.integers(0, bw))
                box[yy: yy + int(rng.integers(1, max(2, bh // 3 + 1))), xx: xx + int(rng.integers(1, max(2, bw // 3 + 1)))] = rng.integers(0, 90, 3)
            box[0, int(rng.integers(0, bw))] = box[bh - 1, int(rng.integers(0, bw))] = 20
            box[int(rng.integers(0, bh)), 0] = box[int(rng.integers(0, bh)), bw - 1] = 20
            r = (x0 - m[0], y0 - m[1], x0 + bw + m[2], y0 + bh + m[3])
            page_dets.append({"category_id": 14, "poly": [r[0], r[1], r[2], r[1], r[2], r[3], r[0], r[3]], "score": 0.9})
        dets.append(page_dets)
    return pages, dets


# ---------------------------------------------------------------------------------------------------------------- a participant
def worker(tree: Path):
    """serves one tree: "run" -> one timed round, "count" -> one round counting the device-to-host copies, "quit\""""
    sys.path.insert(0, str(tree))
    import torch
    from rapiddoc_amd import weights as W
    from rapiddoc_amd.analyze import recognise_formulas
    from rapiddoc_amd.formula_host import FormulaRecognizer
    import rapiddoc_amd
    assert Path(rapiddoc_amd.__file__).resolve().parents[1] == tree.resolve(), rapiddoc_amd.__file__
    rec = FormulaRecognizer(W.synth_state_dict(W.load_manifest(ROOT / "tests" / "golden" / "manifest_ppformulanet_plus_m_m8.json"), 0), max_new_tokens=1)
    pages_np, dets0 = make_batch()
    pages = torch.from_numpy(pages_np).cuda()

    def one_round():
        dets = json.loads(json.dumps(dets0))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = recognise_formulas(pages, dets, rec, batch_size=16)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        assert n == PAGES * PER_PAGE
        return ms, zlib.crc32(json.dumps([[d.get("latex") for d in page] for page in dets]).encode())

    print("READY", flush=True)
    for line in sys.stdin:
        cmd = line.strip()
        if cmd == "run":
            ms, crc = one_round()
            print(f"MS {ms:.4f} {crc}", flush=True)
        elif cmd == "count":
            real, seen = torch.Tensor.cpu, [0]

            def counting(self, *a, **k):
                seen[0] += 1 if self.is_cuda else 0
                return real(self, *a, **k)
            torch.Tensor.cpu = counting
            try:
                one_round()
            finally:
                torch.Tensor.cpu = real
            print(f"COPIES {seen[0]} {' '.join(getattr(rec, 'last_routes', []))}", flush=True)
        elif cmd == "quit":
            break


class Participant:
    def __init__(self, name: str, tree: Path, switch):
        env = {k: v for k, v in os.environ.items() if k != "RD_FORMULA_PREPROC"}
        if switch:
            env["RD_FORMULA_PREPROC"] = switch
        self.name, self.ms, self.crc = name, [], None
        self.proc = subprocess.Popen([sys.executable, str(Path(__file__).resolve()), "--worker", str(tree)], env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                     text=True, bufsize=1)
        self.expect("READY")

    def expect(self, word):
        while True:
            line = self.proc.stdout.readline()
            if not line:
                raise RuntimeError(f"{self.name}: the worker ended (exit status {self.proc.wait()})")
            if line.startswith(word):
                return line.split()[1:]

    def ask(self, cmd, word):
        self.proc.stdin.write(cmd + "\n")
        self.proc.stdin.flush()
        return self.expect(word)

    def close(self):
        try:
            self.proc.stdin.write("quit\n")
            self.proc.stdin.flush()
        except OSError:
            pass
        self.proc.wait(timeout=60)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent", type=Path, default=None)
    ap.add_argument("--worker", type=Path, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker is not None:
        return worker(args.worker)
    parts = []
    try:
        if args.parent is not None:
            parts.append(Participant("parent commit", args.parent, None))
        parts.append(Participant("this tree, RD_FORMULA_PREPROC=device", ROOT, "device"))
        parts.append(Participant("this tree, RD_FORMULA_PREPROC=host", ROOT, "host"))
        parts.append(Participant("this tree, switch unset", ROOT, None))
        print(f"# tools/mb_formula_pre.py {' '.join(sys.argv[1:])}: recognise_formulas on {PAGES * PER_PAGE} regions ({PER_PAGE} on each of {PAGES} pages of "
              f"{PAGE_H} x {PAGE_W}), batch_size 16, max_new_tokens 1; {args.warmup} warm-up + {args.steps} timed rounds, participants alternating")
        for r in range(args.warmup + args.steps):
            row = []
            for p in parts:
                ms, crc = p.ask("run", "MS")
                p.crc = crc if p.crc is None else p.crc
                assert crc == p.crc, (p.name, "the ids changed between rounds")
                row.append(float(ms))
                if r >= args.warmup:
                    p.ms.append(float(ms))
            print(f"round {r:2d}{' (warm-up)' if r < args.warmup else '          '}  " + "  ".join(f"{v:9.2f}" for v in row) + "  ms", flush=True)
        print(f"{'participant':42s} {'median ms':>10s} {'min':>9s} {'max':>9s} {'max - min':>10s}  D2H copies per round   ids crc32")
        for p in parts:
            copies = p.ask("count", "COPIES")
            v = np.asarray(p.ms)
            routes = {k: copies[1:].count(k) for k in sorted(set(copies[1:]))}
            print(f"{p.name:42s} {np.median(v):10.2f} {v.min():9.2f} {v.max():9.2f} {v.max() - v.min():10.2f}  {int(copies[0]):6d}  {p.crc}  routes {routes}")
            print(f"    rounds: {' '.join(f'{x:.2f}' for x in p.ms)}")
        assert len({p.crc for p in parts}) == 1, "the participants decode different ids"
    finally:
        for p in parts:
            p.close()


if __name__ == "__main__":
    main()
