#!/usr/bin/env python3
"""Microbenchmark of the multilingual PP-OCRv3 / v4 mobile recogniser (`ppocr_rec_mv1e`; bench.py measures the default v6 path and stays as
it is).  Same workload and planner as tools/mb_rec_mobile.py: 32 synthetic pages = 1440 text lines per step, every line at the reference
width the strict planner gives it, GPU-sized backbone launches with a line table into one token buffer + ONE ragged tail.

  1. strict step of `ppocr_rec_mv1e` (korean file, 3690 classes) and, from the same run, of `ppocrv5_rec_mobile`, alternating: ms per step
     (median, min, max), lines/s, range flag;
  2. the per-kernel table of one profiled step of `ppocr_rec_mv1e`;
  3. the strip kernel against the direct kernel per layer geometry, on the same operands through the two developer entries
     (rd_debug_dw5_strip, rd_debug_lcv3_dw), routes alternating: ms (median, min, max) and GB/s on algorithmic bytes (input + output once);
     the three geometries of this backbone at 64 lines x w2 = 544 and the three of `ppocrv5_rec_mobile` the strip kernel serves
     (480 channels at w4 = 272);
  4. the network under RD_MV1E_DW_STRIP=0 / 1 (two handles, the switch is read when a plan is made), alternating: strict step and the
     sum of the 5x5 depthwise ops; the same for `ppocrv5_rec_mobile` under RD_LCV3_DW_STRIP=0 / 1.

    python tools/mb_rec_mv1e.py [--steps 5] [--warmup 2] [--pages 32] > profiles/mb_rec_mv1e.txt
"""
import argparse
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from rapiddoc_amd import _lib, ocr_host  # noqa: E402
from rapiddoc_amd import weights as W  # noqa: E402
from rapiddoc_amd.engine import RdEngine, rec_line_table  # noqa: E402
from tools.mb_rec_mobile import ev_ms, table  # noqa: E402

KIND, MOBILE = "ppocr_rec_mv1e", "ppocrv5_rec_mobile"


def stats(v):
    return f"median {float(np.median(v)):.3f} (min {min(v):.3f}, max {max(v):.3f})"


class Workload:
    def __init__(self, pages, n_cu):
        from rapiddoc_amd.pages import synth_batch
        _pages, boxes = synth_batch(0, pages)
        ratios = [float((b[2] - b[0]) / max(1.0, (b[3] - b[1]))) for pb in boxes for b in pb]
        self.batches, line_w = ocr_host.rec_batches_lines(ratios, n_cu=n_cu)
        self.line_w = line_w = np.asarray(line_w)
        self.lens = np.array([ocr_host.rec_seq_len(int(w)) for w in line_w])
        first = np.concatenate([[0], np.cumsum(self.lens)[:-1]])
        g = torch.Generator(device="cuda").manual_seed(0)
        self.xs, self.tabs, pos = [], [], 0
        for c, w in self.batches:
            x = torch.zeros((len(c), 3, 48, int(w)), device="cuda")
            for j, lw in enumerate(line_w[pos: pos + len(c)].tolist()):
                x[j, :, :, :lw] = torch.rand((3, 48, lw), device="cuda", generator=g) * 2 - 1
            self.xs.append(x)
            self.tabs.append(torch.from_numpy(rec_line_table(line_w[pos: pos + len(c)], first[pos: pos + len(c)])).cuda())
            pos += len(c)
        self.n_lines, self.n_tok = len(line_w), int(self.lens.sum())

    def bind(self, eng):
        tokens = torch.zeros((self.n_tok, eng.rec_token_dim), device="cuda")
        tables = eng.rec_tail_tables(self.lens, torch.device("cuda", 0))

        def step():
            for x, tab in zip(self.xs, self.tabs):
                eng.rec_backbone_forward_lines(x, tab, tokens)
            eng.rec_tail_forward(tokens, self.lens, tables)
        return step


def engine(kind, state, env=None):
    """A handle whose plans are all made under `env` (the route switches are read per plan): one step is run before the switch is dropped."""
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        eng = RdEngine(kind).load_weights(state)
        step = WL.bind(eng)
        step()
        torch.cuda.synchronize()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return eng, step


def alternate(named_steps, rounds, title):
    t = {n: [] for n, _s in named_steps}
    for _ in range(rounds):
        for n, s in named_steps:
            t[n].append(ev_ms(s, 1))
    print(f"\n{title} ({rounds} rounds, alternating)")
    for n, _s in named_steps:
        print(f"  {n:44s} {stats(t[n])} ms = {WL.n_lines / float(np.median(t[n])) * 1e3:.0f} lines/s")
    return {n: float(np.median(v)) for n, v in t.items()}


def dw5_ops(eng, step):
    eng.set_profiling(True)
    eng.profile_log.clear()
    step()
    eng.set_profiling(False)
    rows = [r for r in eng.profile_log if r["kind"] == "lcv3_dw5x5"]
    return sum(r["ms"] for r in rows), len(rows), sorted({r["cfg"] for r in rows})


def kernel_ab(rounds):
    lib = _lib.load()
    aff = np.array([1, 0, 1, 0], np.float32)
    print(f"\nstrip kernel (dw5_strip_kernel) against the direct kernel (lcv3_dw_kernel<5, SW, 4>), same operands, {rounds} rounds of 20 launches, "
          "alternating; pre_act and post_act on; GB/s on input + output bytes")
    print(f"{'layer geometry':46s} {'direct ms':>34s} {'GB/s':>6s} {'strip ms':>34s} {'GB/s':>6s}  winner")
    for name, N, H, Wd, Cn, sh, sw in (("mv1e blocks 6-10: C 256, 6 rows, s (1,1)", 64, 6, 544, 256, 1, 1),
                                       ("mv1e block 11:    C 256, 6 rows, s (2,1)", 64, 6, 544, 256, 2, 1),
                                       ("mv1e block 12:    C 512, 3 rows, s (1,2)", 64, 3, 544, 512, 1, 2),
                                       ("v5 mobile blocks6.1: C 480, 6 rows, s (1,1)", 64, 6, 272, 480, 1, 1),
                                       ("v5 mobile blocks6.2: C 480, 6 rows, s (2,1)", 64, 6, 272, 480, 2, 1),
                                       ("v5 mobile blocks6.3: C 480, 3 rows, s (1,1)", 64, 3, 272, 480, 1, 1)):
        OH, OW = (H - 1) // sh + 1, (Wd - 1) // sw + 1
        x = torch.rand((N, H, Wd, Cn), device="cuda") * 8 - 4
        w = torch.rand((25, Cn), device="cuda") * 0.4 - 0.2
        b = torch.rand(Cn, device="cuda") - 0.5
        y = torch.zeros((N, OH, OW, Cn), device="cuda")
        gb = 4.0 * (x.numel() + y.numel()) / 1e6

        def direct(it):
            return lib.rd_debug_lcv3_dw(N, H, Wd, Cn, 5, sh, sw, 1, it, aff.ctypes.data, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), None, None, None)

        def strip(it):
            return lib.rd_debug_dw5_strip(N, H, Wd, Cn, sh, sw, 1, 1, Cn, Cn, it, aff.ctypes.data, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), None, None)
        assert direct(2) >= 0 and strip(2) >= 0
        td, ts = [], []
        for _ in range(rounds):
            td.append(direct(20))
            ts.append(strip(20))
        md, ms = float(np.median(td)), float(np.median(ts))
        win = "strip" if max(ts) < min(td) else "direct" if max(td) < min(ts) else "no difference beyond the spread (direct stays)"
        print(f"{name:46s} {stats(td):>34s} {gb / md:6.0f} {stats(ts):>34s} {gb / ms:6.0f}  {win}")
        del x, y


def main():
    global WL
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pages", type=int, default=32)
    a = ap.parse_args()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    WL = Workload(a.pages, n_cu)
    print(f"lines per step {WL.n_lines}, backbone launches {len(WL.batches)} (launch widths {sorted(set(int(w) for _c, w in WL.batches))}), "
          f"distinct line widths {len(set(WL.line_w.tolist()))}, tokens {WL.n_tok}")
    st = W.synth_state_dict(W.load_manifest(ROOT / f"tests/golden/manifest_{KIND}_korean.json"), 0, kind=KIND)
    st_m = W.synth_state_dict(W.load_manifest(ROOT / f"tests/golden/manifest_{MOBILE}.json"), 0)
    eng, step = engine(KIND, st)
    eng_m, step_m = engine(MOBILE, st_m)
    for _ in range(a.warmup):
        step(), step_m()
    torch.cuda.synchronize()
    alternate([(f"{KIND} (default routes)", step), (f"{MOBILE} (default routes)", step_m)], a.steps, "1. strict step")
    print(f"  range flags: {KIND} {int(eng.range_overflow())}, {MOBILE} {int(eng_m.range_overflow())}")

    eng.set_profiling(True)
    eng.profile_log.clear()
    step()
    eng.set_profiling(False)
    table(eng.profile_log, f"2. per-kernel table of one profiled strict step of {KIND}")

    print("\n3.", end="")
    kernel_ab(a.steps)

    e0, s0 = engine(KIND, st, {"RD_MV1E_DW_STRIP": "0"})
    e1, s1 = engine(KIND, st, {"RD_MV1E_DW_STRIP": "1"})
    alternate([(f"{KIND} RD_MV1E_DW_STRIP=0 (direct)", s0), (f"{KIND} RD_MV1E_DW_STRIP=1 (strip)", s1)], a.steps, "4. the network under either route")
    for n, (e, s) in (("0", (e0, s0)), ("1", (e1, s1))):
        ms, n_ops, cfgs = dw5_ops(e, s)
        print(f"  RD_MV1E_DW_STRIP={n}: {n_ops} 5x5 depthwise ops, {ms:.3f} ms in one profiled step; cfgs {cfgs}")
    m0, sm0 = engine(MOBILE, st_m, {"RD_LCV3_DW_STRIP": "0"})
    m1, sm1 = engine(MOBILE, st_m, {"RD_LCV3_DW_STRIP": "1"})
    alternate([(f"{MOBILE} RD_LCV3_DW_STRIP=0 (default)", sm0), (f"{MOBILE} RD_LCV3_DW_STRIP=1 (opt-in)", sm1)], a.steps, "   the opt-in route of the v5 mobile kind")
    for n, (e, s) in (("0", (m0, sm0)), ("1", (m1, sm1))):
        ms, n_ops, cfgs = dw5_ops(e, s)
        print(f"  RD_LCV3_DW_STRIP={n}: {n_ops} 5x5 depthwise ops, {ms:.3f} ms in one profiled step; cfgs {cfgs}")


if __name__ == "__main__":
    main()
