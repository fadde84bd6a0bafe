"""Micro-benchmark of the formula decode through refilled slots (rd_formula_decode_stream) against the batch path (rd_formula_decode).

  python tools/mb_formula_stream.py [--parent-lib PATH] [--runs 5] > profiles/mb_formula_stream.txt

1. Step cost: ms per step with every row live (EOS row of the lm head zeroed, so nothing ends), `slots` in {8, 16, 32}: the stream step
   and the batch step at B = slots.  A step's cost is the slope between a 64-step and a 192-step call, so the once-per-call work (cross K | V,
   graph capture) drops out.  With --parent-lib (a library built from the parent commit) the batch step is measured on that library too;
   the libraries alternate, one fresh process per run, `--runs` runs each: median, min, max.
2. Throughput on mixed lengths: 96 formulas (the 33-sequence pool of tests/test_gpu_dec_step.py with the seeds 1000 + S, 2000 + S, 3000 + S;
   S = 144, 300 new tokens, EOS row x 3.0): "stream" at 16 slots against chunks of 16 through rd_formula_decode.
Synthetic weights (tests/golden/manifest_ppformulanet_head_dec_long.json)."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
S, SLOTS = 144, (8, 16, 32)


def weights(eos_scale):
    from test_oracle_golden import formula_long_case
    st, _enc, _g = formula_long_case(ROOT / "tests" / "golden")
    st["head.decoder.lm_head.weight"][2] *= np.float32(eos_scale)
    return st


def pool(seed, n):
    return (np.random.default_rng(seed).standard_normal((33, S, 2048)) * 3.0).astype(np.float32)[:n]


def timed(fn, reps=3):
    import torch
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def worker(lib_path):
    """one process, one library: ms per step of the batch path and (where the library has it) of the stream"""
    import torch
    from rapiddoc_amd import _lib
    if lib_path:
        _lib.LIB_PATH = Path(lib_path)
    from rapiddoc_amd.engine import RdEngine
    has_stream = hasattr(__import__("ctypes").CDLL(str(_lib.LIB_PATH)), "rd_formula_decode_stream") if lib_path else True
    if lib_path and not has_stream:          # a parent library: bind only what it exports
        for table in (_lib.SYMBOLS, _lib.DEBUG_SYMBOLS):
            for name in [n for n in table if "decode_stream" in n]:
                del table[name]
    eng = RdEngine("ppformulanet_head").load_weights(weights(0.0))
    out = {}
    for slots in SLOTS:
        enc = torch.from_numpy(pool(1000 + S, slots)).cuda()
        step = lambda fn: (timed(lambda: fn(192)) - timed(lambda: fn(64))) / 128 * 1e3
        eng.formula_decode(enc, 8)
        row = {"batch_ms": step(lambda T: eng.formula_decode(enc, T))}
        if has_stream:
            eng.formula_decode_stream(enc, 8, slots)
            row["stream_ms"] = step(lambda T: eng.formula_decode_stream(enc, T, slots))
            ids, lens, st = eng.formula_decode_stream(enc, 64, slots)
            assert st["steps"] == 64 and st["live_slot_steps"] == 64 * slots, st       # every slot live in every step
        out[str(slots)] = row
    print("WORKER " + json.dumps(out))


def profile_run(slots):
    """for a per-kernel table (`rocprofv3 --kernel-trace --stats -- python tools/mb_formula_stream.py --profile-run 32`): 64 steps of the
    stream and 64 of the batch path with every row live; the stream's launches are the dec_stream_* kernels"""
    import torch
    from rapiddoc_amd.engine import RdEngine
    eng = RdEngine("ppformulanet_head").load_weights(weights(0.0))
    enc = torch.from_numpy(pool(1000 + S, slots)).cuda()
    eng.formula_decode_stream(enc, 64, slots)
    eng.formula_decode(enc, 64)
    torch.cuda.synchronize()


def run_worker(lib):
    r = subprocess.run([sys.executable, __file__, "--worker", lib or ""], capture_output=True, text=True, timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("WORKER ")]
    if r.returncode != 0 or not line:
        raise SystemExit(f"worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(line[0][7:])


def fmt(vals):
    return f"median {statistics.median(vals):.4f}  min {min(vals):.4f}  max {max(vals):.4f}"


def step_cost(parent_lib, runs):
    print(f"== step cost, every row live, S = {S}: ms per step, {runs} runs per library, alternating")
    cur, par = [], []
    for _ in range(runs):
        cur.append(run_worker(None))
        if parent_lib:
            par.append(run_worker(parent_lib))
    for slots in SLOTS:
        k = str(slots)
        print(f"slots {slots:2d}  stream (this tree)   {fmt([r[k]['stream_ms'] for r in cur])}")
        print(f"slots {slots:2d}  batch  (this tree)   {fmt([r[k]['batch_ms'] for r in cur])}")
        if par:
            pv = [r[k]["batch_ms"] for r in par]
            print(f"slots {slots:2d}  batch  (parent lib)  {fmt(pv)}")
            over = statistics.median([r[k]["stream_ms"] for r in cur]) - statistics.median(pv)
            print(f"slots {slots:2d}  stream median - parent median = {over * 1e3:+.1f} us; parent's min-to-max spread {1e3 * (max(pv) - min(pv)):.1f} us")


def throughput():
    import torch
    from rapiddoc_amd.engine import RdEngine
    N, max_new, slots = 96, 300, 16
    eng = RdEngine("ppformulanet_head").load_weights(weights(3.0))
    enc = torch.from_numpy(np.concatenate([pool(k * 1000 + S, 33) for k in (1, 2, 3)])[:N]).cuda()
    eng.formula_decode_stream(enc[:16], 8, slots)
    eng.formula_decode(enc[:16], 8)
    res = {}
    t_stream = timed(lambda: res.__setitem__("s", eng.formula_decode_stream(enc, max_new, slots)), reps=3)
    ids, lens, st = res["s"]
    lens = lens.cpu().numpy()
    tokens = int((lens - 1).sum())

    def chunked():
        res["c"] = [eng.formula_decode(enc[b: b + 16], max_new) for b in range(0, N, 16)]
    t_chunk = timed(chunked, reps=3)
    cols = [int(c.shape[1]) - 1 for c in res["c"]]
    launches = sum(min(max_new, (c + 7) // 8 * 8) for c in cols)          # the batch loop looks at its state every 8 steps
    same = all(bool((c.cpu() == ids[b: b + 16, : c.shape[1]].cpu()).all()) for b, c in zip(range(0, N, 16), res["c"]))
    print(f"== throughput, N = {N}, S = {S}, max_new = {max_new}, EOS row x 3.0; lengths (tokens): {(lens - 1).tolist()}")
    print(f"tokens {tokens}, longest {int(lens.max()) - 1}; the same ids in both modes: {same}")
    print(f"stream 16 slots : {t_stream * 1e3:8.1f} ms  {N / t_stream:7.1f} formulas/s  {tokens / t_stream:8.0f} tokens/s  steps {st['steps']:4d}  "
          f"live slot-steps {tokens / (st['steps'] * slots):.3f}")
    print(f"chunks of 16    : {t_chunk * 1e3:8.1f} ms  {N / t_chunk:7.1f} formulas/s  {tokens / t_chunk:8.0f} tokens/s  steps {launches:4d}  "
          f"live slot-steps {tokens / (launches * 16):.3f}   (steps needed per chunk: {cols})")
    print(f"time ratio chunk / stream {t_chunk / t_stream:.2f}; step-count ratio {launches / st['steps']:.2f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip-throughput", action="store_true")
    ap.add_argument("--profile-run", type=int, default=0, metavar="SLOTS")
    a = ap.parse_args()
    if a.profile_run:
        profile_run(a.profile_run)
    elif a.worker is not None:
        worker(a.worker or None)
    else:
        step_cost(a.parent_lib, a.runs)
        if not a.skip_throughput:
            throughput()
