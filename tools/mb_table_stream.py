"""Micro-benchmark of the UniTable decode through refilled slots (rd_table_decode_stream) against the batch path (rd_table_decode).

  python tools/mb_table_stream.py [--parent-lib PATH] [--runs 5] > profiles/mb_table_stream.txt

1. Step cost: ms per step with every row live (the EOS entry of the generator bias lowered by 1e4, so nothing ends), S = 784, `slots` in
   {1, 8}: the stream step and the batch step at B = slots.  A step's cost is the slope between a 64-step and a 192-step call, so the
   once-per-call work (cross K | V, graph capture) drops out.  With --parent-lib (a library built from the parent commit) the batch step is
   measured on that library too; the libraries alternate, one fresh process per run, `--runs` runs each: median, min, max.
2. Throughput on mixed lengths: 48 tables (default_rng(100 + i).standard_normal((784, 768)) * 3.0), 1024 new tokens, the EOS entry of the
   generator bias raised by --eos-bias (3.0: lengths from 4 to the cap) so that the lengths spread: "stream" at 8 slots against chunks of
   8 through rd_table_decode; the measured time ratio beside the ratio of step launches the schedule predicts (tests/stream_reference.py).
3. The table path: 4 synthetic pages with 8 table regions each through analyze.PageAnalyzer (stub layout, prepared detector and
   recogniser answers for the table crops, the class_pil networks of tools/mb_table_path.py behind Mi355RapidTable with
   batching="stream"), `table_pooled=True` against the per-table route, alternating rounds; the table stage alone beside the whole call.
`--probe`: the lengths several EOS biases give (to choose --eos-bias).  Synthetic weights (tests/golden/manifest_unitable_*.json)."""
import argparse
import copy
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
GOLDEN = ROOT / "tests" / "golden"
S, SLOTS = 784, (1, 8)


def weights(eos_add):
    from rapiddoc_amd import table_unitable as TU, weights as W
    st = dict(W.synth_state_dict(W.load_manifest(GOLDEN / "manifest_unitable_decoder.json"), 0))
    b = st["generator.bias"].copy()
    b[TU.STAND_IN_IDS.eos] += np.float32(eos_add)
    st["generator.bias"] = b
    return st


def memories(n, first=100):
    """standard normal rows times 3.0 (as the formula benchmark's pool): wide enough for the cross-attention to tell the tables apart"""
    return np.stack([np.random.default_rng(first + i).standard_normal((S, 768)) * 3.0 for i in range(n)]).astype(np.float32)


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
    from rapiddoc_amd import _lib, table_unitable as TU
    if lib_path:
        _lib.LIB_PATH = Path(lib_path)
    from rapiddoc_amd.engine import RdEngine
    has_stream = hasattr(__import__("ctypes").CDLL(str(_lib.LIB_PATH)), "rd_table_decode_stream") if lib_path else True
    if lib_path and not has_stream:          # a parent library: bind only what it exports
        for table in (_lib.SYMBOLS, _lib.DEBUG_SYMBOLS):
            for name in [n for n in table if "table_decode_stream" in n]:
                del table[name]
    IDS = TU.STAND_IN_IDS
    eng = RdEngine("unitable_decoder").load_weights(weights(-1e4))
    out = {}
    with torch.cuda.stream(torch.cuda.Stream()):          # (the step is captured into a graph on a stream of the caller's)
        for slots in SLOTS:
            mem = torch.from_numpy(memories(slots)).cuda()
            step = lambda fn: (timed(lambda: fn(192)) - timed(lambda: fn(64))) / 128 * 1e3
            eng.table_decode(mem, IDS, 8)
            row = {"batch_ms": step(lambda T: eng.table_decode(mem, IDS, T))}
            if has_stream:
                eng.table_decode_stream(mem, IDS, 8, slots)
                row["stream_ms"] = step(lambda T: eng.table_decode_stream(mem, IDS, T, slots))
                _ids, _lens, st = eng.table_decode_stream(mem, IDS, 64, slots)
                assert st["steps"] == 64 and st["live_slot_steps"] == 64 * slots, st       # every slot live in every step
            out[str(slots)] = row
    print("WORKER " + json.dumps(out))


def profile_run(slots):
    """for a per-kernel table (`rocprofv3 --kernel-trace --stats -- python tools/mb_table_stream.py --profile-run 8`): 64 steps of the
    stream and 64 of the batch path with every row live; the stream's launches are the td_stream_* kernels"""
    import torch
    from rapiddoc_amd import table_unitable as TU
    from rapiddoc_amd.engine import RdEngine
    eng = RdEngine("unitable_decoder").load_weights(weights(-1e4))
    mem = torch.from_numpy(memories(slots)).cuda()
    with torch.cuda.stream(torch.cuda.Stream()):
        eng.table_decode_stream(mem, TU.STAND_IN_IDS, 64, slots)
        eng.table_decode(mem, TU.STAND_IN_IDS, 64)
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
        print(f"slots {slots}  stream (this tree)   {fmt([r[k]['stream_ms'] for r in cur])}")
        print(f"slots {slots}  batch  (this tree)   {fmt([r[k]['batch_ms'] for r in cur])}")
        if par:
            pv = [r[k]["batch_ms"] for r in par]
            print(f"slots {slots}  batch  (parent lib)  {fmt(pv)}")
            over = statistics.median([r[k]["stream_ms"] for r in cur]) - statistics.median(pv)
            print(f"slots {slots}  stream median - parent median = {over * 1e3:+.1f} us; parent's min-to-max spread {1e3 * (max(pv) - min(pv)):.1f} us")


def probe(biases, N=48, max_new=1024):
    import torch
    from rapiddoc_amd import table_unitable as TU
    from rapiddoc_amd.engine import RdEngine
    mem = torch.from_numpy(memories(N)).cuda()
    for b in biases:
        eng = RdEngine("unitable_decoder").load_weights(weights(b))
        with torch.cuda.stream(torch.cuda.Stream()):
            _ids, lens, st = eng.table_decode_stream(mem, TU.STAND_IN_IDS, max_new, 8)
        print(f"eos bias {b:+.2f}: steps {st['steps']}, lengths {lens.cpu().numpy().tolist()}")
        eng.close()


def throughput(eos_bias):
    import stream_reference as SR
    import torch
    from rapiddoc_amd import table_unitable as TU
    from rapiddoc_amd.engine import RdEngine
    N, max_new, slots = 48, 1024, 8
    IDS = TU.STAND_IN_IDS
    eng = RdEngine("unitable_decoder").load_weights(weights(eos_bias))
    mem = torch.from_numpy(memories(N)).cuda()
    res = {}
    with torch.cuda.stream(torch.cuda.Stream()):
        eng.table_decode_stream(mem[:8], IDS, 8, slots)
        eng.table_decode(mem[:8], IDS, 8)
        t_stream = timed(lambda: res.__setitem__("s", eng.table_decode_stream(mem, IDS, max_new, slots)), reps=3)
        ids, lens, st = res["s"]
        lens = lens.cpu().numpy()
        tokens = int((lens - 1).sum())

        def chunked():
            res["c"] = [eng.table_decode(mem[b: b + 8], IDS, max_new) for b in range(0, N, 8)]
        t_chunk = timed(chunked, reps=3)
    need = [max(n) - 1 for _ids, n in res["c"]]
    launches = sum(min(max_new, (c + 7) // 8 * 8) for c in need)          # the batch loop looks at its state every 8 steps
    same = all(n == lens[b: b + 8].tolist() and all(bool((i[r, :n[r]].cpu() == ids[b + r, :n[r]].cpu()).all()) for r in range(len(n)))
               for b, (i, n) in zip(range(0, N, 8), res["c"]))
    sim, chunk = len(SR.simulate(lens, slots)), SR.chunk_steps(lens, slots)
    print(f"== throughput, N = {N}, S = {S}, max_new = {max_new}, EOS bias {eos_bias:+.2f}; lengths (tokens): {(lens - 1).tolist()}")
    print(f"tokens {tokens}, longest {int(lens.max()) - 1}; the same ids and lengths in both modes: {same}")
    print(f"stream 8 slots : {t_stream * 1e3:8.1f} ms  {N / t_stream:7.1f} tables/s  {tokens / t_stream:8.0f} tokens/s  step launches {st['steps']:5d}  "
          f"live share {tokens / (st['steps'] * slots):.3f}")
    print(f"chunks of 8    : {t_chunk * 1e3:8.1f} ms  {N / t_chunk:7.1f} tables/s  {tokens / t_chunk:8.0f} tokens/s  step launches {launches:5d}  "
          f"live share {tokens / (launches * 8):.3f}   (steps needed per chunk: {need})")
    print(f"time ratio chunk / stream {t_chunk / t_stream:.2f}; launched-step ratio {launches / st['steps']:.2f}; "
          f"the schedule predicts chunk_steps / len(simulate) = {chunk} / {sim} = {chunk / sim:.2f}")


def table_path(rounds, warmup):
    """PageAnalyzer with `table_pooled` on and off on the same pages, alternating"""
    import torch
    from rapiddoc_amd import table_unitable as TU, weights as W
    from rapiddoc_amd.analyze import PageAnalyzer
    from rapiddoc_amd.layout_model import LayoutModel
    from rapiddoc_amd.pages import synth_batch
    from rapiddoc_amd.pipeline import PagePipeline
    exp = json.loads((GOLDEN / "summary_table_path.json").read_text())["class_pil"]
    enc = W.synth_state_dict(W.load_manifest(GOLDEN / "manifest_unitable_encoder.json"), 0)
    cls = TU.Mi355UniTableStructure(enc, weights(float(exp["bias_add"])), TU.STAND_IN_IDS, TU.stand_in_tokens(), max_new_tokens=64, resize="pil",
                                    batching="stream", slots=8)
    model = TU.Mi355RapidTable(cls)
    maps = json.loads((GOLDEN / "layout_category_maps.json").read_text())
    labels = list(maps["label_to_category"]["pp_doclayoutv2"])
    P = 4
    pages_np, _ = synth_batch(0, P)
    H, Wd = pages_np.shape[1:3]
    rects = [(60 + c * (Wd // 2 - 40), 80 + r * (H // 4 - 30), 60 + c * (Wd // 2 - 40) + Wd // 2 - 100, 80 + r * (H // 4 - 30) + H // 4 - 60)
             for r in range(4) for c in range(2)]

    class Session:
        characters = labels

        def __call__(self, x, sf):
            rows = [[labels.index("table"), 0.9, *r, 0] for r in rects] * x.shape[0]
            return [np.asarray(rows, np.float32), np.full(x.shape[0], len(rects), np.int32)]

    def det_raw(canvas, n):
        h, w = int(canvas.shape[1]), int(canvas.shape[2])
        return [np.array([[[10, 10], [w // 2, 10], [w // 2, 40], [10, 40]], [[10, 60], [w - 20, 60], [w - 20, 90], [10, 90]]], np.float32)]

    states = {k: W.synth_state_dict(W.load_manifest(GOLDEN / f"manifest_{k}.json"), 0) for k in ("ppocrv6_det", "ppocrv6_rec")}
    pipe = PagePipeline(states, n_rec_streams=2)
    an = {pooled: PageAnalyzer(LayoutModel(Session(), "pp_doclayoutv3"), pipe, table_model=model, table_use_word_box=False, table_pooled=pooled,
                               table_det_raw_fn=det_raw, table_rec_fn=lambda canvas, q: [("cell", 0.9)] * len(q)) for pooled in (False, True)}
    pages = torch.from_numpy(pages_np).cuda()
    whole = {False: [], True: []}
    stage = {False: [], True: []}
    dets0 = an[False](pages, page_scales=[2.0] * P)
    n_tables = sum(1 for page in dets0 for d in page if d["category_id"] == 5)
    for r in range(warmup + rounds):
        for pooled in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = an[pooled](pages, page_scales=[2.0] * P)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            dets = [[{k: copy.deepcopy(v) for k, v in d.items() if k not in ("html", "formula_boxes", "img_boxes")} for d in page] for page in out]
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            an[pooled].table_ocr(pages, dets, model, [2.0] * P)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if r >= warmup:
                whole[pooled].append((t1 - t0) * 1e3)
                stage[pooled].append((t3 - t2) * 1e3)
    print(f"== table path: {P} pages, {n_tables} table regions, 64 tokens at most, {warmup} warm-up + {rounds} timed rounds, alternating; ms per page batch")
    for pooled in (False, True):
        name = "table_pooled=True " if pooled else "per-table route   "
        print(f"{name} whole PageAnalyzer call {fmt(whole[pooled])}   table stage alone {fmt(stage[pooled])}   "
              f"stream stats of the last call {cls.last_stream_stats[-1] if pooled else '-'}")
    print(f"table stage per-table / pooled {statistics.median(stage[False]) / statistics.median(stage[True]):.2f}; "
          f"whole call {statistics.median(whole[False]) / statistics.median(whole[True]):.2f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--eos-bias", type=float, default=3.0)
    ap.add_argument("--probe", default=None, metavar="B1,B2,...")
    ap.add_argument("--only", default="", help="comma list of step,throughput,path (default: all)")
    ap.add_argument("--profile-run", type=int, default=0, metavar="SLOTS")
    a = ap.parse_args()
    only = [s for s in a.only.split(",") if s] or ["step", "throughput", "path"]
    if a.profile_run:
        profile_run(a.profile_run)
    elif a.worker is not None:
        worker(a.worker or None)
    elif a.probe:
        probe([float(v) for v in a.probe.split(",")])
    else:
        if "step" in only:
            step_cost(a.parent_lib, a.runs)
        if "throughput" in only:
            throughput(a.eos_bias)
        if "path" in only:
            table_path(7, 3)
