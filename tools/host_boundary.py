"""Host stages of the batch boundary on the benchmark's own page batch, Python restatement against library call, in one process (no
GPU needed): box ordering + merging, the strict mode's line widths, CTC rows -> strings, next to `quads_to_crop_matrices`, which stays
in numpy.

    python tools/host_boundary.py [--pages 32] [--reps 20] [--out profiles/host_boundary.txt] [--write-fixture]

`synthetic_rows` and the helpers below are also what tests/test_host_native_*.py feed the two paths with; `--write-fixture` records
`bench_inputs(32)` as tests/golden/bench_det_records.npz (rendering the 32 pages takes two seconds, too long for a unit test)."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def bench_inputs(n_pages: int = 32):
    """What bench.py's timed step hands the host after its det stage: the DB post-process records of maps rendered from the line boxes
    of `synth_pages(range(n_pages))` (page settings: box_thresh 0.3, unclip 1.8).  -> (records [P, mo], counts [P])."""
    from rapiddoc_amd import ocr_host
    from rapiddoc_amd.pages import PAGE_H, PAGE_W, synth_pages
    from rapiddoc_amd.pipeline import DET_LIMIT, render_text_maps
    _pages, boxes = synth_pages(range(n_pages))
    bh, bw = -(-(PAGE_H + 100) // 64) * 64, -(-(PAGE_W + 100) // 64) * 64
    det_hw = ocr_host.det_resize_shape(bh, bw, DET_LIMIT, "max")
    maps = render_text_maps(boxes, (PAGE_H, PAGE_W), det_hw, "cpu").numpy()
    return ocr_host.db_postprocess(maps, [(PAGE_H, PAGE_W)] * n_pages, thresh=0.3, box_thresh=0.3, unclip_ratio=1.8, raw=True)


FIXTURE = ROOT / "tests" / "golden" / "bench_det_records.npz"


def fixture_inputs():
    """`bench_inputs(32)` as recorded by --write-fixture."""
    from rapiddoc_amd import ocr_host
    z = np.load(FIXTURE)
    records = np.zeros(z["pts"].shape[:2], ocr_host.TEXT_BOX_DTYPE)
    records["pts"], records["score"] = z["pts"], z["score"]
    return records, z["counts"]


def boxes_python(records, counts):
    """The Python path of PagePipeline.boxes_from_maps_device on raw records."""
    from rapiddoc_amd import ocr_host
    out = []
    for b in range(len(counts)):
        k = int(counts[b])
        boxes = records["pts"][b, :k].reshape(k, 4, 2).astype(np.int32)
        if k == 0:
            out.append(np.zeros((0, 4, 2), np.float32))
            continue
        q = ocr_host.merge_det_boxes(ocr_host.sorted_boxes(boxes.astype(np.float32)))
        out.append(np.asarray(q, dtype=np.float32).reshape(-1, 4, 2))
    return out


def line_ratios(quads_per_page):
    """Aspect ratios of the pooled lines as PagePipeline._rec_forward_sources_once computes them."""
    from rapiddoc_amd.pipeline import quads_to_crop_matrices
    quads = np.concatenate([np.asarray(q, dtype=np.float64).reshape(-1, 4, 2) for q in quads_per_page], axis=0)
    _m, cws, chs, ok = quads_to_crop_matrices(quads)
    keep = np.nonzero(ok)[0]
    cws, chs = cws[keep], chs[keep]
    rot = chs / cws >= 2.0
    return (np.where(rot, chs, cws) / np.where(rot, cws, chs)).tolist(), quads


def synthetic_rows(texts, confs, row_bytes: int = 0) -> np.ndarray:
    """Rows as rd_ctc_collapse writes them: int32 n_text_bytes, float32 confidence, int32 n_kept, int32 0, UTF-8 text."""
    enc = [t.encode("utf-8") for t in texts]
    row_bytes = row_bytes or (16 + max([len(e) for e in enc] + [0]) + 15) // 16 * 16
    rows = np.random.default_rng(1).integers(0, 256, size=(len(enc), row_bytes), dtype=np.uint8)      # stale bytes behind the text
    for b, (e, c) in enumerate(zip(enc, confs)):
        rows[b, :16] = np.frombuffer(np.array([len(e)], "<i4").tobytes() + np.array([c], "<f4").tobytes()
                                     + np.array([len(e.decode("utf-8")), 0], "<i4").tobytes(), np.uint8)
        rows[b, 16:16 + len(e)] = np.frombuffer(e, np.uint8)
    return rows


def _best_ms(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--write-fixture", action="store_true")
    args = ap.parse_args()
    from rapiddoc_amd import ocr_host
    from rapiddoc_amd.pipeline import quads_to_crop_matrices
    records, counts = bench_inputs(args.pages)
    if args.write_fixture:
        k = int(counts.max())
        np.savez_compressed(FIXTURE, pts=records["pts"][:, :k], score=records["score"][:, :k], counts=counts)
    quads_pp = ocr_host.order_merge_boxes_native(records, counts)
    assert all(np.array_equal(a, b) for a, b in zip(quads_pp, boxes_python(records, counts)))
    ratios, quads = line_ratios(quads_pp)
    n = len(ratios)
    rng = np.random.default_rng(0)
    # lines of 20-60 three-byte characters, the default dictionary's range (PagePipeline without a dictionary file)
    texts = ["".join(chr(0x4E00 + int(c)) for c in rng.integers(0, 6000, size=int(rng.integers(20, 61)))) for _ in range(n)]
    rows = synthetic_rows(texts, rng.random(n).astype(np.float32))

    def rows_python():
        return [(t, ocr_host.format_score(s)) for t, s in ocr_host.parse_ctc_rows(rows)]

    r = args.reps
    table = [
        ("order + merge of the boxes", _best_ms(lambda: boxes_python(records, counts), r), _best_ms(lambda: ocr_host.order_merge_boxes_native(records, counts), r)),
        ("reference widths + launches", _best_ms(lambda: ocr_host.rec_batches_lines(ratios, with_ratio=True, native=False), r),
         _best_ms(lambda: ocr_host.rec_batches_lines(ratios, with_ratio=True, native=True), r)),
        ("CTC rows -> (text, score)", _best_ms(rows_python, r), _best_ms(lambda: ocr_host.parse_ctc_rows_native(rows), r)),
    ]
    t_mat = _best_ms(lambda: quads_to_crop_matrices(quads), r)
    lines = [f"host stages of one step: {args.pages} pages, {int(counts.sum())} det boxes, {n} lines; best of {r} runs, ms, numpy {np.__version__}",
             f"{'stage':<32}{'Python':>10}{'native':>10}"]
    lines += [f"{name:<32}{a:>10.3f}{b:>10.3f}" for name, a, b in table]
    lines.append(f"{'sum of the three':<32}{sum(a for _, a, _b in table):>10.3f}{sum(b for _, _a, b in table):>10.3f}")
    lines.append(f"{'quads_to_crop_matrices (numpy)':<32}{t_mat:>10.3f}{'-':>10}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")
    return 0 if sum(b for _, _a, b in table) < t_mat else 1


if __name__ == "__main__":
    sys.exit(main())
