"""The recogniser stage's plan: everything PagePipeline decides about a call's text lines before the first kernel, as host arithmetic.

`plan_rec` pools the lines of all sources, drops the quads no crop exists for, picks the batcher of the mode, fills the `LINE_DTYPE`
descriptors, lays out the crop scratch, lists the warp launches and - for the two-stage recogniser - places every line's tokens in
the token buffer.  It touches no GPU: numpy, `ocr_host` (whose native batcher lives in the host part of the library) and two helpers
of `engine`.  `PagePipeline._enqueue_rec` / `_decode_rec` read the resulting `RecPlan`."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import ocr_host
from .engine import pad_tail_lengths, rec_line_table

CLS_IMG_H, CLS_IMG_W = 48, 192       # the text-line classifier's input (PaddleOCR cls_image_shape "3, 48, 192")

# rd_line_crop_desc (include/rapiddoc_mi355.h): the reference-shaped two-stage crop (cubic warp to the integer-sized uint8
# crop, rotation of tall crops, linear resize to height 48), homography in float64 like cv2's
LINE_DTYPE = np.dtype([("page", "<i4"), ("out_w", "<i4"), ("crop_w", "<i4"), ("crop_h", "<i4"), ("rot90", "<i4"),
                       ("scratch_off", "<i4"), ("m", "<f8", (9,))])
assert LINE_DTYPE.itemsize == 96
# rd_line_source_desc: a line that names its own source image (rd_line_warp_sources)
LINE_SOURCE_DTYPE = np.dtype([("src", "<u8"), ("pitch", "<i8"), ("W", "<i4"), ("H", "<i4"), ("crop_w", "<i4"), ("crop_h", "<i4"),
                              ("scratch_off", "<i4"), ("reserved", "<i4"), ("m", "<f8", (9,))])
assert LINE_SOURCE_DTYPE.itemsize == 112


def quad_to_crop_matrix(quad: np.ndarray) -> Tuple[np.ndarray, float, float]:
    """Inverse of the reference's perspective rectification (utils/ocr_utils.py:494-536): returns the 3x3 matrix
    that maps rectified-crop pixel (x, y, 1) to page coordinates plus the crop size.  `quad`: 4x2 points
    (tl, tr, br, bl)."""
    q = np.asarray(quad, dtype=np.float64).reshape(4, 2)
    cw = max(np.linalg.norm(q[0] - q[1]), np.linalg.norm(q[2] - q[3]))
    ch = max(np.linalg.norm(q[0] - q[3]), np.linalg.norm(q[1] - q[2]))
    cw, ch = float(int(cw)), float(int(ch))  # ocr_utils.py:508-519 casts to int
    cw, ch = max(cw, 1.0), max(ch, 1.0)
    src = np.array([[0, 0], [cw, 0], [cw, ch], [0, ch]], dtype=np.float64)
    # solve the homography src -> q (8 unknowns)
    A, b = [], []
    for (x, y), (u, v) in zip(src, q):
        A.append([x, y, 1, 0, 0, 0, -u * x, -u * y]); b.append(u)
        A.append([0, 0, 0, x, y, 1, -v * x, -v * y]); b.append(v)
    h = np.linalg.solve(np.asarray(A), np.asarray(b))
    return np.append(h, 1.0).astype(np.float32), cw, ch


def quads_to_crop_matrices(quads: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Vectorised `quad_to_crop_matrix` for [n,4,2] quads -> ([n,9] float64, crop widths, crop heights, ok mask).
    Crop size as `get_rotate_crop_image` computes it (utils/ocr_utils.py:508-519): `int(max(np.linalg.norm(p0 - p1),
    np.linalg.norm(p2 - p3)))` on FLOAT32 points - float32 subtraction, float32 norm (sqrt of the float32 sum of the two
    float32 squares), truncation - so an edge whose length is within float32 rounding of an integer gets the crop size
    the reference gives it.  `ok` is False for quads no homography exists for (zero-size crop, collinear corners): the
    reference's cv2.warpPerspective raises on them; callers here skip them."""
    q32 = np.asarray(quads, dtype=np.float32).reshape(-1, 4, 2)
    q = q32.astype(np.float64)
    n = len(q)

    def norm32(a, b):
        d = a - b                                               # float32
        return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])   # float32 throughout, like np.linalg.norm on a float32 vector
    cw = np.maximum(norm32(q32[:, 0], q32[:, 1]), norm32(q32[:, 2], q32[:, 3])).astype(np.float64)
    ch = np.maximum(norm32(q32[:, 0], q32[:, 3]), norm32(q32[:, 1], q32[:, 2])).astype(np.float64)
    cw, ch = np.floor(cw), np.floor(ch)
    ok = (cw >= 1.0) & (ch >= 1.0) & np.isfinite(cw) & np.isfinite(ch)
    cw, ch = np.where(ok, cw, 1.0), np.where(ok, ch, 1.0)
    z = np.zeros(n)
    src = np.stack([np.stack([z, z], 1), np.stack([cw, z], 1), np.stack([cw, ch], 1), np.stack([z, ch], 1)], axis=1)  # [n,4,2]
    A = np.zeros((n, 8, 8))
    b = np.zeros((n, 8))
    x, y, u, v = src[..., 0], src[..., 1], q[..., 0], q[..., 1]
    A[:, 0::2, 0], A[:, 0::2, 1], A[:, 0::2, 2] = x, y, 1.0
    A[:, 0::2, 6], A[:, 0::2, 7] = -u * x, -u * y
    A[:, 1::2, 3], A[:, 1::2, 4], A[:, 1::2, 5] = x, y, 1.0
    A[:, 1::2, 6], A[:, 1::2, 7] = -v * x, -v * y
    b[:, 0::2], b[:, 1::2] = u, v
    # a singular system (three collinear corners, repeated points) must not abort the whole page batch
    # scale-aware test: a homography of the crop rectangle exists iff no three corners of the quad are collinear - every corner
    # triangle must have an area that is not vanishing next to the crop's (an absolute bound on det(A), whose entries reach
    # coordinate^2, lets near-collinear quads through)
    with np.errstate(all="ignore"):
        for i, j, k in ((0, 1, 2), (1, 2, 3), (2, 3, 0), (3, 0, 1)):
            cross = (q[:, j, 0] - q[:, i, 0]) * (q[:, k, 1] - q[:, i, 1]) - (q[:, j, 1] - q[:, i, 1]) * (q[:, k, 0] - q[:, i, 0])
            ok &= np.isfinite(cross) & (np.abs(cross) > 1e-6 * cw * ch)
    A[~ok] = np.eye(8)
    h = np.linalg.solve(A, b[..., None])[..., 0]
    return np.concatenate([h, np.ones((n, 1))], axis=1), cw, ch, ok


@dataclass
class RecPlan:
    """One recogniser call, planned.  "Pooled" indexes the flat line list in pooled order (all quads, `n_all`); "kept" indexes the
    `n` lines a crop exists for, still in pooled order (`keep[i]` is kept line i's pooled index); "launch order" is the order the
    lines sit in the descriptors and launch tensors (`order_all[j]` is the kept line at position j).  A call without a kept line
    has n == 0 and only the pooling fields."""
    # the pooling: images per source; per pooled line its source and image; the key sort (None: no keys); the kept lines
    n_img: List[int]
    src_of: np.ndarray
    page_of: np.ndarray
    perm: Optional[np.ndarray]
    keep: np.ndarray
    n_all: int
    lines_mode: bool = False            # strict two-stage: reference widths per LINE inside GPU-sized launches
    two_stage: bool = False
    lines_in_launch: bool = False       # lines mode with the line table (the kind computes per-line widths inside a launch)
    # per kept line: crop size before the rotation of tall crops, the rotation, the size and aspect ratio of what the recogniser sees
    crop_w: Optional[np.ndarray] = None
    crop_h: Optional[np.ndarray] = None
    rot90: Optional[np.ndarray] = None
    eff_w: Optional[np.ndarray] = None
    eff_h: Optional[np.ndarray] = None
    ratios: Optional[List[float]] = None
    # launch order: kept line, pooled line, padded width per line (the launch's own outside lines mode), the chunk ratio (lines mode)
    order_all: Optional[np.ndarray] = None
    line_ids: Optional[np.ndarray] = None
    line_w: Optional[np.ndarray] = None
    line_ratio: Optional[np.ndarray] = None
    batches: Optional[List[Tuple[np.ndarray, int]]] = None      # per launch: (kept lines, width of the launch tensor)
    starts: Optional[np.ndarray] = None                         # first position of every launch, and n
    descs: Optional[np.ndarray] = None                          # LINE_DTYPE [n]
    descs_cls: Optional[np.ndarray] = None                      # the classifier's resize (use_cls), else None
    descs_warp: Optional[np.ndarray] = None                     # several sources: every launch's descriptors grouped by source, else None
    warp_jobs: Optional[List[List[Tuple[int, int, int, int]]]] = None   # per launch: (source, first desc, count, max crop pixels)
    # lines that name their own source (PagePipeline.rec_forward_crops; no warp jobs then): LINE_SOURCE_DTYPE of the lines to warp
    # in launch order, per launch (first desc, count), the size of the scratch buffer they are written into
    src_descs: Optional[np.ndarray] = None
    src_jobs: Optional[List[Tuple[int, int]]] = None
    src_scratch_bytes: int = 0
    swap_rb: int = 1                    # the recogniser's resize exchanges channels 0 and 2 (the crops are RGB; rapidocr works on BGR)
    batch_base: Optional[np.ndarray] = None                     # first scratch byte of every launch, and the total
    # two-stage: tokens per line, the groups of S launches that share a tail call, their real and padded (engine.pad_tail_lengths)
    # line lengths, every group's first token, every line's first token, every launch's, the line table of the backbone
    seq_line: Optional[np.ndarray] = None
    groups: Optional[List[List[int]]] = None
    group_lens: Optional[List[np.ndarray]] = None
    group_pad: Optional[List[Tuple[np.ndarray, int]]] = None
    group_base: Optional[np.ndarray] = None
    first_tok: Optional[np.ndarray] = None
    tok_lo: Optional[List[int]] = None
    linetab: Optional[np.ndarray] = None

    @property
    def n(self) -> int:
        return len(self.keep)

    @property
    def scratch_bytes(self) -> int:
        return int(self.batch_base[-1])


def _no_lines(sync, **pooling) -> RecPlan:
    if sync is not None:
        sync(np.zeros(0, np.int64), np.zeros(0))       # a rank without a line still takes part: every rank makes the same calls
    return RecPlan(**pooling)


def plan_rec(sources: Sequence[Tuple[int, Sequence[np.ndarray]]], image_keys: Optional[Sequence[Sequence[int]]] = None, *,
             strict: bool, two_stage: bool, lines_in_launch: bool, chunking: str, rec_batch_num: int, rec_width_multiple: int,
             n_cu: int, n_streams: int, use_cls: bool = False, host_native: bool = True, want_words: bool = False,
             width_sync: Optional[Callable] = None) -> RecPlan:
    """`sources`: per source (number of images, text-line quads per image).  `image_keys[source][image]`: the pooled list is ordered
    by this key first (stable).  `width_sync` (strict two-stage only): (keys int64 [n], ratios float64 [n]) -> (reference width,
    max_wh_ratio) per line, decided over the lines of every rank; called exactly ONCE per plan, with empty arrays when there is no
    kept line."""
    z32 = np.zeros(0, np.int32)
    n_img = [int(k) for k, _q in sources]
    # flat line list in source-major, image-major order (the reference's pooled order: pages, then a page's spans)
    src_of, page_of, quad_list = [], [], []
    for si, (_k, quads_per_img) in enumerate(sources):
        for pi, q in enumerate(quads_per_img):
            q = np.asarray(q, dtype=np.float64).reshape(-1, 4, 2)
            if len(q):
                quad_list.append(q)
                src_of.append(np.full(len(q), si, np.int32))
                page_of.append(np.full(len(q), pi, np.int32))
    if not quad_list:
        return _no_lines(width_sync, n_img=n_img, src_of=z32, page_of=z32, perm=None, keep=np.zeros(0, np.int64), n_all=0)
    quads = np.concatenate(quad_list, axis=0)
    src_of, page_of = np.concatenate(src_of), np.concatenate(page_of)
    perm = None
    if image_keys is not None:      # pooled order: by key (page), then source / image / line as collected
        key = np.array([image_keys[si][pi] for si, pi in zip(src_of.tolist(), page_of.tolist())], dtype=np.int64)
        perm = np.argsort(key, kind="stable")
        quads, src_of, page_of, key = quads[perm], src_of[perm], page_of[perm], key[perm]
    mats, cws_a, chs_a, ok = quads_to_crop_matrices(quads)
    rots_a = (chs_a / cws_a >= 2.0).astype(np.int32)  # ocr_utils.py:531-534 rotates crops with h/w >= 2
    return plan_lines(dict(n_img=n_img, src_of=src_of, page_of=page_of, perm=perm, n_all=len(quads)), mats, cws_a, chs_a, rots_a, ok,
                      key if image_keys is not None else None, len(sources), strict=strict, two_stage=two_stage,
                      lines_in_launch=lines_in_launch, chunking=chunking, rec_batch_num=rec_batch_num, rec_width_multiple=rec_width_multiple,
                      n_cu=n_cu, n_streams=n_streams, use_cls=use_cls, host_native=host_native, want_words=want_words, width_sync=width_sync)


def plan_lines(pooling: dict, mats: np.ndarray, cws_a: np.ndarray, chs_a: np.ndarray, rots_a: np.ndarray, ok: np.ndarray,
               key: Optional[np.ndarray], n_sources: int, *, strict: bool, two_stage: bool, lines_in_launch: bool, chunking: str,
               rec_batch_num: int, rec_width_multiple: int, n_cu: int, n_streams: int, use_cls: bool = False, host_native: bool = True,
               want_words: bool = False, width_sync: Optional[Callable] = None) -> RecPlan:
    """The plan of a pooled line list that is given as crops: per pooled line its crop -> source homography `mats` [n, 9], crop size
    `cws_a` x `chs_a`, `rots_a` (1: the recogniser sees np.rot90 of the crop) and `ok` (False: no crop exists, the line gets ("", 0.0)).
    `pooling`: n_img, src_of, page_of, perm, n_all of the RecPlan; `key`: the pooling key per line, or None.  `plan_rec` ends here;
    `n_sources` = 0 (ocr_model.Mi355RapidOcrModel: every line names its own source, rd_line_warp_sources) lists no warp launches."""
    src_of, page_of = pooling["src_of"], pooling["page_of"]
    keep = np.nonzero(ok)[0]                      # degenerate quads (zero-area / collinear corners) get ("", 0.0)
    n = len(keep)
    pooling = dict(pooling, keep=keep)
    if n == 0:
        return _no_lines(width_sync, **pooling)
    mats, cws_a, chs_a, rots_a = mats[keep], cws_a[keep], chs_a[keep], rots_a[keep]
    eff_w = np.where(rots_a == 1, chs_a, cws_a)
    eff_h = np.where(rots_a == 1, cws_a, chs_a)
    ratios = (eff_w / eff_h).tolist()
    lines_mode = strict and two_stage
    if want_words and not lines_mode:
        raise RuntimeError("word boxes need the strict two-stage recogniser (rec_mode='strict', RD_REC_TWO_STAGE unset)")
    line_ratio = None
    if lines_mode:
        given = None
        if width_sync is not None:  # the widths come from the pooled lines of every rank; key = the image key (global page index)
            line_keys = key[keep] if key is not None else page_of[keep].astype(np.int64)
            given = width_sync(line_keys, np.asarray(ratios, dtype=np.float64))
        batches, line_w, line_ratio = ocr_host.rec_batches_lines(ratios, n_cu=n_cu, with_ratio=True, given=given, native=host_native)
        if not lines_in_launch:
            # same lines, same order, same reference width per line - but a launch holds lines of ONE width (a line's result depends
            # on its pixels and its padded width only, so the launch boundaries do not enter the result)
            batches = ocr_host.rec_batches_equal_width(np.concatenate([c for c, _w in batches]), line_w)
    elif not strict and chunking == "adaptive":
        batches = ocr_host.rec_batches_adaptive(ratios, width_multiple=rec_width_multiple, n_cu=n_cu)
    else:
        batches = ocr_host.rec_batches(ratios, rec_batch_num, width_multiple=rec_width_multiple, strict=strict, merge_equal_width=strict)
    order_all = np.concatenate([c for c, _ in batches])
    if not lines_mode:
        line_w = np.concatenate([np.full(len(c), w) for c, w in batches])     # every line of a launch is as wide as the launch
    descs = np.zeros(n, dtype=LINE_DTYPE)
    descs["page"] = page_of[keep][order_all]
    descs["out_w"] = np.minimum(line_w, np.ceil(ocr_host.REC_IMG_H * (eff_w / eff_h)[order_all])).astype(np.int32)
    descs["crop_w"] = cws_a[order_all].astype(np.int32)
    descs["crop_h"] = chs_a[order_all].astype(np.int32)
    descs["m"] = mats[order_all]
    descs["rot90"] = rots_a[order_all]
    # packed uint8 scratch of the rectified crops, one region per rec batch (batches run on different streams)
    crop_bytes = (descs["crop_w"].astype(np.int64) * descs["crop_h"] * 3 + 15) // 16 * 16
    nb = len(batches)
    starts = np.cumsum([0] + [len(c) for c, _ in batches])
    offs = np.zeros(n, np.int64)
    batch_scratch = []
    for b in range(nb):
        cb = crop_bytes[starts[b]:starts[b + 1]]
        offs[starts[b]:starts[b + 1]] = np.cumsum(cb) - cb
        batch_scratch.append(int(cb.sum()))
    if max(batch_scratch) >= 2 ** 31:
        raise RuntimeError("a rec batch needs >= 2 GB of crop scratch: lower rec_batch_num")
    descs["scratch_off"] = offs.astype(np.int32)
    plan = RecPlan(**pooling, lines_mode=lines_mode, two_stage=two_stage, lines_in_launch=lines_mode and lines_in_launch,
                   crop_w=cws_a, crop_h=chs_a, rot90=rots_a, eff_w=eff_w, eff_h=eff_h, ratios=ratios,
                   order_all=order_all, line_ids=keep[order_all], line_w=line_w, line_ratio=line_ratio, batches=batches, starts=starts,
                   descs=descs, batch_base=np.cumsum([0] + batch_scratch))
    # stage-1 (warp) launches: per rec batch, one per source image array present in it.  A single source (the page
    # pipeline) needs no second descriptor array: the batch's own descriptors are the launch's.
    crop_px = descs["crop_w"].astype(np.int64) * descs["crop_h"]
    plan.warp_jobs = []
    if n_sources == 0:
        plan.warp_jobs = [[] for _ in range(nb)]
    elif n_sources > 1:
        src_sorted = src_of[keep][order_all]
        warp_order = np.concatenate([starts[b] + np.argsort(src_sorted[starts[b]:starts[b + 1]], kind="stable") for b in range(nb)])
        plan.descs_warp = descs[warp_order]
        ws_sorted = src_sorted[warp_order]
        px_sorted = crop_px[warp_order]
        for b in range(nb):
            lo, hi = int(starts[b]), int(starts[b + 1])
            cuts = [lo] + [i for i in range(lo + 1, hi) if ws_sorted[i] != ws_sorted[i - 1]] + [hi]
            plan.warp_jobs.append([(int(ws_sorted[a]), a, e - a, int(px_sorted[a:e].max())) for a, e in zip(cuts[:-1], cuts[1:])])
    else:
        for b in range(nb):
            lo, hi = int(starts[b]), int(starts[b + 1])
            plan.warp_jobs.append([(0, lo, hi - lo, int(crop_px[lo:hi].max()))])
    if use_cls:
        # the classifier's pre-process: the same crops, resized to 48 x min(192, ceil(48 w / h)) and zero-padded to 192 columns
        plan.descs_cls = descs.copy()
        plan.descs_cls["out_w"] = np.minimum(CLS_IMG_W, np.ceil(CLS_IMG_H * (eff_w / eff_h)[order_all])).astype(np.int32)
    if two_stage:
        _plan_tokens(plan, n_streams)
    return plan


def _plan_tokens(plan: RecPlan, S: int) -> None:
    """The two-stage recogniser's token buffer: the launches run the backbone only, each into its slice; the neck + CTC head then run
    once per GROUP of S consecutive launches (one per stream)."""
    starts, nb = plan.starts, len(plan.batches)
    w2_ = (np.asarray(plan.line_w, dtype=np.int64) - 1) // 2 + 1
    seq_line = ((w2_ - 1) // 2 + 1) // 2                  # tokens per line (rd_rec_seq_len of its padded width)
    groups = [list(range(g, min(g + S, nb))) for g in range(0, nb, S)]
    plan.group_lens = [seq_line[int(starts[grp[0]]): int(starts[grp[-1] + 1])] for grp in groups]
    # every group's tail call is padded with dummy lines onto a coarse (lines, longest line, tokens) grid: the plan cache
    # of the tail handle then sees a handful of keys instead of a new one per group (engine.pad_tail_lengths)
    plan.group_pad = [pad_tail_lengths(l) for l in plan.group_lens]
    plan.group_base = np.cumsum([0] + [int(lp.sum()) for lp, _t in plan.group_pad])
    first_tok = np.zeros(plan.n, np.int64)                 # first token of every line in the token buffer
    for gi, grp in enumerate(groups):
        lo, hi = int(starts[grp[0]]), int(starts[grp[-1] + 1])
        first_tok[lo:hi] = int(plan.group_base[gi]) + np.cumsum(seq_line[lo:hi]) - seq_line[lo:hi]
    plan.seq_line, plan.groups, plan.first_tok = seq_line, groups, first_tok
    plan.tok_lo = [int(first_tok[int(starts[bi])]) for bi in range(nb)]
    if plan.lines_in_launch:
        plan.linetab = rec_line_table(plan.line_w, first_tok)
