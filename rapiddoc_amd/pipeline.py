"""Device-resident page-batch hot path: layout backbone -> OCR det -> line crops -> OCR rec -> CTC decode.

Mirrors the stage order of the reference's `BatchAnalyze.__call__`
(rapid_doc/backend/pipeline/batch_analyze.py:78-164) for the stages whose networks are readable in the
reference: page images stay in HBM as u8 HWC, every resize / normalise / crop is a HIP
kernel, the three forwards run through the C-ABI, and only (idx, prob) per CTC time step and the text-line
boxes cross PCIe.
"""
from __future__ import annotations

import os
import time
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ocr_host
from .engine import RdEngine, preproc_resize_norm, preproc_resize_norm_batch, preproc_resize_norm_sources, resize_source_view
from .host_stage import HostImageStage, as_stage_image, pack_images, plan_offsets
from .rec_plan import (CLS_IMG_H, CLS_IMG_W, LINE_DTYPE, LINE_SOURCE_DTYPE, RecPlan, plan_lines, plan_rec,     # noqa: F401  (the crop helpers are imported from here)
                       quad_to_crop_matrix, quads_to_crop_matrices)

LAYOUT_SIZE = 800          # PP-DocLayout-L/plus-L/V2/V3 input (pp_doclayout/main.py:17-29)
DET_LIMIT = 960            # rapidocr Det.limit_side_len (rapid_ocr.py:517-518)


class CropDesc(C.Structure):
    _fields_ = [("page", C.c_int32), ("out_w", C.c_int32), ("crop_w", C.c_float), ("crop_h", C.c_float),
                ("m", C.c_float * 9), ("rot90", C.c_int32), ("pad_", C.c_int32)]


def cls_flip_rule(prob: np.ndarray, thresh: float) -> np.ndarray:
    """The decision rd_line_flip180_batch makes per line from the classifier's softmax [n,2], restated on the host: turned when label 1
    (180 degrees) wins and its score is at or above the threshold."""
    p = np.asarray(prob, dtype=np.float32).reshape(-1, 2)
    return (p[:, 1] > p[:, 0]) & (p[:, 1] >= np.float32(thresh))


def flip180(crop: np.ndarray) -> np.ndarray:
    """cv2.rotate(crop, cv2.ROTATE_180) of an [h,w,3] image: the pixel order reversed (what rd_line_flip180_batch does in place)."""
    return np.ascontiguousarray(np.asarray(crop)[::-1, ::-1])


CROP_DTYPE = np.dtype([("page", "<i4"), ("out_w", "<i4"), ("crop_w", "<f4"), ("crop_h", "<f4"), ("m", "<f4", (9,)),
                       ("rot90", "<i4"), ("pad_", "<i4")])
assert CROP_DTYPE.itemsize == C.sizeof(CropDesc)


def boxes_to_quads(boxes_xyxy: np.ndarray) -> np.ndarray:
    b = np.asarray(boxes_xyxy, dtype=np.float32).reshape(-1, 4)
    return np.stack([b[:, [0, 1]], b[:, [2, 1]], b[:, [2, 3]], b[:, [0, 3]]], axis=1)


def page_det_shape(H: int, W: int) -> Tuple[int, int]:
    """The det input shape of an H x W page, by the rule of `PagePipeline.det_preprocess`: 64-px bucket of the page with its 50-px
    margins, then DetResizeForTest with limit 960 / "max"."""
    bh, bw = -(-(int(H) + 100) // 64) * 64, -(-(int(W) + 100) // 64) * 64
    return ocr_host.det_resize_shape(bh, bw, DET_LIMIT, "max")


def group_pages_by_det_shape(page_hws: Sequence[Tuple[int, int]]):
    """Pages of different sizes -> (det shape per page, groups, inverse): `groups` = [((dh, dw), page indices)] of the pages that share a
    det input shape, in order of first appearance (members in page order); `inverse[i]` = position of page i in the concatenation of
    the groups' members, so that `grouped[inverse[i]]` is page i again."""
    shapes = [page_det_shape(h, w) for h, w in page_hws]
    members: Dict[Tuple[int, int], List[int]] = {}
    for i, s in enumerate(shapes):
        members.setdefault(s, []).append(i)         # dicts keep insertion order: first appearance
    groups = list(members.items())
    inverse = np.zeros(len(shapes), np.int64)
    inverse[[i for _s, m in groups for i in m]] = np.arange(len(shapes))
    return shapes, groups, inverse


def split_page_list(pages: Sequence) -> Tuple[str, list]:
    """A list of [H_i, W_i, 3] uint8 pages -> ("device", the tensors) or ("host", numpy arrays as rd_stage_pack takes them).  A list that
    mixes device and host pages, an empty list and a page of another dtype or rank raise ValueError."""
    if len(pages) == 0:
        raise ValueError("a page list must hold at least one page")
    on_dev = [isinstance(p, torch.Tensor) and p.is_cuda for p in pages]
    if any(on_dev) and not all(on_dev):
        raise ValueError("a page list must be all device tensors or all host pages (numpy arrays / CPU tensors), not a mix")
    out = []
    for p in pages:
        if tuple(p.shape[2:]) != (3,) or len(p.shape) != 3 or p.shape[0] < 1 or p.shape[1] < 1:
            raise ValueError(f"a page of a list must be [H, W, 3], got shape {tuple(p.shape)}")
        if p.dtype != (torch.uint8 if isinstance(p, torch.Tensor) else np.uint8):
            raise ValueError(f"a page of a list must be uint8, got {p.dtype}")
        out.append(p if on_dev[0] else as_stage_image(p.numpy() if isinstance(p, torch.Tensor) else p))
    if on_dev[0] and any(p.device != out[0].device for p in out):
        raise ValueError("the device pages of a list must lie on one device")
    return ("device" if on_dev[0] else "host"), out


@dataclass
class PageResult:
    lines: List[Tuple[np.ndarray, str, float]] = field(default_factory=list)  # (quad 4x2, text, score)
    layout_feats: Optional[List[torch.Tensor]] = None
    # PagePipeline(use_cls=True): per line (turned by 180 degrees before recognition?, the classifier's label 0 / 1, that label's
    # probability) - rapidocr's ClsPostProcess pair plus the decision of its threshold rule; None when the stage is off
    cls: Optional[List[Tuple[bool, int, float]]] = None


@dataclass(slots=True)
class _RecLaunch:
    """One launch of the recogniser stage, filled as its work is enqueued.  With the two-stage recogniser in lines mode the tail call of
    a group of launches has ONE set of products: they sit on the group's last launch (`rows`, `cols`; `idx`, `prob` when tests keep them)."""
    x: Optional[torch.Tensor] = None                # the input tensor (a clone under keep_rec_inputs: the buffer is reused)
    event: Optional[torch.cuda.Event] = None        # its backbone (or whole network) is done: what the tail and the prefetch wait for
    done: Optional[torch.cuda.Event] = None         # its rows are home
    idx: Optional[torch.Tensor] = None
    prob: Optional[torch.Tensor] = None
    rows: Optional[torch.Tensor] = None             # pinned CTC rows (None: device_ctc off)
    cols: Optional[Tuple[torch.Tensor, torch.Tensor]] = None    # want_words: pinned kept columns and their probabilities
    cls_prob: Optional[torch.Tensor] = None         # use_cls: pinned softmax and turn decisions of its lines
    cls_flip: Optional[torch.Tensor] = None


class PagePipeline:
    def __init__(self, states: Dict[str, object], device: int = 0, characters: Optional[Sequence[str]] = None,
                 rec_batch_num: Optional[int] = None, rec_width_multiple: int = 32, keep_feats: bool = False, n_rec_streams: int = 4,
                 rec_mode: Optional[str] = None, rec_chunking: Optional[str] = None, use_cls: bool = False, cls_thresh: float = 0.9):
        """`states`: {'ppocrv6_det': ..., 'ppocrv6_rec': ..., 'pphgnetv2_b4': ...}, each a .safetensors path,
        bytes, or name->ndarray dict.  The detector may be given as 'ppocrv5_det_server' instead of 'ppocrv6_det' (PPHGNetV2-B4 + LKPAN +
        PFHeadLocal) or as 'ppocrv5_det_mobile' (PPLCNetV3 + RSEFPN + DBHead) or as 'ppocrv3_det_mobile' (MobileNetV3 + RSEFPN + DBHead: the multilingual and the
        English PP-OCRv3 files); exactly one of the four, exposed as `det_kind`: pre-process, DB post-process, prefetch and the range guard do not
        care which network drew the map.  The recogniser may be given as 'ppocrv5_rec_server' instead of 'ppocrv6_rec' (PPHGNetV2-B4 +
        SVTR neck + CTC): strict mode then runs the backbone stage once per distinct reference width (that kind has no per-line widths
        inside a launch), everything behind the token buffer - the ragged tail, the collapse, word boxes - is the same.  Or as
        'ppocrv5_rec_mobile' (PPLCNetV3 + the same neck): that kind computes per-line widths inside a launch, so strict mode plans its
        launches as for v6.  Or as 'ppocr_rec_mv1e' (MobileNetV1Enhance + the SVTR neck at dims 64: the ten multilingual PP-OCRv3 / v4
        mobile files), which computes per-line widths inside a launch too.

        `rec_mode`: how the text lines are batched for the recogniser.  A line's logits depend on its batch's padded width
        (LightSVTR attends over the zero-padded columns), so the batching is part of the result:
          "strict"      (the default) the reference's batching, result for result: every line of the call pooled, ONE
                        `np.argsort(ratios)` with numpy's default sort, chunks of `rec_batch_num` = 6 (rapidocr's default),
                        every line padded to int(48 * max ratio of ITS chunk) (rapid_ocr.py:404-449).  The launches are
                        GPU-sized all the same: runs of the sorted list (sizes from `rd_rec_plan_chunks`) share one tensor
                        and the backbone computes every line at its own padded width inside it
                        (`rd_rec_backbone_forward_lines`; `ocr_host.rec_batches_lines`).  `rec_batch_num` /
                        `rec_width_multiple` are ignored.  (With RD_REC_TWO_STAGE=0: one launch per distinct padded width.)
          "throughput"  (chosen when `rec_batch_num` or `rec_chunking` is given without a mode) GPU-sized chunks (`rec_batch_num` lines, default 64) of the same aspect-sorted list, padded width
                        rounded up to `rec_width_multiple`: same per-tensor parity with the oracle, different padded
                        widths than the reference would have used.  `rec_chunking="adaptive"` (the default when no
                        `rec_batch_num` is given - what bench.py measures) lets the chunk SIZE follow the width:
                        `ocr_host.rec_batches_adaptive` picks, chunk by chunk, the size with the most lines per estimated
                        microsecond, i.e. tile counts of the persistent kernels that fill whole rounds of the 256 CUs (64 lines
                        of width 1056 are 3.09 rounds of mixer tiles and cost four).

        `use_cls` (default False: RapidDoc's own page driver never classifies, rapid_ocr.py:51 turns `Global.use_cls` off): rapidocr's
        det -> crop -> cls -> rec order on the device.  `states` must then carry 'ppocr_cls_mobile' (ch_ptocr_mobile_v2.0_cls_mobile).
        Per rec batch, on that batch's stream, between the warp and the recogniser's resize: the classifier's pre-process (linear resize
        to 48 rows, width min(192, ceil(48 w / h)), (x / 255 - 0.5) / 0.5, zero right-padding to 192 - the arithmetic of
        rd_line_resize_norm_batch with a second descriptor array), `rd_cls_forward` on all lines of the batch at once (the reference's
        chunks of cls_batch_num = 6 cannot change a result: the width is fixed and BatchNorm / squeeze-excite work per image), and
        `rd_line_flip180_batch`, which turns every crop with label 1 and a score >= `cls_thresh` by 180 degrees in place.  No host
        synchronisation is added; the decisions come home with the step's results (`PageResult.cls`).  (+) rapidocr's TextClassifier
        source is not available to this project's build: the pre-process and the threshold rule are restated from the public PaddleOCR
        definition (ppocr ClsPostProcess / tools/infer/predict_cls.py: cls_image_shape 3 x 48 x 192, `'180' in label and score >
        cls_thresh` - here label 1 with score >= cls_thresh) and are NOT pinned against the package.  With `want_words` the stage
        raises ValueError: rapidocr defines no word-box mapping for turned lines."""
        self.use_cls, self.cls_thresh = bool(use_cls), float(cls_thresh)
        if self.use_cls and "ppocr_cls_mobile" not in states:
            raise ValueError("use_cls=True needs the text-line classifier's weights: states['ppocr_cls_mobile'] (ch_ptocr_mobile_v2.0_cls_mobile)")
        if rec_mode is None:
            rec_mode = "strict" if rec_batch_num is None and rec_chunking is None else "throughput"
        if rec_mode not in ("strict", "throughput"):
            raise ValueError("rec_mode must be 'strict' or 'throughput'")
        if rec_chunking is None:
            rec_chunking = "adaptive" if rec_batch_num is None else "fixed"
        if rec_batch_num is None:
            rec_batch_num = 64
        if rec_chunking not in ("fixed", "adaptive"):
            raise ValueError("rec_chunking must be 'fixed' or 'adaptive'")
        self.rec_mode = rec_mode
        self.rec_chunking = rec_chunking
        if rec_mode == "strict":
            rec_batch_num, rec_width_multiple = 6, 1
        self.device = device
        self.tdev = torch.device("cuda", device)
        self.n_cu = int(torch.cuda.get_device_properties(self.tdev).multi_processor_count)   # the chunk planners' round size
        # several forwards are in flight at once here, so the engines defer the split-fp16 range guard: run_batch (det,
        # layout) and rec_forward_lines (rec) call check_range_and_fallback() before any result is used
        # (reuse_outputs: the engines hand out the same output tensors for the same shape - every result is consumed inside the
        #  step that produced it - so that buffer addresses repeat from step to step and the library replays a forward as ONE
        #  hipGraph launch; the buffers this class owns are kept per role for the same reason, `_buf`)
        det_kinds = [k for k in ("ppocrv6_det", "ppocrv5_det_server", "ppocrv5_det_mobile", "ppocrv3_det_mobile") if k in states]
        if len(det_kinds) != 1:
            raise ValueError("states must carry exactly one detector: 'ppocrv6_det' or 'ppocrv5_det_server' or 'ppocrv5_det_mobile' or 'ppocrv3_det_mobile'")
        self.det_kind = det_kinds[0]
        self.det = RdEngine(self.det_kind, device, guard="deferred", reuse_outputs=True).load_weights(states[self.det_kind])
        # rec batches are independent: they alternate between `n_rec_streams` HIP streams (one engine handle = one
        # workspace per stream) so that the launch gaps / tails of one batch are filled by kernels of the other
        rec_kinds = [k for k in ("ppocrv6_rec", "ppocrv5_rec_server", "ppocrv5_rec_mobile", "ppocr_rec_mv1e") if k in states]
        if len(rec_kinds) != 1:
            raise ValueError("states must carry exactly one recogniser: 'ppocrv6_rec' or 'ppocrv5_rec_server' or 'ppocrv5_rec_mobile' or 'ppocr_rec_mv1e'")
        self.rec_kind = rec_kinds[0]
        # strict mode: lines of different reference widths share a launch only where the kind computes per-line widths inside one
        self.rec_lines_in_launch = self.rec_kind in ("ppocrv6_rec", "ppocrv5_rec_mobile", "ppocr_rec_mv1e")
        self.rec_engines = [RdEngine(self.rec_kind, device, guard="deferred").load_weights(states[self.rec_kind]) for _ in range(max(1, n_rec_streams))]
        self.rec = self.rec_engines[0]
        self.rec_streams = [torch.cuda.Stream(device=self.tdev) for _ in self.rec_engines]
        # neck + CTC head of the two-stage recogniser: own handle (own workspace) and stream, it runs under the next backbones
        self.rec_tail = RdEngine(self.rec_kind, device, guard="deferred").load_weights(states[self.rec_kind])
        # the optional text-line direction classifier: one handle (one workspace) per rec stream, as the recogniser's
        self.cls_engines = ([RdEngine("ppocr_cls_mobile", device, guard="deferred").load_weights(states["ppocr_cls_mobile"]) for _ in self.rec_engines]
                            if self.use_cls else [])
        self.last_cls = None
        self.tail_stream = torch.cuda.Stream(device=self.tdev)
        self.layout_stream = torch.cuda.Stream(device=self.tdev)
        # det runs on a stream of its own, so that the NEXT batch's det + layout forwards can be enqueued under this batch's
        # recognition (`run_batch(..., prefetch=next_pages)`): `_front` / `_prefetched`
        self.front_stream = torch.cuda.Stream(device=self.tdev)
        self._prefetched: Optional[dict] = None
        self._after_rec_enqueue = None    # one-shot hook of _rec_forward_sources_once: called with the backbones' events once they are all enqueued
        # where in a batch's recognition the next batch's det forward may start: after this fraction of the rec launches (1.0 = when
        # the last backbone is done, i.e. under the neck + CTC head, the decode and the step boundary, where the GPU runs under-filled;
        # earlier, its small kernels only take CUs away from the persistent recognition kernels: measured slower)
        self.prefetch_gate = float(os.environ.get("RD_PREFETCH_GATE", "1.0"))
        self.layout = RdEngine("pphgnetv2_b4", device, guard="deferred", reuse_outputs=True).load_weights(states["pphgnetv2_b4"]) if "pphgnetv2_b4" in states else None
        self._bufs: Dict[tuple, torch.Tensor] = {}
        ncls = self.rec.num_classes
        self.characters = list(characters) if characters is not None else ["blank"] + [chr(0x4E00 + i) for i in range(ncls - 2)] + [" "]
        assert len(self.characters) == ncls, (len(self.characters), ncls)
        self.rec_batch_num = rec_batch_num
        self.rec_width_multiple = rec_width_multiple
        self.keep_feats = keep_feats
        # CTC greedy decode on the device (rd_ctc_collapse): only finished strings + confidences cross PCIe
        tab, self._ctc_max_len = ocr_host.char_table(self.characters)
        self._ctc_table = torch.from_numpy(tab).to(self.tdev)
        self.device_ctc = True
        self.device_db = True            # DB post-process with the maps staying in HBM (ocr_host.db_postprocess_device)
        # the host stages between the GPU stages - box ordering + merging, the strict mode's line widths, CTC rows -> strings - as one
        # library call each; False (RD_HOST_NATIVE=0): the Python restatements of ocr_host, which define the result
        self.host_native = ocr_host.host_native_default()
        self.db_ws: dict = {}            # its device workspaces / pinned result buffers: per pipeline = per host thread and stream
        # recogniser in two stages: the batches run only the backbone (each into its slice of one token buffer) on their
        # streams, then the LightSVTR neck + CTC head run ONCE over all lines (rd_rec_tail_forward); RD_REC_TWO_STAGE=0: whole
        # network batch by batch
        self.rec_two_stage = os.environ.get("RD_REC_TWO_STAGE", "1") != "0"
        # page-sharded runs (dist.GlobalLineWidths): callable (pooling keys int64 [n], aspect ratios float64 [n]) -> (reference width, max_wh_ratio)
        # per line, decided over the lines of EVERY rank; None = this process holds the whole page batch
        self.rec_width_sync = None
        self._sync_this_call = True       # False inside a rec_forward_sources(pooled=False) call: its widths are its own lines'
        self._width_sync_cache = None
        self._width_sync_epoch, self._in_run_batch = 0, False
        self.keep_rec_inputs = False      # tests: keep every rec batch's input tensor and raw (idx, prob) in last_rec_batches
        self.last_rec_batches: List[Tuple[np.ndarray, torch.Tensor, torch.Tensor, torch.Tensor]] = []
        self._raw_scores = False          # True inside rec_forward_crops: the scores as the recogniser gives them, not as analyze_utils.py:280 prints them
        self._lib = _lib.load()
        self.stats: Dict[str, float] = {}

    # ---------------------------------------------------------------- stages
    def _buf(self, role, numel: int, dtype=torch.float32) -> torch.Tensor:
        """A persistent 1-D device buffer per role, grown (x 1.25) when a call needs more: the same role gets the same address
        step after step (hipGraph replays are keyed on the addresses)."""
        key = (role, dtype)
        t = self._bufs.get(key)
        if t is None or t.numel() < numel:
            t = self._bufs[key] = torch.empty(int(numel * 1.25) + 64, dtype=dtype, device=self.tdev)
        return t[:numel]

    def layout_preprocess(self, pages: torch.Tensor) -> torch.Tensor:
        """PPPreProcess for the whole batch in one launch: INTER_CUBIC resize, /255, mean 0 / std 1 (pre_process.py:14-42)."""
        P = pages.shape[0]
        out = self._buf("layout_x", P * 3 * LAYOUT_SIZE * LAYOUT_SIZE).view(P, 3, LAYOUT_SIZE, LAYOUT_SIZE)
        return preproc_resize_norm_batch(pages, (LAYOUT_SIZE, LAYOUT_SIZE), interp=2, out=out)

    def layout_forward(self, pages: torch.Tensor) -> List[torch.Tensor]:
        return self.layout.backbone_forward(self.layout_preprocess(pages))

    def det_preprocess(self, pages: torch.Tensor) -> Tuple[torch.Tensor, Tuple[int, int]]:
        """64-px bucket of the page region with its 50-px white margin, then DetPreProcess (analyze_utils.py:129-188): BGR,
        (x/255 - mean)/std with RapidDoc's Det.mean / Det.std (ocr_host.DET_MEAN), one launch for the batch."""
        P, H, W, _ = pages.shape
        bh, bw = -(-(H + 100) // 64) * 64, -(-(W + 100) // 64) * 64
        dh, dw = ocr_host.det_resize_shape(bh, bw, DET_LIMIT, "max")
        out = self._buf("det_x", P * 3 * dh * dw).view(P, 3, dh, dw)
        x = preproc_resize_norm_batch(pages, (dh, dw), mean=ocr_host.DET_MEAN, std=ocr_host.DET_STD, interp=1, swap_rb=True, out=out)
        return x, (dh, dw)

    def det_forward(self, pages: torch.Tensor) -> Tuple[torch.Tensor, Tuple[int, int]]:
        x, det_hw = self.det_preprocess(pages)
        return self.det.det_forward(x), det_hw

    def rec_forward_lines(self, pages: torch.Tensor, quads_per_page: Sequence[np.ndarray]):
        """All text lines of ONE image array -> [(text, score)] per image: `rec_forward_sources` with a single source."""
        return self.rec_forward_sources([(pages, quads_per_page)])[0]

    def rec_forward_sources(self, sources: Sequence[Tuple[torch.Tensor, Sequence[np.ndarray]]],
                            image_keys: Optional[Sequence[Sequence[int]]] = None, want_words: bool = False,
                            pooled: bool = True):
        """`sources`: [(images [P,H,W,3] u8 on the GPU, text-line quads per image)] - image arrays of DIFFERENT sizes whose
        lines are recognised TOGETHER, the way the reference pools every line of a page batch per language before it sorts
        and chunks them (analyze_utils.py:216-252 -> rapid_ocr.py:404-472).  Returns, per source, per image, [(text, score)]
        in the order of the quads.  `image_keys[source][image]`: the pooled line list is ordered by this key first (stable;
        e.g. the page a region crop came from - the reference pools page by page), which only matters to the strict mode's
        sort when two lines have exactly the same aspect ratio.  Carries the split-fp16 range guard of its rec engines (every caller - run_batch,
        analyze.RegionOcr, RegionTextModel - gets it): a tripped engine is switched to native fp32 and the lines are
        recognised again.  `want_words` (strict two-stage mode only): every line comes back as (text, score, words) with
        words = {cols, confs, n_steps, wh_ratio, max_wh_ratio, crop_hw} - the kept characters' time steps and probabilities and the
        numbers rapidocr's CTCLabelDecode / cal_rec_boxes turn into word boxes (rapiddoc_amd/word_boxes.py; table OCR, analyze_utils.py:308).
        `pooled=False`: a call whose lines the reference does NOT pool across pages (one table's OCR, analyze_utils.py:478-540: one
        recogniser call per table) - its widths depend on its own lines only, so a page-sharded run needs no exchange for it and
        `rec_width_sync` is not consulted (ranks hold different numbers of tables: a collective here would not pair up)."""
        self._sync_this_call = bool(pooled)
        if not self._in_run_batch:          # a call of its own: a new round of the width collective (run_batch opens one per batch)
            self._width_sync_epoch += 1
        out = self._rec_forward_sources_once(sources, image_keys, want_words)
        # a pass can trip a LATER stage only once the earlier one runs in fp32 (an overflowed backbone feeds the tail NaNs or
        # finite-but-huge tokens), so check after every pass; a tripped engine stays in fp32, which bounds the loop
        for _ in range(3):
            if not any([e.check_range_and_fallback() for e in self.rec_engines + [self.rec_tail] + self.cls_engines]):     # list: check every engine
                break
            self.stats["range_fallbacks"] = self.stats.get("range_fallbacks", 0) + 1
            out = self._rec_forward_sources_once(sources, image_keys, want_words)
        return out

    def rec_forward_crops(self, crop_w, crop_h, rot90, ok, scratch_off, scratch: int, scratch_bytes: int, src_descs: Optional[np.ndarray] = None,
                          want_words: bool = False) -> list:
        """The recogniser on lines that are given as CROPS in a scratch buffer the caller owns (ocr_model.Mi355RapidOcrModel: the crops an
        unmodified RapidDoc pools into one `ocr(det=False)` call), pooled as ONE list - the strict mode then batches them exactly as the
        reference's loop does (rapid_ocr.py:404-472).  Line i is the packed uint8 [crop_h[i]][crop_w[i]][3] image at `scratch +
        scratch_off[i]` (BGR, as rapidocr takes it), read by rd_line_resize_norm_batch directly; `rot90[i]`: the recogniser sees np.rot90
        of it; `ok[i]` False: no crop, the line gets ("", 0.0).  `src_descs` (LINE_SOURCE_DTYPE [n], or None): a line whose `src` is
        not 0 is not in the scratch yet - it is warped there from its source image, all such lines of a rec launch by ONE
        rd_line_warp_sources launch (`stats["warp_source_launches"]` counts them).  Returns per line (text, score) in the caller's order,
        the score as the recogniser gives it (with `want_words`: (text, score, words), see rec_forward_sources).  Carries the range guard
        of rec_forward_sources.  `use_cls` pipelines are refused: a turned crop would stay turned in the caller's buffer."""
        if self.use_cls:
            raise ValueError("rec_forward_crops: not available on a use_cls pipeline")
        n = len(crop_w)
        cw, ch = np.asarray(crop_w, dtype=np.float64), np.asarray(crop_h, dtype=np.float64)
        offs = np.asarray(scratch_off, dtype=np.int64)
        if n and (int(scratch_bytes) >= 2 ** 31 or int(offs.max()) >= 2 ** 31):
            raise RuntimeError("rec_forward_crops: the crops of one call must lie inside 2 GB (scratch_off is an int32)")
        pooling = dict(n_img=[1], src_of=np.zeros(n, np.int32), page_of=np.zeros(n, np.int32), perm=None, n_all=n)
        self._sync_this_call = False
        if not self._in_run_batch:
            self._width_sync_epoch += 1

        def once():
            t0 = time.perf_counter()
            self.last_cls = None
            plan = plan_lines(pooling, np.zeros((n, 9)), cw, ch, np.asarray(rot90, dtype=np.int32), np.asarray(ok, dtype=bool), None, 0,
                              **self._plan_modes(self.rec_mode == "strict"), want_words=want_words)
            if plan.n:
                lines = plan.keep[plan.order_all]
                plan.descs["page"] = 0
                plan.descs["scratch_off"] = offs[lines].astype(np.int32)
                plan.batch_base = np.zeros(len(plan.batches) + 1, np.int64)       # every launch reads the caller's buffer from its start
                plan.src_descs = np.zeros(0, LINE_SOURCE_DTYPE)
                plan.src_jobs = [(0, 0)] * len(plan.batches)
                plan.src_scratch_bytes = int(scratch_bytes)
                plan.swap_rb = 0                                                  # the caller's crops are BGR already
                if src_descs is not None:
                    sd = np.ascontiguousarray(src_descs, dtype=LINE_SOURCE_DTYPE)[lines]
                    sd["scratch_off"] = plan.descs["scratch_off"]
                    warp = sd["src"] != 0
                    first = np.concatenate([[0], np.cumsum(warp)])
                    plan.src_descs = np.ascontiguousarray(sd[warp])
                    plan.src_jobs = [(int(first[a]), int(first[e] - first[a])) for a, e in zip(plan.starts[:-1], plan.starts[1:])]
            return self._run_rec_plan(plan, None, want_words, t0, scratch=int(scratch))[0][0]

        self._raw_scores = True
        try:
            out = once()
            for _ in range(3):
                if not any([e.check_range_and_fallback() for e in self.rec_engines + [self.rec_tail]]):
                    break
                self.stats["range_fallbacks"] = self.stats.get("range_fallbacks", 0) + 1
                out = once()
        finally:
            self._raw_scores = False
        return out

    def _synced_widths(self, sync, keys: np.ndarray, ratios: np.ndarray):
        """One collective per recogniser CALL (per page batch inside run_batch): a range-guard repeat (same lines) re-uses the first
        pass's answer - a rank that repeats must not make a collective call its peers do not make."""
        sig = (self._width_sync_epoch, keys.tobytes(), ratios.tobytes())
        if self._width_sync_cache is not None and self._width_sync_cache[0] == sig:
            return self._width_sync_cache[1]
        res = sync(keys, ratios)
        self._width_sync_cache = (sig, res)
        return res

    def _collapse_home(self, name: str, n: int, T: int, call, *extra: torch.Tensor) -> List[torch.Tensor]:
        """What both device CTC collapses share, on the current stream: the row buffer for `n` lines of at most `T` time steps,
        `call(rows pointer, row_bytes)` = the library call, then the rows (and the `extra` device tensors it filled) copied into pinned
        memory; returns the pinned tensors."""
        row_bytes = (16 + T * self._ctc_max_len + 15) // 16 * 16
        rows = torch.empty((n, row_bytes), dtype=torch.uint8, device=self.tdev)
        if call(rows.data_ptr(), row_bytes) != 0:
            raise RuntimeError(f"{name} failed")
        home = []
        for t in (rows,) + extra:
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            home.append(h)
        return home

    def _collapse_rows(self, idx: torch.Tensor, prob: torch.Tensor, nb: int, st, record: bool = True):
        """Device CTC collapse of one batch's (idx, prob) [nb, T] on stream `st` + the D2H of its rows into pinned memory;
        returns (rows or None, event recorded after it or None)."""
        rows = done = None
        with torch.cuda.stream(st):
            if self.device_ctc:
                T = idx.shape[1]
                rows, = self._collapse_home("rd_ctc_collapse", nb, T, lambda out, row_bytes: self._lib.rd_ctc_collapse(
                    self.device, idx.data_ptr(), prob.data_ptr(), nb, T, self._ctc_table.data_ptr(), self._ctc_max_len, len(self.characters),
                    out, row_bytes, st.cuda_stream))
            if record:
                done = torch.cuda.Event()
                done.record(st)
        return rows, done

    def _collapse_lines(self, idx_all: torch.Tensor, prob_all: torch.Tensor, tables: torch.Tensor, n_lines: int, max_tokens: int, st,
                        want_cols: bool = False):
        """Device CTC collapse of the RAGGED lines of one tail call (`tables` = its seg / tokinfo tensor; the first `n_lines` are the
        real ones) on stream `st` + the D2H of the rows into pinned memory; returns (rows, event, kept columns or None)."""
        with torch.cuda.stream(st):
            cols = torch.empty((n_lines, max_tokens), dtype=torch.int16, device=self.tdev) if want_cols else None
            confs = torch.empty((n_lines, max_tokens), dtype=torch.float32, device=self.tdev) if want_cols else None
            rows, *cols_h = self._collapse_home("rd_ctc_collapse_lines", n_lines, max_tokens, lambda out, row_bytes: self._lib.rd_ctc_collapse_lines(
                self.device, idx_all.data_ptr(), prob_all.data_ptr(), n_lines, tables.data_ptr(), max_tokens, self._ctc_table.data_ptr(),
                self._ctc_max_len, len(self.characters), out, row_bytes, cols.data_ptr() if want_cols else None,
                confs.data_ptr() if want_cols else None, st.cuda_stream), *((cols, confs) if want_cols else ()))
            done = torch.cuda.Event()
            done.record(st)
        return rows, done, tuple(cols_h) if want_cols else None

    def _rec_forward_sources_once(self, sources, image_keys=None, want_words=False):
        """One pass of the recogniser stage: plan (host arithmetic, rec_plan.plan_rec), enqueue, decode, scatter."""
        t0 = time.perf_counter()
        if self.use_cls and want_words:
            raise ValueError("use_cls together with want_words: rapidocr defines no word-box mapping for lines turned by 180 degrees")
        self.last_cls = None
        for imgs, _quads in sources:
            assert imgs.is_cuda and imgs.dtype == torch.uint8 and imgs.dim() == 4 and imgs.is_contiguous()
        strict = self.rec_mode == "strict"
        sync = None         # the width collective: a pooled call of the strict two-stage mode of a page-sharded run
        if self.rec_width_sync is not None and strict and self.rec_two_stage and self._sync_this_call:
            sync = lambda keys, ratios: self._synced_widths(self.rec_width_sync, keys, ratios)      # noqa: E731
        plan = plan_rec([(imgs.shape[0], quads) for imgs, quads in sources], image_keys, **self._plan_modes(strict), want_words=want_words,
                        width_sync=sync)
        return self._run_rec_plan(plan, sources, want_words, t0)

    def _plan_modes(self, strict: bool) -> dict:
        """what rec_plan.plan_rec / plan_lines need to know about this pipeline"""
        return dict(strict=strict, two_stage=self.rec_two_stage, lines_in_launch=self.rec_lines_in_launch, chunking=self.rec_chunking,
                    rec_batch_num=self.rec_batch_num, rec_width_multiple=self.rec_width_multiple, n_cu=self.n_cu,
                    n_streams=len(self.rec_engines), use_cls=self.use_cls, host_native=self.host_native)

    def _run_rec_plan(self, plan: RecPlan, sources, want_words: bool, t0: float, scratch: Optional[int] = None):
        """enqueue, decode, scatter of a planned call.  `scratch`: device address of a crop scratch the CALLER owns (rec_forward_crops);
        default: the pipeline's own, grown to the plan's size."""
        scatter = lambda per_line: self._scatter_texts(per_line, plan.src_of, plan.page_of, plan.n_img, plan.perm)      # noqa: E731
        cls_of: List[tuple] = [(False, 0, 0.0)] * plan.n_all
        if plan.n == 0:                 # nothing to recognise: degenerate quads get ("", 0.0)
            if self.use_cls and plan.n_all:
                self.last_cls = scatter(cls_of)
            return scatter([("", 0.0, None) if want_words else ("", 0.0)] * plan.n_all)
        if scratch is None:
            if getattr(self, "_crop_scratch", None) is None or self._crop_scratch.numel() < plan.scratch_bytes:
                self._crop_scratch = torch.empty(int(plan.scratch_bytes * 1.25) + 1024, dtype=torch.uint8, device=sources[0][0].device)
            scratch = self._crop_scratch.data_ptr()
        self.stats["t_descs_ms"] = (time.perf_counter() - t0) * 1e3
        main = torch.cuda.current_stream()
        launches = self._enqueue_rec(plan, sources, want_words, scratch)
        self.stats["t_rec_enqueue_ms"] = (time.perf_counter() - t0) * 1e3 - self.stats["t_descs_ms"]
        hook, self._after_rec_enqueue = self._after_rec_enqueue, None
        if hook is not None:
            t_h = time.perf_counter()
            S, nb = len(self.rec_engines), len(launches)
            m = max(1, min(nb, int(np.ceil(self.prefetch_gate * nb))))
            hook([l.event for l in launches[max(0, m - S): m]])   # streams run their launches in order: the last S up to m cover all before them
            self.stats["t_front_next_ms"] = (time.perf_counter() - t_h) * 1e3
        texts = self._decode_rec(plan, launches, want_words)
        for st in self.rec_streams + [self.tail_stream]:
            main.wait_stream(st)
        self.stats["rec_lines"] = plan.n
        self.stats["rec_batches"] = len(launches)
        self.last_pool_order = plan.perm
        if self.use_cls:       # (every batch's `done` has been waited for above: the copies enqueued in front of its recogniser are complete)
            ph = np.concatenate([l.cls_prob.numpy() for l in launches])
            fh = np.concatenate([l.cls_flip.numpy() for l in launches])
            for j, i in enumerate(plan.line_ids.tolist()):
                label = int(ph[j, 1] > ph[j, 0])
                cls_of[i] = (bool(fh[j]), label, float(ph[j, label]))
            self.last_cls = scatter(cls_of)
            self.last_cls_prob = (plan.line_ids, ph)      # tests: pooled line ids and the raw probabilities
        return scatter(texts)

    def _enqueue_rec(self, plan: RecPlan, sources, want_words: bool, scratch_base: int) -> List[_RecLaunch]:
        """Everything the stage puts on the GPU, in launch order: the descriptor uploads, then per launch `bi` on stream `bi % S` the warp
        jobs, the optional classifier, the recogniser's resize and its forward; with the two-stage recogniser `_enqueue_tail(g)` directly
        after the last launch of group g.  A plan of rec_forward_crops has no warp jobs and carries `src_descs` / `src_jobs` instead: ONE
        rd_line_warp_sources launch per rec launch that has lines to warp."""
        dev, S, lib = (sources[0][0].device if sources else self.tdev), len(self.rec_engines), self._lib
        keep_inputs = self.keep_rec_inputs
        upload = lambda descs: torch.from_numpy(descs.view(np.uint8)).to(dev, non_blocking=True)      # noqa: E731
        descs_dev = upload(plan.descs)
        cls = None
        if self.use_cls:     # (descriptors, device probabilities and flips, their pinned copies)
            cls = (upload(plan.descs_cls), self._buf("cls_prob", 2 * plan.n).view(plan.n, 2), self._buf("cls_flip", plan.n, torch.int32),
                   torch.empty((plan.n, 2), dtype=torch.float32, pin_memory=True), torch.empty((plan.n,), dtype=torch.int32, pin_memory=True))
        descs_warp_dev = upload(plan.descs_warp) if plan.descs_warp is not None else descs_dev
        src_descs_dev = upload(plan.src_descs) if plan.src_descs is not None and len(plan.src_descs) else None
        if keep_inputs:          # tests: the descriptors in launch order, every batch's scratch base and first line; the classifier's inputs
            self.last_rec_descs = (plan.descs.copy(), np.asarray(plan.batch_base, dtype=np.int64), np.asarray(plan.starts, dtype=np.int64))
            self.last_cls_inputs = []
        main = torch.cuda.current_stream()
        ready = torch.cuda.Event()
        ready.record(main)
        tokens = linetab = tables = None
        if plan.two_stage:
            base = plan.group_base
            tokens = self._buf("rec_tokens", int(base[-1]) * self.rec.rec_token_dim).view(int(base[-1]), self.rec.rec_token_dim)
            for gi, lens in enumerate(plan.group_lens):         # the dummy lines' tokens: finite values (their outputs are ignored)
                tokens[int(base[gi]) + int(lens.sum()): int(base[gi + 1])].zero_()
            tables = [self.rec_tail.rec_tail_tables(lp, dev, out=self._buf(("tail_tab", gi), 2 * len(lp) + int(lp.sum()), torch.int32))
                      for gi, (lp, _t) in enumerate(plan.group_pad)]   # uploaded now, used later
            if plan.linetab is not None:
                tab_h = torch.from_numpy(plan.linetab).pin_memory()
                linetab = self._buf("rec_linetab", 4 * plan.n, torch.int32).view(plan.n, 4)
                linetab.copy_(tab_h, non_blocking=True)
                self._keep_linetab = tab_h                        # the pinned source must outlive the asynchronous copy
            ready.record(main)
            self.tail_stream.wait_event(ready)
        launches: List[_RecLaunch] = []
        for bi, (chunk, wpad) in enumerate(plan.batches):
            nb, pos = len(chunk), int(plan.starts[bi])
            k = bi % S
            st = self.rec_streams[k]
            if bi < S:
                st.wait_event(ready)          # descriptors (and the pages, the token buffer) are ready
            with torch.cuda.stream(st):
                # one input buffer per stream (batches bi, bi + S, ... of a stream run one after the other)
                x = self._buf(("rec_x", k), nb * 3 * ocr_host.REC_IMG_H * wpad).view(nb, 3, ocr_host.REC_IMG_H, wpad)
                scratch = scratch_base + int(plan.batch_base[bi])
                if plan.src_jobs is not None and plan.src_jobs[bi][1]:       # stage 1, every line from a source of its own: one launch
                    first, cnt = plan.src_jobs[bi]
                    off = first * LINE_SOURCE_DTYPE.itemsize
                    rc = lib.rd_line_warp_sources(self.device, plan.src_descs.ctypes.data + off, src_descs_dev.data_ptr() + off, cnt, scratch,
                                                  int(plan.src_scratch_bytes), st.cuda_stream)
                    if rc != 0:
                        raise RuntimeError(lib.rd_create_error().decode())
                    self.stats["warp_source_launches"] = self.stats.get("warp_source_launches", 0) + 1
                for si, first, cnt, max_px in plan.warp_jobs[bi]:            # stage 1: page / canvas -> rectified uint8 crops
                    imgs = sources[si][0]
                    rc = lib.rd_line_warp_batch(self.device, imgs.data_ptr(), imgs.shape[0], imgs.shape[1], imgs.shape[2],
                                                descs_warp_dev.data_ptr() + first * LINE_DTYPE.itemsize, cnt, max_px, scratch, st.cuda_stream)
                    if rc != 0:
                        raise RuntimeError("rd_line_warp_batch failed")
                launch = _RecLaunch()
                if cls is not None:           # classify the crops and turn the upside-down ones in the scratch, before the recogniser reads it
                    self._enqueue_cls(launch, cls, descs_dev, k, pos, nb, scratch, plan.line_ids[pos: pos + nb])
                rc = lib.rd_line_resize_norm_batch(self.device, descs_dev.data_ptr() + pos * LINE_DTYPE.itemsize, nb, scratch,
                                                   ocr_host.REC_IMG_H, wpad, plan.swap_rb, x.data_ptr(), st.cuda_stream)   # stage 2
                if rc != 0:
                    raise RuntimeError("rd_line_resize_norm_batch failed")
                if plan.lines_in_launch:
                    self.rec_engines[k].rec_backbone_forward_lines(x, linetab[pos: pos + nb], tokens)
                elif plan.two_stage:
                    self.rec_engines[k].rec_backbone_forward(x, tokens[plan.tok_lo[bi]: plan.tok_lo[bi] + nb * int(plan.seq_line[pos])])
                else:
                    launch.idx, launch.prob, _ = self.rec_engines[k].rec_forward(x)
                    launch.rows, launch.done = self._collapse_rows(launch.idx, launch.prob, nb, st)
                launch.event = launch.done
                if plan.two_stage:
                    launch.event = torch.cuda.Event()
                    launch.event.record(st)
                launch.x = x.clone() if keep_inputs else x
            launches.append(launch)
            if plan.two_stage and ((bi + 1) % S == 0 or bi + 1 == len(plan.batches)):
                self._enqueue_tail(plan, launches, bi // S, tokens, tables[bi // S], want_words)
        return launches

    def _enqueue_cls(self, launch: _RecLaunch, cls, descs_dev, k: int, pos: int, nb: int, scratch: int, line_ids: np.ndarray) -> None:
        """On the current stream (launch's, engine k), for its `nb` lines from position `pos`: the classifier's resize, its forward, the
        180-degree turn of the crops in the scratch and the two copies home."""
        descs_cls_dev, cls_prob, cls_flip, cls_prob_h, cls_flip_h = cls
        stream = torch.cuda.current_stream().cuda_stream
        sl = slice(pos, pos + nb)
        xc = self._buf(("cls_x", k), nb * 3 * CLS_IMG_H * CLS_IMG_W).view(nb, 3, CLS_IMG_H, CLS_IMG_W)
        rc = self._lib.rd_line_resize_norm_batch(self.device, descs_cls_dev.data_ptr() + pos * LINE_DTYPE.itemsize, nb, scratch,
                                                 CLS_IMG_H, CLS_IMG_W, 1, xc.data_ptr(), stream)
        if rc != 0:
            raise RuntimeError("rd_line_resize_norm_batch (classifier) failed")
        self.cls_engines[k].cls_forward(xc, out=cls_prob[sl])
        if self.keep_rec_inputs:
            self.last_cls_inputs.append((line_ids, xc.clone()))
        rc = self._lib.rd_line_flip180_batch(self.device, descs_dev.data_ptr() + pos * LINE_DTYPE.itemsize, nb, cls_prob[sl].data_ptr(),
                                             self.cls_thresh, scratch, cls_flip[sl].data_ptr(), stream)
        if rc != 0:
            raise RuntimeError("rd_line_flip180_batch failed")
        launch.cls_prob, launch.cls_flip = cls_prob_h[sl], cls_flip_h[sl]
        launch.cls_prob.copy_(cls_prob[sl], non_blocking=True)     # home with the step's results: the host reads them
        launch.cls_flip.copy_(cls_flip[sl], non_blocking=True)     # behind the batch's `done`

    def _enqueue_tail(self, plan: RecPlan, launches: List[_RecLaunch], gi: int, tokens: torch.Tensor, tables: torch.Tensor, want_words: bool) -> None:
        """Neck + CTC head over the tokens of group `gi` on the tail stream, behind the group's backbones, and the device CTC collapse:
        ONE launch over the group's ragged lines in lines mode (its products go to the group's last launch), one per launch otherwise.
        Every launch of the group gets the event to wait for in `done`."""
        grp = [launches[bi] for bi in plan.groups[gi]]
        t_lo, t_hi = int(plan.group_base[gi]), int(plan.group_base[gi + 1])
        lens_pad, max_tokens = plan.group_pad[gi]
        for launch in grp:
            self.tail_stream.wait_event(launch.event)
        with torch.cuda.stream(self.tail_stream):
            n_tok = t_hi - t_lo
            idx_all, prob_all = self.rec_tail.rec_tail_forward(
                tokens[t_lo:t_hi], lens_pad, tables, max_tokens=max_tokens,
                out=(self._buf(("tail_idx", gi), n_tok, torch.int32), self._buf(("tail_prob", gi), n_tok)))
        done = None
        if plan.lines_mode:
            last = grp[-1]
            last.rows, done, last.cols = self._collapse_lines(idx_all, prob_all, tables, len(plan.group_lens[gi]), max_tokens, self.tail_stream,
                                                              want_words)
            if self.keep_rec_inputs:
                with torch.cuda.stream(self.tail_stream):        # (after the tail call, on its stream)
                    last.idx, last.prob = idx_all.clone(), prob_all.clone()
        else:
            for bi, launch in zip(plan.groups[gi], grp):
                nb, t = len(plan.batches[bi][0]), int(plan.seq_line[int(plan.starts[bi])])
                lo = plan.tok_lo[bi] - t_lo
                launch.idx, launch.prob = idx_all[lo: lo + nb * t].view(nb, t), prob_all[lo: lo + nb * t].view(nb, t)
                launch.rows, ev = self._collapse_rows(launch.idx, launch.prob, nb, self.tail_stream, record=launch is grp[-1])
                done = ev or done
        for launch in grp:
            launch.done = done

    def _texts_from_rows(self, rows_np: np.ndarray, line_ids: np.ndarray, texts: list) -> None:
        """Collapsed CTC rows -> texts[pooled line] = (text, score as analyze_utils.py:280 prints it), in the library or in Python."""
        if self.host_native:
            txt, conf, conf3 = ocr_host.parse_ctc_rows_native(rows_np)
            for i, t, s in zip(line_ids.tolist(), txt, conf if self._raw_scores else conf3):
                texts[i] = (t, s)
        elif self._raw_scores:
            for i, ts in zip(line_ids.tolist(), ocr_host.parse_ctc_rows(rows_np)):
                texts[i] = ts
        else:
            for i, (t, s) in zip(line_ids.tolist(), ocr_host.parse_ctc_rows(rows_np)):
                texts[i] = (t, ocr_host.format_score(s))

    def _words_from_rows(self, plan: RecPlan, lo: int, rows_np: np.ndarray, cols, texts: list) -> None:
        """`want_words`: rows and kept columns of the lines from launch position `lo` -> texts[pooled line] = (text, raw score, words)
        (raw: the reference's ocr(det=False) returns rapidocr's float as it is, rapid_ocr.py:295-297)."""
        n_kept = rows_np[:, 8:12].copy().view("<i4")[:, 0]
        cols_np, confs_np = cols[0].numpy(), cols[1].numpy()
        for j, (t, sc) in enumerate(ocr_host.parse_ctc_rows(rows_np)):
            i, k = int(plan.order_all[lo + j]), int(n_kept[j])
            words = {"cols": cols_np[j, :k].astype(np.int64).tolist(), "confs": confs_np[j, :k].astype(np.float64).tolist(),
                     "n_steps": int(plan.seq_line[lo + j]), "wh_ratio": float(plan.ratios[i]), "max_wh_ratio": float(plan.line_ratio[lo + j]),
                     "crop_hw": (int(plan.eff_h[i]), int(plan.eff_w[i]))}
            texts[int(plan.keep[i])] = (t, sc, words)

    def _decode_groups(self, plan: RecPlan, launches: List[_RecLaunch], want_words: bool, texts: list) -> list:
        """`_decode_rec` in lines mode: one wait and one set of rows per group of launches (on the group's last launch)."""
        ids, starts = plan.line_ids, plan.starts
        t_dec = 0.0
        for gi, grp in enumerate(plan.groups):
            tail = launches[grp[-1]]
            tail.done.synchronize()
            t1 = time.perf_counter()
            lo, hi = int(starts[grp[0]]), int(starts[grp[-1] + 1])
            if want_words:
                self._words_from_rows(plan, lo, tail.rows.numpy(), tail.cols, texts)
            else:
                self._texts_from_rows(tail.rows.numpy(), ids[lo:hi], texts)
            t_dec += time.perf_counter() - t1
            if tail.idx is not None:    # tests: per rec batch (pooled line ids, input tensor, reference width per line, per-line idx, prob)
                g0 = int(plan.group_base[gi])
                for bi in grp:
                    a, e = int(starts[bi]), int(starts[bi + 1])
                    sl = [(int(plan.first_tok[i]) - g0, int(plan.seq_line[i])) for i in range(a, e)]
                    self.last_rec_batches.append((ids[a:e], launches[bi].x, np.asarray(plan.line_w[a:e]),
                                                  [tail.idx[o: o + t] for o, t in sl], [tail.prob[o: o + t] for o, t in sl]))
        self.stats["t_decode_ms"] = t_dec * 1e3
        return texts

    def _decode_rec(self, plan: RecPlan, launches: List[_RecLaunch], want_words: bool) -> list:
        """Waits group by group (lines mode) or launch by launch and turns the rows that came home into the pooled lines' results; the host
        decode of one overlaps the GPU work of those still in flight.  -> per pooled line (text, score[, words])."""
        texts: List[tuple] = [("", 0.0, None) if want_words else ("", 0.0)] * plan.n_all
        ids, starts = plan.line_ids, plan.starts
        t_dec = 0.0
        if self.keep_rec_inputs:
            self.last_rec_crop_sizes = (plan.crop_w.astype(np.int64), plan.crop_h.astype(np.int64), plan.rot90, plan.keep)
        if self.keep_rec_inputs or plan.lines_mode:
            self.last_rec_batches = []
        if plan.lines_mode:
            return self._decode_groups(plan, launches, want_words, texts)
        for bi, launch in enumerate(launches):
            ids_b = ids[int(starts[bi]): int(starts[bi + 1])]
            if self.keep_rec_inputs:
                self.last_rec_batches.append((ids_b, launch.x, launch.idx, launch.prob))
            launch.done.synchronize()
            if launch.rows is not None:
                t1 = time.perf_counter()
                self._texts_from_rows(launch.rows.numpy(), ids_b, texts)
            else:                       # device_ctc off: the raw (idx, prob) come home and the host collapses them
                idx_h, prob_h = launch.idx.cpu().numpy(), launch.prob.cpu().numpy()
                t1 = time.perf_counter()
                for i, (t, s) in zip(ids_b.tolist(), ocr_host.ctc_decode(idx_h, prob_h, self.characters)):
                    texts[i] = (t, ocr_host.format_score(s))
            t_dec += time.perf_counter() - t1
        self.stats["t_decode_ms"] = t_dec * 1e3
        return texts

    @staticmethod
    def _scatter_texts(texts, src_of, page_of, n_img, perm=None):
        """pooled-order results -> [source][image][line], lines in the order their quads were given"""
        if perm is not None:             # undo the key sort: collection order is (source, image, line)
            inv = np.argsort(perm, kind="stable")
            texts = [texts[i] for i in inv.tolist()]
            src_of, page_of = src_of[inv], page_of[inv]
        out = [[[] for _ in range(k)] for k in n_img]
        for t, si, pi in zip(texts, src_of.tolist(), page_of.tolist()):
            out[si][pi].append(t)
        return out

    # ---------------------------------------------------------------- det maps -> text-line quads (host)
    def boxes_from_maps(self, maps_host: np.ndarray, page_hw: Tuple[int, int], box_thresh: float = 0.3,
                        unclip_ratio: float = 1.8) -> List[np.ndarray]:
        """DB post-process + reading-order sort + same-line merge (rapid_ocr.py:537-538; analyze_utils.py:196-204).
        box_thresh 0.3 / unclip 1.8 are the page-OCR settings (backend/pipeline/model_init.py:73)."""
        P = maps_host.shape[0]
        res = ocr_host.db_postprocess(maps_host, [page_hw] * P, thresh=0.3, box_thresh=box_thresh, unclip_ratio=unclip_ratio,
                                      raw=self.host_native)
        t0 = time.perf_counter()
        if self.host_native:
            out = ocr_host.order_merge_boxes_native(*res)
            self.stats["t_boxes_ms"] = (time.perf_counter() - t0) * 1e3
            return out
        out = []
        for boxes, _scores in res:
            if len(boxes) == 0:
                out.append(np.zeros((0, 4, 2), np.float32))
                continue
            b = ocr_host.sorted_boxes(boxes.astype(np.float32))
            b = ocr_host.merge_det_boxes(b)
            out.append(np.asarray(b, dtype=np.float32).reshape(-1, 4, 2))
        self.stats["t_boxes_ms"] = (time.perf_counter() - t0) * 1e3
        return out

    def boxes_from_maps_device(self, maps_dev: torch.Tensor, page_hw: Tuple[int, int], box_thresh: float = 0.3,
                               unclip_ratio: float = 1.8) -> List[np.ndarray]:
        """`boxes_from_maps` with the maps staying in HBM (ocr_host.db_postprocess_device)."""
        P = maps_dev.shape[0]
        res = ocr_host.db_postprocess_device(maps_dev, [page_hw] * P, thresh=0.3, box_thresh=box_thresh, unclip_ratio=unclip_ratio,
                                             stats=self.stats, cache=self.db_ws, raw=self.host_native)
        t0 = time.perf_counter()
        if self.host_native:
            out = ocr_host.order_merge_boxes_native(*res)
            self.stats["t_boxes_ms"] = (time.perf_counter() - t0) * 1e3
            return out
        out = []
        for boxes, _scores in res:
            if len(boxes) == 0:
                out.append(np.zeros((0, 4, 2), np.float32))
                continue
            b = ocr_host.merge_det_boxes(ocr_host.sorted_boxes(boxes.astype(np.float32)))
            out.append(np.asarray(b, dtype=np.float32).reshape(-1, 4, 2))
        self.stats["t_boxes_ms"] = (time.perf_counter() - t0) * 1e3
        return out

    def _boxes_via_host_maps(self, src: torch.Tensor, page_hw: Tuple[int, int]) -> List[np.ndarray]:
        """Round-1 path: the float maps cross PCIe (pinned buffer) and the whole post-process runs on the host."""
        if getattr(self, "_maps_host", None) is None or self._maps_host.shape != src.shape:
            self._maps_host = torch.empty(src.shape, dtype=torch.float32, pin_memory=True)
        t0 = time.perf_counter()
        self._maps_host.copy_(src, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        t1 = time.perf_counter()
        quads = self.boxes_from_maps(self._maps_host.numpy(), page_hw)
        self.stats["t_wait_maps_ms"] = (t1 - t0) * 1e3
        self.stats["t_db_post_ms"] = (time.perf_counter() - t1) * 1e3 - self.stats["t_boxes_ms"]
        return quads

    # ---------------------------------------------------------------- whole batch
    def run_batch(self, pages: torch.Tensor, quads_per_page: Optional[Sequence[np.ndarray]] = None,
                  det_maps_override: Optional[torch.Tensor] = None, prefetch: Optional[torch.Tensor] = None,
                  page_keys: Optional[Sequence[int]] = None) -> List[PageResult]:
        """`page_keys`: the pages' positions in the GLOBAL page list of a page-sharded run (the pooling key of `rec_width_sync`,
        dist.GlobalLineWidths); default: the local page index.
        `_run_batch_once` plus the range guard of the split-fp16 kernels (include/rapiddoc_mi355.h, rd_range_status):
        an engine that met an operand outside the fp16 range is switched to native fp32 for good and the batch is
        repeated, so a result is never silently wrong.  `pages`: [P,H,W,3] uint8 RGB on the GPU, or host pages (numpy / CPU tensor,
        what the reference's caller holds: batch_analyze.py:108-111), which are uploaded first - a stream of batches should go through
        `PageUploader` instead, whose copies run under the previous batch.

        `prefetch`: the NEXT batch's pages, already on the GPU (valid on the current stream).  Their det and layout forwards are
        enqueued as soon as this batch's det maps have been consumed, so they run under this batch's recognition instead of in
        front of the next batch's; the next `run_batch` call on that very tensor picks them up (any other call drops them).  The
        tensor is recognised by address and shape: its CONTENTS must not change between the two calls.  Results are the same with or
        without it (the same kernels on the same inputs); `last_det` then already belongs to the next batch when this call returns.

        `pages` may also be a SEQUENCE of [H_i, W_i, 3] uint8 pages of different sizes (`_run_list_once`): all device tensors, used
        where they lie, or all host pages, which go through one pinned pack and one copy; a mix raises ValueError.  Pages of equal det
        input shape form a group (one det forward and one DB post-process per group), one rd_preproc_resize_norm_sources launch
        writes every group's det input, and every line of every page is pooled into ONE recogniser plan, so the strict mode's padded
        widths are the reference's for the whole batch.  `det_maps_override` is then a sequence of one [1, 1, dh_i, dw_i] map per page,
        `prefetch` may be a list of device pages, and `last_det` is a list of (maps, det_hw, page indices) per group."""
        if isinstance(pages, (list, tuple)):
            return self._run_batch_list(pages, quads_per_page, det_maps_override, prefetch, page_keys)
        if isinstance(pages, np.ndarray) or not pages.is_cuda:
            src = torch.from_numpy(np.ascontiguousarray(pages)) if isinstance(pages, np.ndarray) else pages.contiguous()
            pages = src.to(self.tdev, non_blocking=src.is_pinned())
        self._page_keys = None if page_keys is None else [int(k) for k in page_keys]
        assert self._page_keys is None or len(self._page_keys) == pages.shape[0]
        if self.rec_width_sync is not None and page_keys is None and getattr(self.rec_width_sync, "world_size", 1) > 1:
            # local page indices would interleave the ranks' pages in the pooled order (every rank has a page 0)
            raise ValueError("rec_width_sync over more than one rank needs page_keys: the pages' positions in the GLOBAL page list")
        self._width_sync_epoch += 1
        self._in_run_batch = True
        try:
            return self._run_batch_guarded(pages, quads_per_page, det_maps_override, prefetch)
        finally:
            self._in_run_batch = False

    def _run_batch_guarded(self, pages, quads_per_page, det_maps_override, prefetch):
        results = self._run_batch_once(pages, quads_per_page, det_maps_override, prefetch)
        # det and the layout backbone (the rec engines are guarded inside rec_forward_lines)
        engines = [self.det] + ([self.layout] if self.layout is not None else [])
        if os.environ.get("RD_DEV_SKIP_RANGE_CHECK") == "1":
            engines = []
        if any([e.check_range_and_fallback() for e in engines]):
            self.stats["range_fallbacks"] = self.stats.get("range_fallbacks", 0) + 1
            self._prefetched = None        # made by the engine that has just been replaced: the next batch computes its own
            results = self._run_batch_once(pages, quads_per_page, det_maps_override, prefetch)
        return results

    @staticmethod
    def _front_key(pages: torch.Tensor) -> tuple:
        return (pages.data_ptr(), tuple(pages.shape))

    def _front(self, pages: torch.Tensor, n_results: int, gate: Sequence[torch.cuda.Event] = ()) -> dict:
        """Enqueue the batch's det forward (front stream) and, behind it, its layout backbone (layout stream).  The det forward starts
        after everything enqueued on the current stream so far - the pages' upload, and the previous batch's use of the det maps,
        whose buffer it overwrites - and after the `gate` events."""
        cur = torch.cuda.current_stream()
        h = {"key": self._front_key(pages), "feats": None, "layout_done": None}
        self.front_stream.wait_stream(cur)
        for ev in gate:
            self.front_stream.wait_event(ev)
        with torch.cuda.stream(self.front_stream):
            h["prob_maps"], h["det_hw"] = self.det_forward(pages)
            h["det_done"] = torch.cuda.Event()
            h["det_done"].record(self.front_stream)
        # the layout backbone keeps the GPU busy (on its own stream, so it also overlaps the recognition batches that follow)
        # while the host turns the det maps into boxes
        if self.layout is not None:
            self.layout_stream.wait_event(h["det_done"])       # det first: it is on the batch's critical path, the layout features are not
            with torch.cuda.stream(self.layout_stream):
                feats = self.layout_forward(pages)
                if self.keep_feats:                   # copies: the engine re-uses its output tensors on the next call of this shape
                    h["feats"] = [[f[i].clone() for f in feats] for i in range(n_results)]
                h["layout_done"] = torch.cuda.Event()
                h["layout_done"].record(self.layout_stream)
        return h

    def _run_batch_once(self, pages: torch.Tensor, quads_per_page: Optional[Sequence[np.ndarray]] = None,
                        det_maps_override: Optional[torch.Tensor] = None, prefetch: Optional[torch.Tensor] = None) -> List[PageResult]:
        """pages: [P,H,W,3] uint8 RGB on the GPU.  Text-line quads come from the DB post-process of the det maps
        unless `quads_per_page` is given.  `det_maps_override` (benchmark / tests with random weights, whose maps carry
        no text): device maps [P,1,h,w] that replace the network's output as the post-process input - the det forward
        still runs."""
        assert pages.is_cuda and pages.dtype == torch.uint8 and pages.dim() == 4
        P, H, W, _ = pages.shape
        results = [PageResult() for _ in range(P)]
        cur = torch.cuda.current_stream()
        h, self._prefetched = self._prefetched, None
        if h is None or h["key"] != self._front_key(pages):
            h = self._front(pages, P)
            self.stats["front_prefetched"] = 0.0
        else:
            self.stats["front_prefetched"] = 1.0
        cur.wait_event(h["det_done"])
        if self.rec_width_sync is not None and self.det.precision != "fp32" and os.environ.get("RD_DEV_SKIP_RANGE_CHECK") != "1":
            # page-sharded strict mode: the det maps decide which (key, ratio) list this rank hands to the width collective, so the det
            # range guard is settled BEFORE the recogniser stage - an overflowed map must neither feed the peers' widths nor make this rank
            # repeat a collective its peers make once (without the exchange the deferred check of _run_batch_guarded is enough)
            if self.det.check_range_and_fallback():
                self.stats["range_fallbacks"] = self.stats.get("range_fallbacks", 0) + 1
                h = self._front(pages, P)             # det (and layout) again, the det engine now on fp32 MFMA
                self.stats["front_prefetched"] = 0.0
                cur.wait_event(h["det_done"])
        prob_maps, det_hw = h["prob_maps"], h["det_hw"]
        self.last_det = (prob_maps, det_hw)         # a VIEW of the engine's output buffer: valid until the next det forward of this shape
        if quads_per_page is None:
            src = det_maps_override if det_maps_override is not None else prob_maps
            quads_per_page = self.boxes_from_maps_device(src.contiguous(), (H, W)) if self.device_db else self._boxes_via_host_maps(src, (H, W))
        if prefetch is not None:
            front_next = self._front_next_hook(prefetch)
            self._after_rec_enqueue = front_next
        try:
            keys = getattr(self, "_page_keys", None)
            texts = self.rec_forward_sources([(pages, quads_per_page)], image_keys=None if keys is None else [keys])[0]
        except BaseException:
            self._after_rec_enqueue = None             # a failed batch must not leave its hook to the next one
            raise
        if self._after_rec_enqueue is not None:        # no line to recognise: the hook was not reached
            self._after_rec_enqueue = None
            front_next(())
        if h["layout_done"] is not None:
            cur.wait_event(h["layout_done"])
        for i in range(P):
            qs = np.asarray(quads_per_page[i], dtype=np.float32).reshape(-1, 4, 2)
            results[i].lines = [(qs[j], t, s) for j, (t, s) in enumerate(texts[i])]
            if h["feats"] is not None:
                results[i].layout_feats = h["feats"][i]
            if self.use_cls and self.last_cls is not None:
                results[i].cls = list(self.last_cls[0][i])
        return results


    def _front_next_hook(self, prefetch):
        """The hook that enqueues the NEXT batch's det and layout forwards: for a [P,H,W,3] tensor or a list of device pages."""
        if isinstance(prefetch, (list, tuple)):
            kind, nxt = split_page_list(prefetch)
            if kind != "device":
                raise ValueError("prefetch takes device pages: upload a list of host pages first (PageUploader.submit)")

            def front_next(gate):
                self._prefetched = self._front_list(nxt, gate)
        else:
            assert prefetch.is_cuda and prefetch.dtype == torch.uint8 and prefetch.dim() == 4

            def front_next(gate):
                self._prefetched = self._front(prefetch, prefetch.shape[0], gate)
        return front_next

    # ---------------------------------------------------------------- whole batch, pages of different sizes
    @staticmethod
    def _front_key_list(pages: Sequence[torch.Tensor]) -> tuple:
        return tuple((p.data_ptr(), tuple(p.shape)) for p in pages)

    def _run_batch_list(self, pages, quads_per_page, det_maps_override, prefetch, page_keys) -> List[PageResult]:
        """`run_batch` for a sequence of pages: the upload of host pages (one pack, one copy), then `_run_list_once` under the same range
        guard as `_run_batch_guarded`."""
        kind, pages = split_page_list(pages)
        if kind == "host":
            if getattr(self, "_page_stage", None) is None:
                self._page_stage = HostImageStage(self.tdev)
            pages = self._page_stage.upload(pages).views
        P = len(pages)
        self._page_keys = None if page_keys is None else [int(k) for k in page_keys]
        if self._page_keys is not None and len(self._page_keys) != P:
            raise ValueError("page_keys: one key per page")
        if quads_per_page is not None and len(quads_per_page) != P:
            raise ValueError("quads_per_page: one array of quads per page")
        if det_maps_override is not None and len(det_maps_override) != P:
            raise ValueError("det_maps_override: for a list of pages, one [1, 1, dh, dw] map per page")
        if self.rec_width_sync is not None and page_keys is None and getattr(self.rec_width_sync, "world_size", 1) > 1:
            raise ValueError("rec_width_sync over more than one rank needs page_keys: the pages' positions in the GLOBAL page list")
        self._width_sync_epoch += 1
        self._in_run_batch = True
        try:
            results = self._run_list_once(pages, quads_per_page, det_maps_override, prefetch)
            engines = [self.det] + ([self.layout] if self.layout is not None else [])
            if os.environ.get("RD_DEV_SKIP_RANGE_CHECK") == "1":
                engines = []
            if any([e.check_range_and_fallback() for e in engines]):
                self.stats["range_fallbacks"] = self.stats.get("range_fallbacks", 0) + 1
                self._prefetched = None
                results = self._run_list_once(pages, quads_per_page, det_maps_override, prefetch)
            return results
        finally:
            self._in_run_batch = False
            if kind == "host":
                self._page_stage.release()          # everything that reads the uploaded pages has been enqueued

    def _front_list(self, pages: Sequence[torch.Tensor], gate: Sequence[torch.cuda.Event] = ()) -> dict:
        """`_front` for pages of different sizes: ONE rd_preproc_resize_norm_sources launch writes the det input of every group of pages
        that share a det shape (buffers per shape, so addresses repeat), then one det forward per group; behind them, on the layout
        stream, one launch brings all pages to 800 x 800 and ONE backbone forward runs over the whole batch."""
        cur = torch.cuda.current_stream()
        P = len(pages)
        hws = [(int(p.shape[0]), int(p.shape[1])) for p in pages]
        shapes, groups, _inverse = group_pages_by_det_shape(hws)
        h = {"key": self._front_key_list(pages), "feats": None, "layout_done": None, "groups": groups, "hws": hws, "preproc_launches": 1}
        self.front_stream.wait_stream(cur)
        for ev in gate:
            self.front_stream.wait_event(ev)
        with torch.cuda.stream(self.front_stream):
            xs = [self._buf(("det_x", dh, dw), len(m) * 3 * dh * dw).view(len(m), 3, dh, dw) for (dh, dw), m in groups]
            dst: List[Optional[torch.Tensor]] = [None] * P
            for x, (_shape, members) in zip(xs, groups):
                for j, i in enumerate(members):
                    dst[i] = x[j]
            preproc_resize_norm_sources(pages, shapes, mean=ocr_host.DET_MEAN, std=ocr_host.DET_STD, interp=1, swap_rb=True, out=dst)
            h["prob_maps"] = [self.det.det_forward(x) for x in xs]
            h["det_done"] = torch.cuda.Event()
            h["det_done"].record(self.front_stream)
        if self.layout is not None:
            self.layout_stream.wait_event(h["det_done"])
            with torch.cuda.stream(self.layout_stream):
                x = self._buf("layout_x", P * 3 * LAYOUT_SIZE * LAYOUT_SIZE).view(P, 3, LAYOUT_SIZE, LAYOUT_SIZE)
                preproc_resize_norm_sources(pages, [(LAYOUT_SIZE, LAYOUT_SIZE)] * P, interp=2, out=list(x))
                h["preproc_launches"] += 1
                feats = self.layout.backbone_forward(x)
                if self.keep_feats:
                    h["feats"] = [[f[i].clone() for f in feats] for i in range(P)]
                h["layout_done"] = torch.cuda.Event()
                h["layout_done"].record(self.layout_stream)
        return h

    def _boxes_device_sizes(self, maps_dev: torch.Tensor, page_hws: Sequence[Tuple[int, int]], box_thresh: float = 0.3,
                            unclip_ratio: float = 1.8) -> List[np.ndarray]:
        """`boxes_from_maps_device` for maps of one det shape whose pages differ in size: the post-process takes a size per image."""
        res = ocr_host.db_postprocess_device(maps_dev, list(page_hws), thresh=0.3, box_thresh=box_thresh, unclip_ratio=unclip_ratio,
                                             stats=self.stats, cache=self.db_ws, raw=self.host_native)
        if self.host_native:
            return ocr_host.order_merge_boxes_native(*res)
        out = []
        for boxes, _scores in res:
            if len(boxes) == 0:
                out.append(np.zeros((0, 4, 2), np.float32))
                continue
            b = ocr_host.merge_det_boxes(ocr_host.sorted_boxes(boxes.astype(np.float32)))
            out.append(np.asarray(b, dtype=np.float32).reshape(-1, 4, 2))
        return out

    def _run_list_once(self, pages: Sequence[torch.Tensor], quads_per_page, det_maps_override, prefetch) -> List[PageResult]:
        """`_run_batch_once` for device pages of different sizes; results in the caller's page order."""
        P = len(pages)
        results = [PageResult() for _ in range(P)]
        cur = torch.cuda.current_stream()
        h, self._prefetched = self._prefetched, None
        if h is None or h["key"] != self._front_key_list(pages):
            h = self._front_list(pages)
            self.stats["front_prefetched"] = 0.0
        else:
            self.stats["front_prefetched"] = 1.0
        cur.wait_event(h["det_done"])
        if self.rec_width_sync is not None and self.det.precision != "fp32" and os.environ.get("RD_DEV_SKIP_RANGE_CHECK") != "1":
            if self.det.check_range_and_fallback():       # settled before the recogniser stage, as in _run_batch_once
                self.stats["range_fallbacks"] = self.stats.get("range_fallbacks", 0) + 1
                h = self._front_list(pages)
                self.stats["front_prefetched"] = 0.0
                cur.wait_event(h["det_done"])
        groups, hws = h["groups"], h["hws"]
        self.last_det = [(maps, shape, list(members)) for maps, (shape, members) in zip(h["prob_maps"], groups)]
        self.stats["det_groups"] = len(groups)
        self.stats["preproc_launches"] = h["preproc_launches"]
        if quads_per_page is None:
            if not self.device_db:
                raise ValueError("a list of pages needs the device DB post-process (device_db=True)")
            quads_per_page = [None] * P
            for maps, ((dh, dw), members) in zip(h["prob_maps"], groups):
                src = maps
                if det_maps_override is not None:
                    for i in members:
                        if tuple(det_maps_override[i].shape) != (1, 1, dh, dw):
                            raise ValueError(f"det_maps_override[{i}] must be [1, 1, {dh}, {dw}], got {tuple(det_maps_override[i].shape)}")
                    src = torch.cat([det_maps_override[i] for i in members])
                for i, q in zip(members, self._boxes_device_sizes(src.contiguous(), [hws[i] for i in members])):
                    quads_per_page[i] = q
        if prefetch is not None:
            front_next = self._front_next_hook(prefetch)
            self._after_rec_enqueue = front_next
        try:
            keys = getattr(self, "_page_keys", None)
            texts = self._rec_forward_pages(pages, quads_per_page, list(range(P)) if keys is None else keys)
        except BaseException:
            self._after_rec_enqueue = None
            raise
        if self._after_rec_enqueue is not None:        # no line to recognise: the hook was not reached
            self._after_rec_enqueue = None
            front_next(())
        if h["layout_done"] is not None:
            cur.wait_event(h["layout_done"])
        for i in range(P):
            qs = np.asarray(quads_per_page[i], dtype=np.float32).reshape(-1, 4, 2)
            results[i].lines = [(qs[j], t, s) for j, (t, s) in enumerate(texts[i])]
            if h["feats"] is not None:
                results[i].layout_feats = h["feats"][i]
            if self.use_cls and self.last_cls is not None:
                results[i].cls = list(self.last_cls[i][0])
        return results

    def _rec_forward_pages(self, pages: Sequence[torch.Tensor], quads_per_page: Sequence[np.ndarray], keys: Sequence[int]):
        """`rec_forward_sources` with one source per page, every line pooled into ONE plan (pooling key = `keys[page]`), and every rec
        launch's lines warped by ONE rd_line_warp_sources launch: each line names its page.  -> per page [(text, score)].  Carries the
        range guard of rec_forward_sources."""
        self._sync_this_call = True
        if not self._in_run_batch:
            self._width_sync_epoch += 1
        out = self._rec_pages_once(pages, quads_per_page, keys)
        for _ in range(3):
            if not any([e.check_range_and_fallback() for e in self.rec_engines + [self.rec_tail] + self.cls_engines]):
                break
            self.stats["range_fallbacks"] = self.stats.get("range_fallbacks", 0) + 1
            out = self._rec_pages_once(pages, quads_per_page, keys)
        return out

    def _rec_pages_once(self, pages, quads_per_page, keys):
        t0 = time.perf_counter()
        self.last_cls = None
        self.stats["warp_source_launches"] = 0
        strict = self.rec_mode == "strict"
        sync = None
        if self.rec_width_sync is not None and strict and self.rec_two_stage and self._sync_this_call:
            sync = lambda k, ratios: self._synced_widths(self.rec_width_sync, k, ratios)      # noqa: E731
        plan = plan_rec([(1, [q]) for q in quads_per_page], [[int(k)] for k in keys], **self._plan_modes(strict), width_sync=sync)
        scratch = None
        if plan.n:
            lines_name_their_sources(plan, [resize_source_view(p) for p in pages], [(int(p.shape[0]), int(p.shape[1])) for p in pages])
            if getattr(self, "_crop_scratch", None) is None or self._crop_scratch.numel() < plan.src_scratch_bytes:
                self._crop_scratch = torch.empty(int(plan.src_scratch_bytes * 1.25) + 1024, dtype=torch.uint8, device=self.tdev)
            scratch = self._crop_scratch.data_ptr()
        per_source = self._run_rec_plan(plan, None, False, t0, scratch=scratch)
        return [s[0] for s in per_source]


def lines_name_their_sources(plan: RecPlan, views: Sequence[Tuple[int, int]], hws: Sequence[Tuple[int, int]]) -> None:
    """Host only: turns a `plan_rec` plan over one-image sources of different sizes into one whose lines name their source
    (LINE_SOURCE_DTYPE), so that ONE rd_line_warp_sources launch per rec launch replaces a rd_line_warp_batch launch per source.
    `views[s]` = (device address, row pitch) and `hws[s]` = (H, W) of source s.  The crops keep their places: a launch's region of the
    scratch starts where it did, the offsets become offsets from the buffer's start (as in rec_forward_crops)."""
    starts, total = plan.starts, int(plan.batch_base[-1])
    if total >= 2 ** 31:
        raise RuntimeError("the crops of one call must lie inside 2 GB (scratch_off is an int32): split the page list")
    base_of = np.repeat(np.asarray(plan.batch_base[:-1], dtype=np.int64), np.diff(starts))
    plan.descs["scratch_off"] = (plan.descs["scratch_off"].astype(np.int64) + base_of).astype(np.int32)
    if plan.descs_cls is not None:
        plan.descs_cls["scratch_off"] = plan.descs["scratch_off"]
    src = plan.src_of[plan.line_ids]                          # source of every line, in launch order
    sd = np.zeros(plan.n, LINE_SOURCE_DTYPE)
    sd["src"] = np.asarray([v[0] for v in views], dtype=np.uint64)[src]
    sd["pitch"] = np.asarray([v[1] for v in views], dtype=np.int64)[src]
    sd["H"] = np.asarray([hw[0] for hw in hws], dtype=np.int32)[src]
    sd["W"] = np.asarray([hw[1] for hw in hws], dtype=np.int32)[src]
    for f in ("crop_w", "crop_h", "scratch_off", "m"):
        sd[f] = plan.descs[f]
    plan.src_descs = sd
    plan.src_jobs = [(int(a), int(e - a)) for a, e in zip(starts[:-1], starts[1:])]
    plan.src_scratch_bytes = total
    plan.warp_jobs = [[] for _ in plan.batches]
    plan.descs_warp = None
    plan.batch_base = np.zeros(len(plan.batches) + 1, np.int64)


def render_text_maps(boxes_per_page: Sequence[np.ndarray], page_hw: Tuple[int, int], map_hw: Tuple[int, int],
                     device) -> torch.Tensor:
    """Synthetic DB probability maps for pages whose text-line boxes are known (benchmark helper): 0.9 inside every
    line box shrunk by 0.32 x its height on every side (so that the post-process' unclip, ratio 1.8, grows the region
    back to about the original box), 0.02 elsewhere.  Used because random-weight det maps carry no text to find."""
    H, W = page_hw
    h, w = map_hw
    maps = torch.full((len(boxes_per_page), 1, h, w), 0.02, dtype=torch.float32)
    for i, boxes in enumerate(boxes_per_page):
        for x0, y0, x1, y1 in np.asarray(boxes, dtype=np.float64).reshape(-1, 4):
            bw, bh = x1 - x0, y1 - y0
            d = 0.32 * min(bw, bh)
            xa, xb = int(round((x0 + d) * w / W)), int(round((x1 - d) * w / W))
            ya, yb = int(round((y0 + d) * h / H)), int(round((y1 - d) * h / H))
            if xb > xa and yb > ya:
                maps[i, 0, ya:yb, xa:xb] = 0.9
    return maps.to(device)


class PageUploader:
    """Host -> device upload of a STREAM of page batches.  The reference hands host arrays to every batch
    (`np.array(image)` per page, batch_analyze.py:108-111); on the GPU the 6 MB a page weighs (192 MB per 32-page batch, ~4 ms of
    PCIe) must not sit in front of the networks, so: `n_buffers` device buffers, the copy of batch i + 1 enqueued on a copy stream of
    its own while batch i computes, and an event per batch that the consumer's stream waits on.

        up = PageUploader(device)
        nxt = up.submit(first_batch)                    # numpy [P,H,W,3] u8 or a CPU tensor (pinned: truly asynchronous)
        for batch in rest:
            cur, nxt = nxt, up.submit(batch)            # batch i + 1 travels under batch i's kernels
            results = pipe.run_batch(up.wait(cur))      # the current stream waits for ITS pages only
            up.release(cur)                             # everything that reads batch i is enqueued: its buffer may be recycled

    A buffer is re-used `n_buffers` submits later.  The copy that recycles it must run AFTER the last kernel that reads the old batch:
    `release(ticket)` records that point on the consumer's stream and the recycling `submit` makes the copy stream wait for it.  A
    ticket that was handed out by `wait` and never released is still safe as long as its consumers were ENQUEUED before the
    recycling submit: `submit` then waits for everything enqueued so far on the stream `wait` was called on (coarser than
    `release`: it also waits for later batches' work on that stream).  Pageable sources are staged through a pinned buffer of the
    uploader (one host memcpy); render into `pinned_like(...)` buffers to avoid it."""

    def __init__(self, device: int = 0, n_buffers: int = 2):
        self.tdev = torch.device("cuda", device)
        self.stream = torch.cuda.Stream(device=self.tdev)
        self.n = max(2, n_buffers)
        self._dev: List[Optional[torch.Tensor]] = [None] * self.n
        self._pin: List[Optional[torch.Tensor]] = [None] * self.n
        self._released: List[Optional[torch.cuda.Event]] = [None] * self.n
        self._consumer: List[Optional[torch.cuda.Stream]] = [None] * self.n    # stream `wait` handed buffer k out on, until `release`
        self._i = 0
        self.bytes_uploaded = 0

    @staticmethod
    def pinned_like(shape) -> torch.Tensor:
        """A pinned uint8 host buffer to render pages into (its upload needs no staging copy)."""
        return torch.empty(tuple(shape), dtype=torch.uint8, pin_memory=True)

    @staticmethod
    def plan_list(shapes: Sequence[Tuple[int, int]]) -> Tuple[List[int], int]:
        """Where the [h, w, 3] pages of a LIST lie in the upload: (byte offset per page, total bytes) - 16-byte aligned page starts, in
        order (host_stage.plan_offsets)."""
        return plan_offsets(shapes)

    def _submit_list(self, pages_host: Sequence) -> Tuple[List[torch.Tensor], torch.cuda.Event, int]:
        """`submit` for a list of host pages of different sizes: ONE pinned pack (rd_stage_pack) and ONE copy; the ticket's first entry is
        the list of device views, which `wait` returns."""
        kind, arrs = split_page_list(pages_host)
        if kind != "host":
            raise ValueError("PageUploader.submit takes host pages")
        shapes = [(int(a.shape[0]), int(a.shape[1])) for a in arrs]
        offsets, total = self.plan_list(shapes)
        k = self._i % self.n
        self._i += 1
        if self._dev[k] is None or self._dev[k].numel() < total:
            self._dev[k] = torch.empty(int(total * 1.1) + 256, dtype=torch.uint8, device=self.tdev)
        if self._consumer[k] is not None:
            rel = torch.cuda.Event()
            rel.record(self._consumer[k])
            self._released[k], self._consumer[k] = rel, None
        if self._released[k] is not None:
            self.stream.wait_event(self._released[k])
        if self._pin[k] is None or self._pin[k].numel() < total:
            self._pin[k] = torch.empty(int(total * 1.1) + 256, dtype=torch.uint8, pin_memory=True)
        self.stream.synchronize()                                  # the staging buffer's previous copy has left the host
        pack_images(arrs, offsets, self._pin[k].data_ptr(), total)
        with torch.cuda.stream(self.stream):
            self._dev[k][:total].copy_(self._pin[k][:total], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.bytes_uploaded += total
        views = [self._dev[k][o: o + 3 * h * w].view(h, w, 3) for o, (h, w) in zip(offsets, shapes)]
        return views, ev, k

    def submit(self, pages_host) -> Tuple[torch.Tensor, torch.cuda.Event, int]:
        if isinstance(pages_host, (list, tuple)):
            return self._submit_list(pages_host)
        src = torch.from_numpy(pages_host) if isinstance(pages_host, np.ndarray) else pages_host
        assert not src.is_cuda and src.dtype == torch.uint8 and src.dim() == 4 and src.is_contiguous()
        k = self._i % self.n
        self._i += 1
        if self._dev[k] is None or self._dev[k].numel() < src.numel():
            self._dev[k] = torch.empty(int(src.numel() * 1.1) + 256, dtype=torch.uint8, device=self.tdev)
        dst = self._dev[k][: src.numel()].view(src.shape)
        if self._consumer[k] is not None:                          # handed out and never released: wait for all of that stream's work so far
            rel = torch.cuda.Event()
            rel.record(self._consumer[k])
            self._released[k], self._consumer[k] = rel, None
        if self._released[k] is not None:
            self.stream.wait_event(self._released[k])              # the batch that used this buffer has been consumed (enqueued work done)
        if not src.is_pinned():
            if self._pin[k] is None or self._pin[k].numel() < src.numel():
                self._pin[k] = torch.empty(int(src.numel() * 1.1) + 256, dtype=torch.uint8, pin_memory=True)
            self.stream.synchronize()                              # the staging buffer's previous copy has left the host
            stage = self._pin[k][: src.numel()].view(src.shape)
            stage.copy_(src)
            src = stage
        with torch.cuda.stream(self.stream):
            dst.copy_(src, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.bytes_uploaded += src.numel()
        return dst, ev, k

    def wait(self, ticket: Tuple[torch.Tensor, torch.cuda.Event, int]) -> torch.Tensor:
        """The device tensor of a submitted batch, valid on the CURRENT stream from here on."""
        dst, ev, k = ticket
        cur = torch.cuda.current_stream()
        cur.wait_event(ev)
        self._consumer[k] = cur
        return dst

    def release(self, ticket) -> None:
        """Call after the work that reads the batch has been enqueued on the current stream: its buffer may be recycled once that
        work is done."""
        _dst, _ev, k = ticket
        rel = torch.cuda.Event()
        rel.record(torch.cuda.current_stream())
        self._released[k], self._consumer[k] = rel, None


class PagePipelinePool:
    """`workers` PagePipelines on one GPU, each fed a contiguous shard of the page batch from its own host thread and HIP
    streams.  A page batch has host stages between its GPU stages (det maps -> DB post-process -> crop descriptors;
    rec indices -> CTC decode): with two shards in flight the GPU runs one shard's networks while the host works on the
    other's.  Results come back in page order, identical to a single pipeline's (pages are independent)."""

    def __init__(self, states: Dict[str, object], device: int = 0, workers: int = 2, **kw):
        self.device = device
        self.pipes = [PagePipeline(states, device, **kw) for _ in range(max(1, workers))]
        self.streams = [torch.cuda.Stream(device=self.pipes[0].tdev) for _ in self.pipes]
        self.pool = ThreadPoolExecutor(max_workers=len(self.pipes))
        self.stats: Dict[str, float] = {}

    @property
    def engines(self) -> List[RdEngine]:
        out = []
        for p in self.pipes:
            out += [p.det, *([p.layout] if p.layout is not None else []), *p.rec_engines, p.rec_tail]
        return out

    def run_batch(self, pages: torch.Tensor, quads_per_page: Optional[Sequence[np.ndarray]] = None,
                  det_maps_override: Optional[torch.Tensor] = None, prefetch: Optional[torch.Tensor] = None,
                  page_keys: Optional[Sequence[int]] = None) -> List[PageResult]:
        """`prefetch`: the next batch's device pages (PagePipeline.run_batch) - every shard's pipeline enqueues its shard of them.
        `page_keys`: PagePipeline.run_batch (global page indices of a page-sharded run; one worker only: the width collective is
        made once per batch by one pipeline)."""
        assert page_keys is None or len(self.pipes) == 1 or all(p.rec_width_sync is None for p in self.pipes)
        if isinstance(pages, np.ndarray) or not pages.is_cuda:      # host pages: one upload for all shards (see PagePipeline.run_batch)
            src = torch.from_numpy(np.ascontiguousarray(pages)) if isinstance(pages, np.ndarray) else pages.contiguous()
            pages = src.to(self.pipes[0].tdev, non_blocking=src.is_pinned())
        P = pages.shape[0]
        n = min(len(self.pipes), max(1, P))
        bounds = [P * k // n for k in range(n + 1)]
        nb = None
        if prefetch is not None and min(len(self.pipes), max(1, prefetch.shape[0])) == n:     # the next call will shard it the same way
            nb = [prefetch.shape[0] * k // n for k in range(n + 1)]
        ready = torch.cuda.Event()
        ready.record()

        def work(k: int):
            lo, hi = bounds[k], bounds[k + 1]
            torch.cuda.set_device(self.device)
            st = self.streams[k]
            with torch.cuda.stream(st):
                st.wait_event(ready)
                res = self.pipes[k].run_batch(pages[lo:hi], None if quads_per_page is None else quads_per_page[lo:hi],
                                              None if det_maps_override is None else det_maps_override[lo:hi],
                                              None if nb is None else prefetch[nb[k]:nb[k + 1]],
                                              None if page_keys is None else page_keys[lo:hi])
                done = torch.cuda.Event()
                done.record(st)
            return res, done

        outs = list(self.pool.map(work, range(n)))
        results: List[PageResult] = []
        for res, done in outs:
            torch.cuda.current_stream().wait_event(done)
            results += res
        self.stats = {}
        for k, p in enumerate(self.pipes[:n]):
            for key, v in p.stats.items():
                self.stats[key] = self.stats.get(key, 0.0) + v
        return results

