"""The reference's OCR-MODEL seam: the one object per language an unmodified RapidDoc gets from `ocr_model_init()`
(rapid_doc/backend/pipeline/model_init.py:45-54, through `AtomModelSingleton.get_atom_model(OCR, ...)`) and drives with five call forms:

    det_batch_predict(img_list, max_batch_size)                      analyze_utils.py:191      same-size white-padded BGR canvases
    ocr(img_crop_list, det=False)[0]                                 analyze_utils.py:253,260  EVERY line crop of the page batch, one call
    ocr(img, mfd_res=..., rec=False)[0]                              analyze_utils.py:344,367, rapid_table.py:133
    ocr(img, mfd_res=...)[0]                                         rapid_table.py:169
    ocr(crops, det=False, return_word_box=..., ori_img=, dt_boxes=)  analyze_utils.py:493-519  table OCR with word boxes

`Mi355RapidOcrModel` answers them on the engine.  Behind this seam RapidDoc's own driver keeps everything it does around the model - the
text-layer mode (`use_det_mode="auto"`), `merge_det_boxes` / `update_det_boxes`, the `LowScoreText` demotion, the table stage's OCR - and
the engine sees the whole pooled line list of a page batch, which is what `PagePipeline(rec_mode="strict")` needs to run the reference's
chunks of six inside GPU-sized launches.  `plugin.install_ocr_model` puts it in place of `ocr_model_init`.

`LazyLineCrop` (with `install_ocr_model(device_crops=True)`): what the replaced `get_rotate_crop_image` returns - the source image, the four
points and the crop's shape.  `ocr(list, det=False)` uploads every distinct source once and warps all lazy lines of a rec launch in ONE
`rd_line_warp_sources` launch; anything else that touches the object gets the exact eager array, made by the original function.

The module imports without RapidDoc and without cv2."""
from __future__ import annotations

import time
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import host_stage, ocr_host
from .rec_plan import LINE_SOURCE_DTYPE, quads_to_crop_matrices

DRIVER_KEYS = ("engine_type", "use_det_mode", "custom_model", "seal_enable")      # popped by the reference too (rapid_ocr.py:104-107)
# keys that choose WHICH network runs and where: here that is the pipeline's engines, so they cannot change a result
_MODEL_CHOICE = ("engine_type", "model_path", "model_dir", "ocr_version", "model_type", "lang_type", "task_type", "rec_keys_path", "rec_img_shape")
ROTATE_RATIO = 2.0        # get_rotate_crop_image: np.rot90 for crops with h / w >= 2 (utils/ocr_utils.py:534-536)
DET_LAUNCH = 32           # images of one size in one detector launch


def crop_shape(points) -> Tuple[int, int, int]:
    """(crop_w, crop_h, rot90) of `get_rotate_crop_image(img, points)` (utils/ocr_utils.py:516-536): the float32 edge norms truncated,
    and whether the crop is turned by np.rot90.  A side of 0 has no crop (cv2 raises on it): rot90 is 0 then."""
    q = np.asarray(points, dtype=np.float32).reshape(4, 2)
    d = [q[0] - q[1], q[2] - q[3], q[0] - q[3], q[1] - q[2]]
    n = [float(np.sqrt(v[0] * v[0] + v[1] * v[1])) for v in d]          # float32 products and sum, like np.linalg.norm on float32
    w, h = max(n[0], n[1]), max(n[2], n[3])
    w, h = (int(w) if np.isfinite(w) else 0), (int(h) if np.isfinite(h) else 0)
    return w, h, int(w >= 1 and h >= 1 and h * 1.0 / w >= ROTATE_RATIO)


class LazyLineCrop(np.lib.mixins.NDArrayOperatorsMixin):
    """A text-line crop that has not been cut yet: the source image, the four points, the crop's `shape` (the reference's own rule,
    its np.rot90 of tall crops included) - and the function that cuts it.  `Mi355RapidOcrModel.ocr(list, det=False)` reads the three
    and cuts the line on the device.  Everything else - `np.asarray`, indexing, arithmetic, any numpy function - first makes the eager
    array, ONCE, through the original `get_rotate_crop_image` captured at install time, and then behaves as that array.  An array-like,
    deliberately not an ndarray subclass (see session.LazySoftmax)."""

    __array_priority__ = 1000.0

    def __init__(self, source: np.ndarray, points, shape: Tuple[int, int, int], original):
        self.source, self.points, self.shape = source, np.array(points, dtype=np.float32).reshape(4, 2), tuple(int(v) for v in shape)
        self._original, self._host = original, None

    dtype = np.dtype(np.uint8)
    ndim = 3

    @property
    def materialized(self) -> bool:
        return self._host is not None

    def materialize(self) -> np.ndarray:
        if self._host is None:
            self._host = np.asarray(self._original(self.source, self.points.copy()))
        return self._host

    def __array__(self, dtype=None, copy=None):
        a = self.materialize()
        return a if dtype is None or np.dtype(dtype) == a.dtype else a.astype(dtype)

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        inputs = tuple(x.materialize() if isinstance(x, LazyLineCrop) else x for x in inputs)
        if "out" in kwargs:
            kwargs["out"] = tuple(x.materialize() if isinstance(x, LazyLineCrop) else x for x in kwargs["out"])
        return getattr(ufunc, method)(*inputs, **kwargs)

    def __array_function__(self, func, types, args, kwargs):
        def conv(v):
            if isinstance(v, LazyLineCrop):
                return v.materialize()
            if isinstance(v, (list, tuple)):
                return type(v)(conv(e) for e in v)
            return v
        return func(*conv(tuple(args)), **{k: conv(v) for k, v in kwargs.items()})

    def __getitem__(self, key):
        return self.materialize()[key]

    def __setitem__(self, key, value):
        self.materialize()[key] = value

    def __len__(self) -> int:
        return self.shape[0]

    def __iter__(self):
        return iter(self.materialize())

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self.materialize(), name)

    @property
    def size(self) -> int:
        return int(np.prod(self.shape))

    @property
    def nbytes(self) -> int:
        return self.size

    def __repr__(self) -> str:
        return "LazyLineCrop(shape=%s, %s)" % (self.shape, "materialized" if self.materialized else "not cut yet")


def lazy_crop_function(original):
    """The replacement of `get_rotate_crop_image(img, points)`: a `LazyLineCrop`, or - for what has no lazy form (an image that is not a
    uint8 [h, w, 3] array, points that are not 4 x 2, a crop side of 0: the reference's own call decides, and raises, there) - the
    original's answer."""
    def get_rotate_crop_image(img, points):
        try:
            pts = np.asarray(points, dtype=np.float32)
            lazy = isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.size and pts.shape == (4, 2)
            w, h, rot = crop_shape(pts) if lazy else (0, 0, 0)
        except (TypeError, ValueError):
            lazy = False
        if not lazy or w < 1 or h < 1:
            return original(img, points)
        return LazyLineCrop(img, pts, (w, h, 3) if rot else (h, w, 3), original)
    get_rotate_crop_image.rapiddoc_amd_original = original
    return get_rotate_crop_image


def normalize_image(img) -> np.ndarray:
    """`check_img` + `preprocess_image` (utils/ocr_utils.py:73-102) on the host: a grey image becomes three equal channels, a fourth
    channel is blended onto white with the reference's float arithmetic; the result is what `host_stage.as_stage_image` takes."""
    a = np.asarray(img)
    if a.ndim == 2:
        a = np.stack([a, a, a], axis=2)                                  # cv2.COLOR_GRAY2BGR
    if a.ndim == 3 and a.shape[2] == 4:
        alpha = a[:, :, 3] / 255
        a = np.stack([(255 * (1 - alpha) + a[:, :, c] * alpha).astype(np.uint8) for c in range(3)], axis=2)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"an OCR image must be [h, w], [h, w, 3] or [h, w, 4], got shape {a.shape}")
    return host_stage.as_stage_image(a)


def pack_line_sources(base: int, offsets: Sequence[int], shapes: Sequence[Tuple[int, int]], source_of: Sequence[int], mats: np.ndarray,
                      crop_w: Sequence[int], crop_h: Sequence[int], first_byte: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """Host only: one rd_line_source_desc per lazy line.  `base` / `offsets` / `shapes`: a `host_stage.Staged`'s; line k is cut from
    upload `source_of[k]` with the homography `mats[k]` into a crop_w[k] x crop_h[k] crop.  The crops lie one behind the other from byte
    `first_byte` (a multiple of 16) on, each at a multiple of 16; a crop without pixels takes no bytes.  -> (descriptors, their
    `scratch_off` as int64, the first byte behind the last crop)."""
    n = len(source_of)
    descs = np.zeros(n, dtype=LINE_SOURCE_DTYPE)
    sizes = [(int(h), int(w)) for w, h in zip(crop_w, crop_h)]
    rel, total = host_stage.plan_offsets(sizes)
    offs = np.asarray(rel, dtype=np.int64).reshape(n) + int(first_byte)
    for k, s in enumerate(source_of):
        h, w = shapes[s]
        descs[k] = (int(base) + int(offsets[s]), 3 * w, w, h, sizes[k][1], sizes[k][0], 0, 0, mats[k])
    descs["scratch_off"] = np.minimum(offs, 2 ** 31 - 1).astype(np.int32)      # (a call beyond the int32 range is refused by its caller)
    return descs, offs, int(first_byte) + int(total)


def check_ocr_config(ocr_config: Optional[dict], served: dict) -> dict:
    """The reference's `default_params.update(ocr_config)` for an engine whose networks are fixed: `served` with the values the
    configuration overrides.  Driver keys are ignored, as the reference pops them; keys that only choose a model file or a runtime are
    ignored (the pipeline's engines are the model); a key that names a served setting must be one this class can honour; any other
    key raises ValueError naming it."""
    out = dict(served)
    for key, value in (ocr_config or {}).items():
        if key in DRIVER_KEYS or key.startswith("EngineConfig.") or key in ("Global.model_root_dir", "Global.log_level"):
            continue
        if "." in key and key.split(".", 1)[1] in _MODEL_CHOICE:
            continue
        if key in ("Det.box_thresh", "Det.unclip_ratio"):
            out[key] = float(value)
            continue
        if key in served:
            same = list(value) == list(served[key]) if isinstance(served[key], (list, tuple)) else value == served[key]
            if same:
                continue
            raise ValueError(f"ocr_config[{key!r}] = {value!r} is not served by Mi355RapidOcrModel (it runs with {served[key]!r})")
        raise ValueError(f"ocr_config[{key!r}] is not served by Mi355RapidOcrModel")
    return out


class Mi355RapidOcrModel:
    """`rapid_doc.model.ocr.rapid_ocr.RapidOcrModel` on the engine: the reference's constructor arguments plus `pipeline` (a
    `PagePipeline`, or {language: PagePipeline} - `lang` picks one).  Defaults follow rapid_ocr.py:44-66: drop_score 0.5, detector limit
    960 / 'max', dilation on.  `is_seal=True` raises ValueError: the seal detector is a different network and polygon boxes are not
    served.  Word boxes need a strict two-stage pipeline (`rec_mode="strict"`), `use_cls` pipelines are refused.

    `det_maps_fn((h, w), (dh, dw), first, n) -> [n, 1, dh, dw] maps or None` (attribute, default None; `first`: the launch's first image
    in its size group): replaces the detector network's output as the post-process input - tests and benchmarks with random weights,
    whose maps carry no text (RegionOcr._detect_group)."""

    def __init__(self, pipeline, det_db_box_thresh=0.5, lang=None, ocr_config=None, use_dilation=True, det_db_unclip_ratio=1.8,
                 enable_merge_det_boxes=True, is_seal=False):
        if is_seal:
            raise ValueError("Mi355RapidOcrModel: is_seal=True is not served (the seal detector is a network of its own and its boxes are "
                             "polygons); plugin.install_ocr_model hands seal requests to the reference's own model")
        served = {"Global.use_cls": False, "Det.limit_side_len": 960, "Det.limit_type": "max", "Det.std": [0.229, 0.224, 0.225],
                  "Det.mean": [0.485, 0.456, 0.406], "Det.thresh": 0.3, "Det.box_thresh": float(det_db_box_thresh), "Det.use_dilation": bool(use_dilation),
                  "Det.unclip_ratio": float(det_db_unclip_ratio), "Det.box_type": "quad", "Det.score_mode": "fast", "Rec.rec_batch_num": 6}
        self.params = check_ocr_config(ocr_config, served)
        if not self.params["Det.use_dilation"]:
            raise ValueError("ocr_config['Det.use_dilation'] = False is not served by Mi355RapidOcrModel (the DB post-process dilates)")
        if isinstance(pipeline, dict):
            if lang not in pipeline:
                raise KeyError(f"no OCR pipeline for language {lang!r} (have {sorted(pipeline)})")
            pipeline = pipeline[lang]
        if getattr(pipeline, "use_cls", False):
            raise ValueError("Mi355RapidOcrModel: a use_cls pipeline is not served here (RapidDoc's driver never classifies, rapid_ocr.py:51)")
        self.pipe, self.lang = pipeline, lang
        self.drop_score = 0.5
        self.enable_merge_det_boxes, self.is_seal = bool(enable_merge_det_boxes), False
        self.rec_batch_num = 6
        self.box_thresh, self.unclip_ratio = self.params["Det.box_thresh"], self.params["Det.unclip_ratio"]
        self.det_maps_fn = None
        self._region = None
        self._stage = None
        self._scratch = None
        self.last_staged = None            # tests: the `Staged` of the last ocr(det=False) call and the indices of its uploads
        self.stats: dict = {}

    # ------------------------------------------------------------------------------------------------------------ helpers
    def _region_ocr(self):
        if self._region is None:
            from .analyze import RegionOcr
            self._region = RegionOcr(self.pipe, box_thresh=self.box_thresh, unclip_ratio=self.unclip_ratio)
        return self._region

    def _stage_for(self):
        if self._stage is None:
            self._stage = host_stage.HostImageStage(self.pipe.tdev)
        return self._stage

    def _own_scratch(self, nbytes: int) -> int:
        """device address of this model's own crop scratch of at least `nbytes` (grown geometrically, re-used call after call: every
        recogniser call ends with the current stream waiting for its launches)"""
        import torch
        if self._scratch is None or self._scratch.numel() < nbytes:
            self._scratch = torch.empty(max(int(nbytes), 2 * (self._scratch.numel() if self._scratch is not None else 0), 1 << 16),
                                        dtype=torch.uint8, device=self.pipe.tdev)
        return self._scratch.data_ptr()

    def _rgb_canvases(self, staged, groups) -> list:
        """per size group ((h, w), members) the device uint8 [len, h, w, 3] RGB array of the uploaded BGR images: ONE rd_stage_canvases
        launch for the groups whose width is a multiple of 4 (every 64-px canvas of the reference's driver), a channel flip of the
        uploaded bytes for the others"""
        import torch
        out = [None] * len(groups)
        fast = [g for g, ((_h, w), _m) in enumerate(groups) if w % 4 == 0]
        for g, canv in zip(fast, host_stage.stage_canvases(staged, [groups[g] for g in fast], swap_rb=True)):
            out[g] = canv
        for g, (_hw, members) in enumerate(groups):
            if out[g] is None:
                out[g] = torch.stack([staged.views[i].flip(-1) for i in members]).contiguous()
        return out

    def _detect(self, canvases) -> List[np.ndarray]:
        """the raw DB boxes of same-size RGB canvases [b, h, w, 3], in launches of at most DET_LAUNCH images"""
        region, out = self._region_ocr(), []
        b, h, w, _ = canvases.shape
        for lo in range(0, b, DET_LAUNCH):
            part = canvases[lo: lo + DET_LAUNCH]
            override = None
            if self.det_maps_fn is not None:
                override = self.det_maps_fn((h, w), ocr_host.det_resize_shape(h, w, 960, "max"), lo, int(part.shape[0]))
            out.extend(region._detect_group(part, override, self.pipe))
        return out

    # ------------------------------------------------------------------------------------------------------------ det_batch_predict
    def det_batch_predict(self, img_list, max_batch_size=8):
        """numpy BGR uint8 images -> per image (boxes, elapse): `boxes` = what RegionOcr's raw detection seam returns for that canvas
        (float32 [n, 4, 2] in DB post-process order), None when nothing was detected (rapidocr's value).  The images are uploaded by ONE
        copy and grouped by size; a size group runs in engine-sized launches whatever `max_batch_size` says - the engine is
        launch-invariant, so an image's result does not depend on it.  The reference's caller hands over one size per call: one launch."""
        if not img_list:
            return []
        t0 = time.time()
        imgs = [normalize_image(im) for im in img_list]
        by_size: dict = {}
        for i, im in enumerate(imgs):
            if im.shape[0] < 1 or im.shape[1] < 1:
                raise ValueError(f"det_batch_predict: image {i} has no pixels")
            by_size.setdefault((int(im.shape[0]), int(im.shape[1])), []).append(i)
        groups = list(by_size.items())
        stage = self._stage_for()
        staged = stage.upload(imgs)
        canvases = self._rgb_canvases(staged, groups)
        stage.release()
        boxes: list = [None] * len(imgs)
        for (_hw, members), canv in zip(groups, canvases):
            for i, raw in zip(members, self._detect(canv)):
                boxes[i] = raw if raw is not None and len(raw) else None
        elapse = (time.time() - t0) / len(imgs)
        return [(b, elapse) for b in boxes]

    # ------------------------------------------------------------------------------------------------------------ ocr
    def ocr(self, img, det=True, rec=True, mfd_res=None, tqdm_enable=False, tqdm_desc="OCR-rec Predict", return_word_box=False,
            ori_img=None, dt_boxes=None):
        """The reference's `ocr` (rapid_ocr.py:225-299), with its return nesting: a one-element list."""
        if isinstance(img, list) and det:
            raise ValueError("When input a list of images, det must be false")      # (the reference logs this and exits the process)
        if det:
            boxes, lines = self._det_rec(normalize_image(img), mfd_res, rec)
            if boxes is None:
                return [None]
            if not rec:
                return [[b.tolist() for b in boxes]]
            if not boxes and not lines:
                return [None]
            return [[[b.tolist(), res] for b, res in zip(boxes, lines)]]
        if not rec:
            return None                                                              # (the reference falls through its three branches)
        crops = img if isinstance(img, list) else [img]
        want_words = bool(return_word_box and ori_img is not None and dt_boxes is not None and len(dt_boxes))
        raw = self._recognise(crops, want_words)
        if want_words:
            from . import word_boxes as WB
            quads = [np.array(b, dtype=np.float32) for b in dt_boxes]
            lines = WB.lines_with_words(raw, quads)
            raw_h, raw_w = ori_img.shape[:2]
            origin = WB.calc_word_boxes([wl for _t, _s, wl in lines], raw_h, raw_w)
            return [list(zip([t for t, _s, _w in lines], [s for _t, s, _w in lines], origin))]      # rapid_ocr.py:295 - zip, as it is
        return [[(t, s) for t, s in raw]]

    def __call__(self, img, mfd_res=None):
        """rapid_ocr.py:351-401: (boxes, [(text, score)]) of the lines at or above drop_score, (None, None) without an image or a box"""
        if img is None:
            return None, None
        boxes, lines = self._det_rec(normalize_image(img), mfd_res, True)
        return (None, None) if boxes is None else (boxes, lines)

    def _det_rec(self, img: np.ndarray, mfd_res, rec: bool):
        """one BGR image -> (boxes after sort / merge / formula cut, [(text, score)] after the drop_score filter or None); (None, None)
        when the detector finds nothing"""
        h, w = int(img.shape[0]), int(img.shape[1])
        if h < 1 or w < 1:
            return None, None
        stage = self._stage_for()
        staged = stage.upload([img])
        try:
            raw = self._detect(self._rgb_canvases(staged, [((h, w), [0])])[0])[0]
            if raw is None or len(raw) == 0:
                return None, None
            boxes = list(ocr_host.sorted_boxes(np.asarray(raw, dtype=np.float32)))
            if self.enable_merge_det_boxes:
                boxes = ocr_host.merge_det_boxes(boxes)
            if mfd_res:
                boxes = ocr_host.update_det_boxes(boxes, mfd_res)
            boxes = [np.asarray(b, dtype=np.float32).reshape(4, 2) for b in boxes]
            if not rec:
                return boxes, None
            # the lines are cut from the uploaded image itself: every box a lazy line of source 0, warped into the model's own scratch
            res = self._recognise_staged(staged, 16 * ((3 * h * w + 15) // 16), [], [(0, b) for b in boxes], None, False) if boxes else []
        finally:
            stage.release()
        keep = [i for i, (_t, s) in enumerate(res) if s >= self.drop_score]
        return [boxes[i] for i in keep], [res[i] for i in keep]

    def _recognise(self, crops: Sequence, want_words: bool) -> list:
        """`ocr(list, det=False)`: eager arrays and LazyLineCrops in any mix, ONE upload (every eager crop, every distinct source of a
        lazy crop once - keyed by object identity: get_ocr_result_list copies the region image once per region, so all lines of a region
        share a source), ONE pooled recogniser call."""
        if not crops:
            return []
        uploads, eager, lazy, slot = [], [], [], [None] * len(crops)
        source_index: dict = {}
        for i, c in enumerate(crops):
            if isinstance(c, LazyLineCrop) and not c.materialized:
                continue
            a = normalize_image(c.materialize() if isinstance(c, LazyLineCrop) else c)
            slot[i] = ("e", len(eager))
            eager.append(len(uploads))
            uploads.append(a)
        for i, c in enumerate(crops):
            if slot[i] is None:
                s = source_index.get(id(c.source))
                if s is None:
                    s = source_index[id(c.source)] = len(uploads)
                    uploads.append(host_stage.as_stage_image(c.source))
                slot[i] = ("l", len(lazy))
                lazy.append((s, c.points))
        stage = self._stage_for()
        shapes = [(int(a.shape[0]), int(a.shape[1])) for a in uploads]
        _offs, total = host_stage.plan_offsets(shapes)
        # room behind the uploads for the warped lines, when there are crops to read in place next to them (else: the model's own scratch)
        tail = sum(16 * ((3 * w * h + 15) // 16) for w, h, _r in (crop_shape(p) for _s, p in lazy)) if eager else 0
        staged = stage.upload(uploads, tail_bytes=tail)
        self.last_staged = (staged, dict(eager=list(eager), sources=sorted(source_index.values())))
        try:
            return self._recognise_staged(staged, total, eager, lazy, slot, want_words)
        finally:
            stage.release()

    def _recognise_staged(self, staged, total: int, eager: Sequence[int], lazy: Sequence[tuple], slot: Optional[Sequence], want_words: bool) -> list:
        """the pooled recogniser call on an upload of `total` bytes: `eager[k]` = the upload that IS line k's crop, `lazy[k]` = (upload,
        points) of a line still to be cut, `slot[i]` = ("e" | "l", k) of the caller's line i (None: the eager lines, then the lazy ones)"""
        n_e, n_l = len(eager), len(lazy)
        cw = np.zeros(n_e + n_l, np.int64)
        ch = np.zeros(n_e + n_l, np.int64)
        rot = np.zeros(n_e + n_l, np.int32)
        ok = np.ones(n_e + n_l, bool)
        offs = np.zeros(n_e + n_l, np.int64)
        for k, u in enumerate(eager):            # an uploaded crop is the scratch layout already: packed [h][w][3], no rotation, BGR
            h, w = staged.shapes[u]
            cw[k], ch[k], offs[k], ok[k] = max(w, 1), max(h, 1), staged.offsets[u], h > 0 and w > 0
        src_descs = None
        scratch, end = staged.base, total
        if n_l:
            mats, lw, lh, lok = quads_to_crop_matrices(np.stack([np.asarray(p, dtype=np.float32).reshape(4, 2) for _s, p in lazy]))
            # where the warped lines go: behind the uploads, in the room `upload(tail_bytes=)` kept (their offsets and the eager crops'
            # count from one base) - or, when no line is read in place, into a buffer of this model's own
            descs, loffs, end = pack_line_sources(staged.base, staged.offsets, staged.shapes, [s for s, _p in lazy], mats, lw.astype(np.int64),
                                                  lh.astype(np.int64), total if n_e else 0)
            if not n_e:
                scratch = self._own_scratch(end)
            elif end > self._stage_for()._dev.numel():
                raise RuntimeError(f"the staged upload has no room for the warped lines ({end} > {self._stage_for()._dev.numel()} bytes)")
            cw[n_e:], ch[n_e:], ok[n_e:], offs[n_e:] = lw, lh, lok, loffs
            rot[n_e:] = (lh / lw >= ROTATE_RATIO).astype(np.int32)
            src_descs = np.zeros(n_e + n_l, dtype=LINE_SOURCE_DTYPE)
            src_descs[n_e:] = descs
        if end >= 2 ** 31:
            raise RuntimeError(f"ocr(det=False): the crops of one call take {end} bytes on the device; the limit is 2 GB (int32 offsets) - "
                               "hand the list over in parts")
        sel = np.asarray([(k if kind == "e" else n_e + k) for kind, k in slot] if slot is not None else range(n_e + n_l), dtype=np.int64)
        before = self.pipe.stats.get("warp_source_launches", 0)
        out = self.pipe.rec_forward_crops(cw[sel], ch[sel], rot[sel], ok[sel], offs[sel], scratch, end,
                                          src_descs[sel] if src_descs is not None else None, want_words=want_words)
        self.stats["warp_source_launches"] = self.pipe.stats.get("warp_source_launches", 0) - before
        self.stats["rec_batches"] = self.pipe.stats.get("rec_batches", 0)
        return out
