"""Host side of the formula stage (PP-FormulaNet_plus): image pre-processing and the batch_predict-shaped driver.

Reference: rapid_doc/model/formula/rapid_formula_self/model_handler/pp_formulanet_plus/pre_process.py:12-256
  UniMERNetImgDecode  crop the margin (normalised grey < 200), PIL bilinear resize so the short side is 384, thumbnail to
                      fit 384x384, centre-pad with 0                              (:39-163)
  UniMERNetTestTransform  (x/255 - 0.7931) / 0.1738, grey = .299 R + .587 G + .114 B of the *RGB-ordered* array read as BGR
                          by cv2.cvtColor(COLOR_BGR2GRAY), i.e. .114 c0 + .587 c1 + .299 c2      (:188-208)
  LatexImageFormat    pad to a multiple of 16 with 1, keep one channel -> [1,1,H,W]                (:229-246)
PIL does the resampling exactly like the reference (PIL is what the reference calls); the three cv2 calls
(findNonZero, boundingRect, cvtColor) are restated in numpy - cv2 is not installed here, so those are parity-unpinned.
The driver mirrors RapidFormulaModel.batch_predict (rapid_formula_model.py:34-41 -> rapid_formula_self/main.py:28-41):
chunks of `batch_size`, one [B,1,384,384] tensor per chunk -> encoder -> greedy decoder -> token ids.
"""
from __future__ import annotations

import math
import os
from typing import Callable, List, Optional, Sequence

import numpy as np
from PIL import Image, ImageOps

INPUT_SIZE = (384, 384)
MEAN, STD = 0.7931, 0.1738
# RD_FORMULA_PREPROC (read once): "host" = every crop is pre-processed on the host with Pillow, device tensors are copied first (the path
# before the device pre-process, kept for A/B); "device" = device tensors take `engine.formula_preprocess`; unset = DEVICE_BY_DEFAULT.
PREPROC_SWITCH = os.environ.get("RD_FORMULA_PREPROC", "").strip().lower()
DEVICE_BY_DEFAULT = True


def device_preproc_enabled() -> bool:
    """whether device tensors handed to `FormulaRecognizer.batch_predict` stay on the device (and `analyze.recognise_formulas` hands
    device views over at all)"""
    if PREPROC_SWITCH in ("host", "device"):
        return PREPROC_SWITCH == "device"
    return DEVICE_BY_DEFAULT


def _crop_margin(img: Image.Image) -> Image.Image:
    data = np.array(img.convert("L")).astype(np.uint8)
    mx, mn = data.max(), data.min()
    if mx == mn:
        return img
    norm = (data - mn) / (mx - mn) * 255
    ys, xs = np.nonzero(norm < 200)
    if len(xs) == 0:      # cv2.boundingRect(None) -> (0, 0, 0, 0): an empty crop, which the caller treats as failure
        return img.crop((0, 0, 0, 0))
    a, b = int(xs.min()), int(ys.min())
    return img.crop((a, b, int(xs.max()) + 1, int(ys.max()) + 1))


def decode_image(img: np.ndarray, input_size=INPUT_SIZE) -> Optional[np.ndarray]:
    """UniMERNetImgDecode.img_decode: uint8 HxWx3 (or HxW) -> uint8 384x384x3, or None for an empty image."""
    pil = _crop_margin(Image.fromarray(img).convert("RGB"))
    if pil.height == 0 or pil.width == 0:
        return None
    w, h = pil.size
    short, long_ = (w, h) if w <= h else (h, w)
    new_short = min(input_size)
    new_long = int(new_short * long_ / short)
    new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
    pil = pil.resize((new_w, new_h), resample=2)            # PIL bilinear
    pil.thumbnail((input_size[1], input_size[0]))
    dw, dh = input_size[1] - pil.width, input_size[0] - pil.height
    pw, ph = dw // 2, dh // 2
    return np.array(ImageOps.expand(pil, (pw, ph, dw - pw, dh - ph)))


def to_network_input(img384: np.ndarray) -> np.ndarray:
    """UniMERNetTestTransform + LatexImageFormat: uint8 HxWx3 -> float32 [1,1,H16,W16]."""
    x = (img384.astype("float32") * float(1 / 255.0) - np.float32(MEAN)) / np.float32(STD)
    grey = (np.float32(0.114) * x[..., 0] + np.float32(0.587) * x[..., 1] + np.float32(0.299) * x[..., 2]).astype(np.float32)
    h, w = grey.shape
    H, W_ = math.ceil(h / 16) * 16, math.ceil(w / 16) * 16
    grey = np.pad(grey, ((0, H - h), (0, W_ - w)), constant_values=(1, 1))
    return grey[None, None]


def preprocess(imgs: Sequence[np.ndarray]) -> List[Optional[np.ndarray]]:
    out = []
    for im in imgs:
        d = decode_image(im)
        out.append(None if d is None else to_network_input(d))
    return out


def make_token_decoder(tokenizer_json, fix_text="auto") -> Callable[[List[int]], str]:
    """ids -> LaTeX string exactly as UniMERNetDecode.token2str produces it after its EOS cut
    (pp_formulanet_plus/post_process.py:92-94 builds `tokenizers.Tokenizer.from_buffer(fast_tokenizer_file JSON)`, :277-296
    `tokenizer.decode(ids, skip_special_tokens=True)`, :350-381 LaTeX fix-ups then `ftfy.fix_text`).

    tokenizer_json: path to / str of / dict of the `fast_tokenizer_file` JSON the reference downloads with the model
    (`PP-FormulaNet_plus-M_inference.yml` -> PostProcess.character_dict).  fix_text: a callable, None, or "auto" =
    `ftfy.fix_text` when that package is importable (it is not part of this container; the reference imports it lazily)."""
    import json
    import os
    from tokenizers import Tokenizer
    from .latex_post import latex_postprocess
    if isinstance(tokenizer_json, dict):
        tok = Tokenizer.from_str(json.dumps(tokenizer_json))
    elif isinstance(tokenizer_json, (str, os.PathLike)) and os.path.exists(str(tokenizer_json)):
        tok = Tokenizer.from_file(str(tokenizer_json))
    else:
        tok = Tokenizer.from_str(str(tokenizer_json))
    if fix_text == "auto":
        try:
            from ftfy import fix_text as _ft   # noqa: WPS433
            fix_text = _ft
        except ImportError:
            fix_text = None

    def decode(ids: List[int]) -> str:
        text = latex_postprocess(tok.decode([int(i) for i in ids], skip_special_tokens=True))
        return fix_text(text) if fix_text else text
    return decode


class FormulaRecognizer:
    """`batch_predict(image_list, batch_size) -> list[str]` like rapid_doc.model.custom.CustomBaseModel / RapidFormulaModel
    when a tokenizer is given (`tokenizer_json=`, see `make_token_decoder`).

    Returns one entry per input image: the decoded string when `token_decoder` (ids -> str, e.g. the reference's
    UniMERNetDecode.token2str with its downloaded tokenizer) is given, otherwise the list of generated token ids with the
    start token, everything from EOS on, and padding removed.  Alternatively pass `bpe_decode` (ids -> raw string: only the
    tokenizer, whose JSON the reference downloads) and, optionally, `fix_text` (ftfy's): the LaTeX fix-ups in between are
    this package's own (`rapiddoc_amd.latex_post`, pinned to the reference's)."""

    def __init__(self, weights, device: int = 0, max_new_tokens: Optional[int] = None,
                 token_decoder: Optional[Callable[[List[int]], str]] = None,
                 bpe_decode: Optional[Callable[[List[int]], str]] = None,
                 fix_text: Optional[Callable[[str], str]] = None, tokenizer_json=None, batching: str = "chunk", slots: int = 16,
                 host_images: str = "host"):
        """`host_images`: what happens to NUMPY images (what an unmodified RapidDoc hands over).  "host" (default): each is pre-processed on
        the host with Pillow.  "stage": the uint8 [h, w, 3] arrays of a call are uploaded by one copy (`host_stage.HostImageStage`) and their
        device views take the device pre-process chunk by chunk, like device tensors - the same bits; RD_FORMULA_PREPROC=host keeps
        everything on the host.
        `batching`: "chunk" decodes every chunk of `batch_size` formulas as one batch, which runs until its longest formula has ended;
        "stream" encodes the chunks, then decodes all formulas through `slots` decode rows that take the next waiting formula as soon as
        theirs ends (`RdEngine.formula_decode_stream`).  Both return the same strings in the caller's order."""
        import torch  # noqa: F401  (device memory + stream only)
        from . import weights as W
        from .engine import RdEngine
        if batching not in ("chunk", "stream"):
            raise ValueError("batching must be 'chunk' or 'stream'")
        if host_images not in ("host", "stage"):
            raise ValueError("host_images must be 'host' or 'stage'")
        self.host_images, self._stage = host_images, None
        self.batching, self.slots = batching, int(slots)
        if isinstance(weights, (str, bytes)):
            blob = weights if isinstance(weights, bytes) else open(weights, "rb").read()
            state = W.strip_model_prefix(W.from_safetensors_bytes(blob))
        else:
            state = dict(weights)
        self.encoder = RdEngine("pphgnetv2_b6_formula", device).load_weights({k: v for k, v in state.items() if k.startswith("backbone.")})
        self.decoder = RdEngine("ppformulanet_head", device).load_weights({k: v for k, v in state.items() if k.startswith("head.")})
        self.max_new_tokens = max_new_tokens or self.decoder.formula_max_new_tokens
        if token_decoder is None and tokenizer_json is not None:
            token_decoder = make_token_decoder(tokenizer_json, fix_text if fix_text is not None else "auto")
        if token_decoder is None and bpe_decode is not None:
            from .latex_post import latex_postprocess

            def token_decoder(ids, _bpe=bpe_decode, _fix=fix_text):   # UniMERNetDecode.token2str after the EOS cut
                text = latex_postprocess(_bpe(ids))
                return _fix(text) if _fix else text
        self.token_decoder = token_decoder

    accepts_device_images = True      # batch_predict takes device uint8 [H, W, 3] RGB tensors (page windows) next to numpy images

    def batch_predict(self, image_list: Sequence, batch_size: int = 16, **kwargs) -> list:
        """numpy images are pre-processed on the host exactly as before.  Device tensors take `engine.formula_preprocess` per chunk (one
        device-to-host copy of the margin boxes per chunk; a crop it declines is copied and pre-processed on the host: the same bits),
        unless RD_FORMULA_PREPROC says "host".  `self.last_routes[i]`: "numpy", "device", "host" or "empty" for image i.
        With host_images="stage" the numpy images travel in one upload and are then treated like device tensors: "staged" where the device
        pre-processed the upload's view, "host" where its plan declined (the view is copied back: the same bits), "empty"."""
        import torch
        from .engine import formula_preprocess
        results: list = [None] * len(image_list)
        on_device = device_preproc_enabled()
        inputs: list = [None] * len(image_list)
        routes = ["numpy"] * len(image_list)
        staged_ids = self._stage_numpy(image_list) if self.host_images == "stage" and on_device else {}
        for i, im in enumerate(image_list):
            if i in staged_ids:
                inputs[i], routes[i] = staged_ids[i], "device" if staged_ids[i] is not None else "empty"
                continue
            if isinstance(im, torch.Tensor) and on_device and im.is_cuda and im.numel() > 0:
                inputs[i] = im                                            # pre-processed with its chunk
                routes[i] = "device"
            else:
                if isinstance(im, torch.Tensor):
                    im, routes[i] = im.cpu().numpy(), "host"
                inputs[i] = preprocess([im])[0]
                if inputs[i] is None:
                    routes[i] = "empty"
        valid = [i for i, x in enumerate(inputs) if x is not None]
        if self.batching == "stream":
            self._predict_stream(valid, inputs, routes, results, batch_size)
            valid = []
        for beg in range(0, len(valid), batch_size):
            chunk = valid[beg: beg + batch_size]
            dev_rows = [k for k, i in enumerate(chunk) if routes[i] == "device"]
            if dev_rows:
                xd, got = formula_preprocess([inputs[chunk[k]] for k in dev_rows])
                for k, r in zip(dev_rows, got):
                    routes[chunk[k]] = r                                  # "device", or "host" where the plan declined
            host_rows = [k for k in range(len(chunk)) if routes[chunk[k]] in ("numpy", "host") and k not in dev_rows]
            xh = torch.from_numpy(np.concatenate([inputs[chunk[k]] for k in host_rows], axis=0)).cuda(self.encoder.device) if host_rows else None
            if not dev_rows:
                x = xh
            elif not host_rows:
                x = xd
            else:                                                         # a chunk of both kinds: every row goes to its place
                x = torch.empty((len(chunk), 1) + tuple(INPUT_SIZE), dtype=torch.float32, device=xd.device)
                x[host_rows] = xh
                x[dev_rows] = xd
            ids = self.decoder.formula_decode(self.encoder.formula_encoder_forward(x), self.max_new_tokens).cpu().numpy()
            for row, i in zip(ids, chunk):
                toks = row[1:].tolist()
                if 2 in toks:
                    toks = toks[: toks.index(2)]          # UniMERNetDecode cuts at EOS (post_process.py:277-296)
                results[i] = self.token_decoder(toks) if self.token_decoder else toks
        if any(v is not None for v in staged_ids.values()):
            self._stage.release()                                         # every pre-process that reads the upload is enqueued
            for i in staged_ids:
                routes[i] = "staged" if routes[i] == "device" else routes[i]
        self.last_routes = routes
        return [r if r is not None else ([] if self.token_decoder is None else "") for r in results]

    def _stage_numpy(self, image_list: Sequence) -> dict:
        """host_images="stage": {index: device view} of the images of the call that are uint8 [h, w, 3] numpy arrays, uploaded by ONE copy
        (None for one without pixels: nothing to read, route "empty"); every other image keeps its route"""
        mine = [i for i, im in enumerate(image_list) if isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3]
        ids = [i for i in mine if image_list[i].size > 0]
        if not ids:
            return {i: None for i in mine}
        if self._stage is None:
            import torch
            from .host_stage import HostImageStage
            self._stage = HostImageStage(torch.device("cuda", self.encoder.device))
        staged = self._stage.upload([image_list[i] for i in ids])
        return {**{i: None for i in mine}, **dict(zip(ids, staged.views))}

    def _predict_stream(self, valid: list, inputs: list, routes: list, results: list, batch_size: int) -> None:
        """batching="stream": pre-process and encode the valid crops in chunks of `batch_size` (the chunk path's routes), decode every
        window of formulas that fits the token limit with one `formula_decode_stream`, cut the rows by `lens`."""
        import torch
        from .engine import FORMULA_STREAM_MAX_TOKENS, formula_preprocess
        encs = []
        for beg in range(0, len(valid), batch_size):
            chunk = valid[beg: beg + batch_size]
            dev_rows = [k for k, i in enumerate(chunk) if routes[i] == "device"]
            x = torch.empty((len(chunk), 1) + tuple(INPUT_SIZE), dtype=torch.float32, device=torch.device("cuda", self.encoder.device))
            if dev_rows:
                xd, got = formula_preprocess([inputs[chunk[k]] for k in dev_rows])
                x[dev_rows] = xd
                for k, r in zip(dev_rows, got):
                    routes[chunk[k]] = r
            host_rows = [k for k in range(len(chunk)) if k not in dev_rows]
            if host_rows:
                x[host_rows] = torch.from_numpy(np.concatenate([inputs[chunk[k]] for k in host_rows], axis=0)).to(x.device)
            encs.append(self.encoder.formula_encoder_forward(x))
        if not encs:
            self.last_stream_stats = []
            return
        enc = torch.cat(encs, dim=0)                                      # [n, S, 2048]
        self.last_stream_stats = []
        for beg, end in stream_windows(enc.shape[0], enc.shape[1], FORMULA_STREAM_MAX_TOKENS):
            ids, lens, stats = self.decoder.formula_decode_stream(enc[beg:end], self.max_new_tokens, self.slots)
            self.last_stream_stats.append(stats)
            ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
            for row, n, i in zip(ids, lens, valid[beg:end]):
                toks = row[1:int(n)].tolist()
                if toks and toks[-1] == 2:
                    toks = toks[:-1]                      # UniMERNetDecode cuts at EOS (post_process.py:277-296)
                results[i] = self.token_decoder(toks) if self.token_decoder else toks


def stream_windows(n: int, S: int, max_tokens: int) -> list:
    """(begin, end) windows over n formulas of S encoder tokens each: as many formulas per `formula_decode_stream` call as its token limit
    takes (N * S <= max_tokens).  One formula alone must fit."""
    if n <= 0:
        return []
    per = max_tokens // S
    if per < 1:
        raise ValueError(f"one formula has {S} encoder tokens, the stream decode takes {max_tokens} per call")
    return [(b, min(n, b + per)) for b in range(0, n, per)]
