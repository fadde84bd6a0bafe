"""Thin Python handle over the C-ABI: PyTorch-ROCm tensors provide device memory and the stream, the
library does all the arithmetic."""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, weights as W

REC_UNFUSED_CTC, REC_WANT_SOFTMAX, REC_WANT_LOGITS = 1, 2, 4
REC_WANT_NECK = 64          # ppocrv5_rec_server / ppocrv5_rec_mobile: `full` receives the neck's output [B, T, 120] instead (ppocr_rec_mv1e: [B, T, 64])
REC_NECK_DIMS = {"ppocr_rec_mv1e": 64}      # the SVTR neck's `dims` where it is not 120
DET_WANT_NECK = 1           # ppocrv5_det_server / ppocrv5_det_mobile / ppocrv3_det_mobile: also hand out the neck's output `fuse` [B, 256 / 96, H/4, W/4]
DET_NECK_CHANNELS = {"ppocrv5_det_server": 256, "ppocrv5_det_mobile": 96}
DET_NECK_CHANNELS_V3_MOBILE = {"ppocrv3_det_mobile": 96}    # the PP-OCRv3 multilingual detector: the same RSEFPN
CLS_WANT_AUX = 1            # ppocr_cls_mobile: also hand out [B, 2 logits | 200 pooled features]
CLS_FEATURES = 200          # channels of the classifier's pooled features (conv2 of MobileNetV3 small scale 0.35)
FORMULA_STREAM_MAX_TOKENS = 65536      # RD_FORMULA_STREAM_MAX_TOKENS: N * S of one rd_formula_decode_stream call
FORMULA_STREAM_MAX_SLOTS = 32          # RD_FORMULA_STREAM_MAX_SLOTS
TABLE_STREAM_MAX_TOKENS = 65536        # RD_TABLE_STREAM_MAX_TOKENS: N * S of one rd_table_decode_stream call
TABLE_STREAM_MAX_SLOTS = 8             # RD_TABLE_STREAM_MAX_SLOTS


class FormulaStreamStats(C.Structure):
    """rd_formula_stream_stats (include/rapiddoc_mi355.h)"""
    _fields_ = [(n, C.c_int32) for n in ("steps", "live_slot_steps", "slots", "admitted")]


class TableStreamStats(C.Structure):
    """rd_table_stream_stats (include/rapiddoc_mi355.h)"""
    _fields_ = [(n, C.c_int32) for n in ("steps", "live_slot_steps", "slots", "admitted")]


KINDS = ("ppocrv6_det", "ppocrv5_det_server", "ppocrv5_det_mobile", "ppocrv3_det_mobile", "ppocr_cls_mobile", "unitable_encoder", "unitable_decoder", "ppocrv6_rec", "ppocrv5_rec_server", "ppocrv5_rec_mobile", "ppocr_rec_mv1e", "pphgnetv2_b4", "pphgnetv2_b6_formula", "ppformulanet_head")


def rec_line_table(widths, first_tokens) -> np.ndarray:
    """int32 [B, 4] line table of rd_rec_backbone_forward_lines (include/rapiddoc_mi355.h): (w, width after stem1, width after stem3 =
    the blocks' width, first token); a line of padded width w yields (w4 // 2) = rd_rec_seq_len(w) tokens."""
    w = np.asarray(widths, dtype=np.int64).reshape(-1)
    w2 = (w - 1) // 2 + 1
    w4 = (w2 - 1) // 2 + 1
    return np.ascontiguousarray(np.stack([w, w2, w4, np.asarray(first_tokens, dtype=np.int64).reshape(-1)], axis=1).astype(np.int32))


def ragged_tables(line_lengths: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(seg int32 [n][2] = (first token, tokens) per line, tokinfo int32 [n_tokens] = position | tokens << 16)."""
    lens = np.asarray(line_lengths, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    seg = np.stack([off, lens], axis=1).astype(np.int32)
    pos = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(off, lens)
    tokinfo = (pos | (np.repeat(lens, lens) << 16)).astype(np.int32)
    return seg, tokinfo


TAIL_LINE_BUCKET, TAIL_T_BUCKET, TAIL_TOKEN_BUCKET = 32, 8, 256


def pad_tail_lengths(line_lengths) -> Tuple[np.ndarray, int]:
    """Line lengths of one `rec_tail_forward` call padded with DUMMY lines so that the plan key of the call - (lines, longest
    line, tokens) - falls on a coarse grid (multiples of 32 lines / 8 tokens / 256 tokens).  On real documents almost every
    group of rec batches has a new total token count; an exact key would build a new plan (and possibly grow the workspace,
    with a stream sync) per call.  Returns (padded lengths = the real lines followed by the dummy ones, padded longest line).
    The dummy tokens must be finite (zero) in the token buffer; their outputs sit behind the real ones and are ignored."""
    lens = np.asarray(line_lengths, dtype=np.int64)
    n, tok = len(lens), int(lens.sum())
    T = -(-int(lens.max()) // TAIL_T_BUCKET) * TAIL_T_BUCKET
    d = (n // TAIL_LINE_BUCKET + 1) * TAIL_LINE_BUCKET - n          # 1 .. 32 dummy lines
    while True:
        pad = -(-(tok + d) // TAIL_TOKEN_BUCKET) * TAIL_TOKEN_BUCKET - tok      # >= d: every dummy line gets >= 1 token
        if pad <= d * T:                                                      # and none is longer than the longest line
            break
        d += TAIL_LINE_BUCKET
    base, extra = divmod(pad, d)
    dummy = np.full(d, base, dtype=np.int64)
    dummy[:extra] += 1
    return np.concatenate([lens, dummy]), T


class EngineError(RuntimeError):
    pass


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


class RdEngine:
    """One network on one GPU (`rd_handle`).

    Range guard of the split-fp16 kernels (include/rapiddoc_mi355.h, rd_range_status) lives HERE, once, for every
    forward of every network kind: with `guard="sync"` (default) a forward that raised the range flag is repeated in
    native fp32 before it returns (one stream synchronisation per call); `guard="deferred"` is for callers that keep
    several forwards in flight (PagePipeline) and promise to call `check_range_and_fallback()` before they use the
    results; `guard="off"` leaves the flag to the caller (tests)."""

    def __init__(self, kind: str, device: int = 0, guard: str = "sync", reuse_outputs: bool = False):
        """`reuse_outputs`: the output tensors of a forward are cached per shape and handed out again by the next call with
        that shape (a later call overwrites what an earlier one returned).  For callers that consume a result before they
        issue the next forward of the same shape (PagePipeline): stable addresses are what lets the library replay a forward
        as one hipGraph launch instead of 30-90 kernel launches (csrc/engine.cpp, Engine::run)."""
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}")
        if not torch.cuda.is_available():
            raise EngineError("no ROCm device visible: rapiddoc_amd runs on MI355X only (no CPU fallback)")
        self._l = _lib.load()
        self.kind, self.device = kind, device
        self._h = self._l.rd_create(device, kind.encode())
        if not self._h:
            raise EngineError(self._l.rd_create_error().decode())
        self._tdev = torch.device("cuda", device)
        self._profiling = False
        if guard not in ("sync", "deferred", "off"):
            raise ValueError("guard must be 'sync', 'deferred' or 'off'")
        self.guard = guard
        self.range_fallbacks = 0
        self.reuse_outputs = reuse_outputs
        self._out_cache: Dict[tuple, torch.Tensor] = {}
        self.precision = os.environ.get("RD_PRECISION", "auto")   # the library reads the same variable in rd_create
        self.profile_log: List[dict] = []

    def close(self):
        if getattr(self, "_h", None):
            self._l.rd_destroy(self._h)
            self._h = None

    __del__ = close

    def _chk(self, rc: int):
        if rc != 0:
            raise EngineError(self._l.rd_last_error(self._h).decode())

    # ------------------------------------------------------------------ weights
    def load_weights(self, src: Union[bytes, str, Dict[str, np.ndarray]]):
        """`src`: path to / bytes of a .safetensors file, or a name->ndarray state dict."""
        if isinstance(src, dict):
            blob = W.to_safetensors_bytes({k: np.asarray(v) for k, v in src.items()}, skip_int=True)
        elif isinstance(src, (bytes, bytearray)):
            blob = bytes(src)
        else:
            blob = open(src, "rb").read()
        buf = C.create_string_buffer(blob, len(blob))
        self._chk(self._l.rd_load_weights(self._h, buf, len(blob)))
        return self

    @property
    def num_classes(self) -> int:
        return self._l.rd_rec_num_classes(self._h)

    def workspace_bytes(self, B: int, H: int, W_: int, flags: int = 0) -> int:
        n = C.c_size_t(0)
        self._chk(self._l.rd_query_workspace(self._h, B, H, W_, flags, C.byref(n)))
        return n.value

    # ------------------------------------------------------------------ forwards
    def _out(self, tag: str, shape: tuple, dtype, device) -> torch.Tensor:
        if not self.reuse_outputs:
            return torch.empty(shape, dtype=dtype, device=device)
        key = (tag, tuple(shape), dtype)
        t = self._out_cache.get(key)
        if t is None:
            if len(self._out_cache) > 64:
                self._out_cache.clear()
            t = self._out_cache[key] = torch.empty(shape, dtype=dtype, device=device)
        return t

    def _prep(self, x: torch.Tensor) -> torch.Tensor:
        if x.device.type != "cuda":
            x = x.to(self._tdev, non_blocking=True)
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.contiguous().float()
        return x

    def det_forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, after_launch=None, want_neck: bool = False, want_stages: bool = False):
        """Either detector kind.  `out` / `after_launch`: as in `rec_forward` (a caller-owned [B,1,H,W] float32 result tensor; work
        enqueued behind the launch).  `want_neck` (ppocrv5_det_server / ppocrv5_det_mobile / ppocrv3_det_mobile): returns (maps, fuse [B,256 / 96,H/4,W/4])
        through rd_det_forward_ex.  `want_stages` (developer, ppocrv3_det_mobile; rd_debug_det_forward_stages): returns (maps, fuse, [the four stage features NCHW])."""
        x = self._prep(x)
        B, Cc, H, W_ = x.shape
        if out is None:
            out = self._out("det", (B, 1, H, W_), torch.float32, x.device)
        elif out.shape != (B, 1, H, W_) or out.dtype != torch.float32 or not out.is_contiguous():
            raise EngineError("det_forward: `out` does not match the forward's shape")

        if want_stages:
            if self.kind != "ppocrv3_det_mobile":
                raise EngineError("det_forward: want_stages is offered by ppocrv3_det_mobile only")
            shapes = [(B, 96, H // 4, W_ // 4), (B, 16, H // 4, W_ // 4), (B, 24, H // 8, W_ // 8), (B, 56, H // 16, W_ // 16), (B, 480, H // 32, W_ // 32)]
            sizes = [int(np.prod(s)) for s in shapes]
            aux = torch.empty((sum(sizes),), dtype=torch.float32, device=x.device)

            def launch_stages():
                fn = self._l.rd_debug_det_forward_stages       # developer entry, not in the public header
                self._chk(fn(self._h, x.data_ptr(), B, H, W_, out.data_ptr(), aux.data_ptr(), _stream_ptr()))
                self._log()
            self._guarded(launch_stages)
            parts = [t.view(s) for t, s in zip(torch.split(aux, sizes), shapes)]
            return out, parts[0], parts[1:]

        neck_channels = {**DET_NECK_CHANNELS, **DET_NECK_CHANNELS_V3_MOBILE}
        if want_neck and self.kind not in neck_channels:
            raise EngineError(f"det_forward: want_neck is offered by {sorted(neck_channels)} only")
        neck = torch.empty((B, neck_channels[self.kind], H // 4, W_ // 4), dtype=torch.float32, device=x.device) if want_neck else None

        def launch():
            if want_neck:
                self._chk(self._l.rd_det_forward_ex(self._h, x.data_ptr(), B, H, W_, out.data_ptr(), DET_WANT_NECK, neck.data_ptr(), None, 0,
                                                    _stream_ptr()))
            else:
                self._chk(self._l.rd_det_forward(self._h, x.data_ptr(), B, H, W_, out.data_ptr(), None, 0, _stream_ptr()))
            self._log()
            if after_launch is not None:
                after_launch()
        self._guarded(launch)
        return (out, neck) if want_neck else out

    def cls_forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, want_aux: bool = False, want_stages: bool = False):
        """Text-line direction classifier (ppocr_cls_mobile): x [B,3,H,W] (the classifier's pre-process gives 48 x 192) -> the head's
        softmax [B,2] = (P(0 deg), P(180 deg)).  `out`: a caller-owned contiguous float32 [B,2] result tensor.  `want_aux`
        (RD_CLS_WANT_AUX): returns (prob, aux [B, 2 + 200] = logits | pooled features).  `want_stages` (developer,
        rd_debug_cls_forward_stages): returns (prob, aux, [the outputs of blocks 0, 3, 8, 10 as NCHW])."""
        if self.kind != "ppocr_cls_mobile":
            raise EngineError("cls_forward: the handle is not a ppocr_cls_mobile model")
        x = self._prep(x)
        B, Cc, H, W_ = x.shape
        if out is None:
            out = self._out("cls", (B, 2), torch.float32, x.device)
        elif out.shape != (B, 2) or out.dtype != torch.float32 or not out.is_contiguous():
            raise EngineError("cls_forward: `out` does not match the forward's shape")
        aux = torch.empty((B, 2 + CLS_FEATURES), dtype=torch.float32, device=x.device) if (want_aux or want_stages) else None
        if want_stages:
            rows, h = [], (H - 1) // 2 + 1
            for i, s in enumerate((2, 2, 1, 2, 1, 1, 1, 1, 2, 1, 1)):
                h = (h - 1) // s + 1
                if i in (0, 3, 8, 10):
                    rows.append(h)
            cols = (W_ - 1) // 2 + 1
            shapes = [(B, c, r, cols) for c, r in zip((8, 16, 32, 32), rows)]
            sizes = [int(np.prod(s)) for s in shapes]
            stages = torch.empty((sum(sizes),), dtype=torch.float32, device=x.device)

            def launch_stages():
                fn = self._l.rd_debug_cls_forward_stages       # developer entry, not in the public header
                self._chk(fn(self._h, x.data_ptr(), B, H, W_, out.data_ptr(), aux.data_ptr(), stages.data_ptr(), _stream_ptr()))
                self._log()
            self._guarded(launch_stages)
            return out, aux, [t.view(s) for t, s in zip(torch.split(stages, sizes), shapes)]

        def launch():
            self._chk(self._l.rd_cls_forward(self._h, x.data_ptr(), B, H, W_, out.data_ptr(), CLS_WANT_AUX if want_aux else 0,
                                             aux.data_ptr() if want_aux else None, None, 0, _stream_ptr()))
            self._log()
        self._guarded(launch)
        return (out, aux) if want_aux else out

    def table_encoder_forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, want_taps: bool = False):
        """UniTable table-structure encoder (unitable_encoder): x [B,3,H,W], already normalised (H, W multiples of 16, at most 1024
        patches; the product shape is 448 x 448) -> memory [B,T,768].  `out`: a caller-owned contiguous float32 [B,T,768] result tensor.
        `want_taps` (developer, rd_debug_table_encoder_taps): returns (memory, [patch embedding, layer 0 output, layer 11 output]), each
        [B,T,768]."""
        if self.kind != "unitable_encoder":
            raise EngineError("table_encoder_forward: the handle is not a unitable_encoder model")
        x = self._prep(x)
        B, Cc, H, W_ = x.shape
        if Cc != 3 or H % 16 or W_ % 16 or H < 16 or W_ < 16 or (H // 16) * (W_ // 16) > 1024:
            raise EngineError(f"table_encoder_forward: input {tuple(x.shape)}: [B,3,H,W] with H, W multiples of 16 and at most 1024 patches")
        T = (H // 16) * (W_ // 16)
        if out is None:
            out = self._out("vit", (B, T, 768), torch.float32, x.device)
        elif out.shape != (B, T, 768) or out.dtype != torch.float32 or not out.is_contiguous():
            raise EngineError("table_encoder_forward: `out` does not match the forward's shape")
        if want_taps:
            taps = torch.empty((3, B, T, 768), dtype=torch.float32, device=x.device)

            def launch_taps():
                fn = self._l.rd_debug_table_encoder_taps       # developer entry, not in the public header
                self._chk(fn(self._h, x.data_ptr(), B, H, W_, out.data_ptr(), taps.data_ptr(), _stream_ptr()))
                self._log()
            self._guarded(launch_taps)
            return out, [taps[0], taps[1], taps[2]]

        def launch():
            self._chk(self._l.rd_table_encoder_forward(self._h, x.data_ptr(), B, H, W_, out.data_ptr(), None, 0, _stream_ptr()))
            self._log()
        self._guarded(launch)
        return out

    def table_decode(self, memory: torch.Tensor, ids, max_new_tokens: int = 1024):
        """UniTable decoder and greedy loop (unitable_decoder; rd_table_decode): memory [B,S,768] from `table_encoder_forward`, B <= 8;
        `ids`: table_unitable.TableIds.  Returns (ids int64 [B, max_new_tokens + 1] on the device: prefix, emitted tokens, `pad` behind a
        table's EOS; n_tokens: per table the tokens up to and including its EOS)."""
        from .table_unitable import cfg_struct
        if self.kind != "unitable_decoder":
            raise EngineError("table_decode: the handle is not a unitable_decoder model")
        if memory.dim() != 3 or memory.shape[2] != 768 or memory.shape[0] < 1 or memory.shape[1] < 1:
            raise EngineError(f"table_decode: memory must be [B, S, 768], got {tuple(memory.shape)}")
        memory = self._prep(memory)
        B, S, _ = memory.shape
        out = torch.empty((B, max_new_tokens + 1), dtype=torch.int64, device=memory.device)
        n = (C.c_int32 * max(B, 1))()
        cfg = cfg_struct(ids)
        self._chk(self._l.rd_table_decode(self._h, memory.data_ptr(), B, S, max_new_tokens, C.byref(cfg), out.data_ptr(), n, _stream_ptr()))
        return out, [int(v) for v in n]

    def table_decode_stream(self, memory: torch.Tensor, ids, max_new_tokens: int = 1024, slots: int = 8, trace: Optional[dict] = None):
        """memory [N,S,768] -> (ids [N, max_new_tokens + 1] int64, lens [N] int32, stats): the N tables run through `slots` decode rows, a
        row whose table ends takes the next one (rd_table_decode_stream).  Row i is what `table_decode` gives table i alone - prefix,
        tokens, EOS, `pad` behind it - and lens[i] the columns that count.  N * S may be at most TABLE_STREAM_MAX_TOKENS.
        `trace` (developer, rd_debug_table_decode_stream): a dict with any of "logits" [N, max_new, 960], "hidden" [N, max_new, 4, 768]
        (float32) and "sched" [max_steps, slots, 2] (int32) device tensors, written inside the step."""
        from .table_unitable import cfg_struct
        if self.kind != "unitable_decoder":
            raise EngineError("table_decode_stream: the handle is not a unitable_decoder model")
        if memory.dim() != 3 or memory.shape[2] != 768:
            raise EngineError(f"table_decode_stream: memory must be [N, S, 768], got {tuple(memory.shape)}")
        memory = self._prep(memory)
        N, S, _ = memory.shape
        out = torch.empty((N, max(max_new_tokens, 0) + 1), dtype=torch.int64, device=memory.device)
        lens = torch.empty((N,), dtype=torch.int32, device=memory.device)
        st, cfg = TableStreamStats(), cfg_struct(ids)
        if trace is None:
            rc = self._l.rd_table_decode_stream(self._h, memory.data_ptr(), N, S, max_new_tokens, slots, C.byref(cfg), out.data_ptr(), lens.data_ptr(),
                                                C.byref(st), _stream_ptr())
        else:
            ptr = lambda k: trace[k].data_ptr() if trace.get(k) is not None else None
            sched = trace.get("sched")
            rc = self._l.rd_debug_table_decode_stream(self._h, memory.data_ptr(), N, S, max_new_tokens, slots, C.byref(cfg), out.data_ptr(),
                                                      lens.data_ptr(), C.byref(st), _stream_ptr(), ptr("logits"), ptr("hidden"), ptr("sched"),
                                                      int(sched.shape[0]) if sched is not None else 0)
        self._chk(rc)
        return out, lens, {"steps": st.steps, "live_slot_steps": st.live_slot_steps, "slots": st.slots, "admitted": st.admitted}

    def table_decode_debug(self, memory: torch.Tensor, ids, steps: int, forced: Optional[torch.Tensor] = None):
        """Developer (rd_debug_table_decode): `steps` steps with traces; forced int32 [B, steps] = the token fed to every step (EOS latch
        off), or None for the free loop.  Returns dict(ids [B, steps + 1], hidden [steps, 4, B, 768], logits [steps, B, 960], chosen /
        emitted int32 [steps, B]); rows of steps the free loop did not run are NaN / -1."""
        from .table_unitable import cfg_struct
        if self.kind != "unitable_decoder":
            raise EngineError("table_decode_debug: the handle is not a unitable_decoder model")
        if memory.dim() != 3 or memory.shape[2] != 768 or memory.shape[0] < 1 or memory.shape[1] < 1:
            raise EngineError(f"table_decode_debug: memory must be [B, S, 768], got {tuple(memory.shape)}")
        memory = self._prep(memory)
        B, S, _ = memory.shape
        dev = memory.device
        out = torch.empty((B, steps + 1), dtype=torch.int64, device=dev)
        hidden = torch.full((steps, 4, B, 768), float("nan"), device=dev)
        logits = torch.full((steps, B, 960), float("nan"), device=dev)
        chosen = torch.full((steps, B), -1, dtype=torch.int32, device=dev)
        emitted = torch.full((steps, B), -1, dtype=torch.int32, device=dev)
        if forced is not None:
            forced = forced.to(dev, torch.int32).contiguous()
            if forced.shape != (B, steps):
                raise EngineError("table_decode_debug: forced must be [B, steps]")
        fn = self._l.rd_debug_table_decode                 # developer entry, not in the public header
        cfg = cfg_struct(ids)
        self._chk(fn(self._h, memory.data_ptr(), B, S, steps, C.byref(cfg), forced.data_ptr() if forced is not None else None, out.data_ptr(),
                     hidden.data_ptr(), logits.data_ptr(), chosen.data_ptr(), emitted.data_ptr(), _stream_ptr()))
        return dict(ids=out, hidden=hidden, logits=logits, chosen=chosen, emitted=emitted)

    def rec_forward(self, x: torch.Tensor, flags: int = 0, out: Optional[tuple] = None,
                    after_launch=None) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """`out`: (idx int32 [B,T], prob float32 [B,T], full float32 [B,T,C] or None) contiguous device tensors to write into - a caller
        that hands over the SAME addresses call after call (session.Mi355RecSession) lets the library replay the forward as one
        hipGraph launch.  `after_launch()`: enqueued behind every (re)launch, in front of the range guard's synchronisation (e.g. the
        caller's device -> host copies, so that one synchronisation serves both)."""
        x = self._prep(x)
        B, Cc, H, W_ = x.shape
        if H != 48:
            raise EngineError("rec input height must be 48")
        T = self._l.rd_rec_seq_len(W_)
        want_full = bool(flags & (REC_WANT_SOFTMAX | REC_WANT_LOGITS | REC_WANT_NECK))
        n_full = REC_NECK_DIMS.get(self.kind, 120) if flags & REC_WANT_NECK else None       # (the SVTR neck's `dims`; every other flag: the class count)
        if out is not None:
            idx, prob, full = out
            ok = (idx.shape == (B, T) and idx.dtype == torch.int32 and idx.is_contiguous() and prob.shape == (B, T)
                  and prob.dtype == torch.float32 and prob.is_contiguous()
                  and (not want_full or (full is not None and full.shape == (B, T, n_full or self.num_classes) and full.dtype == torch.float32
                                         and full.is_contiguous())))
            if not ok:
                raise EngineError("rec_forward: `out` tensors do not match the forward's shapes")
        else:
            idx = torch.empty((B, T), dtype=torch.int32, device=x.device)
            prob = torch.empty((B, T), dtype=torch.float32, device=x.device)
            full = torch.empty((B, T, n_full or self.num_classes), dtype=torch.float32, device=x.device) if want_full else None

        def launch():
            self._chk(self._l.rd_rec_forward(self._h, x.data_ptr(), B, W_, idx.data_ptr(), prob.data_ptr(),
                                             full.data_ptr() if want_full else None, flags, None, 0, _stream_ptr()))
            self._log()
            if after_launch is not None:
                after_launch()
        self._guarded(launch)
        return idx, prob, (full if want_full else None)

    @property
    def backbone(self) -> str:
        """The backbone the loaded weights picked (read-only): "pphgnetv2_b4" or "pphgnet_small" for the two server kinds - a PP-OCRv4
        server state dict (ch_PP-OCRv4_det_server / _rec_server) loads under "ppocrv5_det_server" / "ppocrv5_rec_server" with PPHGNet_small;
        "" for every other kind."""
        return (self._l.rd_backbone_name(self._h) or b"").decode()

    # two-stage form of the recogniser (include/rapiddoc_mi355.h: rd_rec_backbone_forward / rd_rec_tail_forward)
    @property
    def rec_token_dim(self) -> int:
        return self._l.rd_rec_token_dim(self._h)

    def rec_backbone_forward(self, x: torch.Tensor, tokens_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [B,3,48,W] -> pooled backbone tokens [B, T, dim]; `tokens_out`: a contiguous float32 view to write them into."""
        x = self._prep(x)
        B, Cc, H, W_ = x.shape
        if H != 48:
            raise EngineError("rec input height must be 48")
        T = self._l.rd_rec_seq_len(W_)
        if tokens_out is None:
            tokens_out = torch.empty((B, T, self.rec_token_dim), dtype=torch.float32, device=x.device)
        if tokens_out.numel() != B * T * self.rec_token_dim or not tokens_out.is_contiguous() or tokens_out.dtype != torch.float32:
            raise EngineError("tokens_out must be a contiguous float32 tensor of B*T*dim elements")

        def launch():
            self._chk(self._l.rd_rec_backbone_forward(self._h, x.data_ptr(), B, W_, tokens_out.data_ptr(), None, 0, _stream_ptr()))
            self._log()
        self._guarded(launch)
        return tokens_out

    def rec_backbone_forward_lines(self, x: torch.Tensor, line_tab: torch.Tensor, tokens_out: torch.Tensor) -> torch.Tensor:
        """The backbone stage over lines of DIFFERENT reference padded widths (rd_rec_backbone_forward_lines): x [B,3,48,W] with
        line b in columns [0, w_b), `line_tab` = `rec_line_table(widths, first tokens)` on the device, `tokens_out` the token buffer
        the table's offsets refer to.  Line b's tokens == rec_backbone_forward(x[b:b+1, :, :, :w_b])."""
        x = self._prep(x)
        B, Cc, H, W_ = x.shape
        if H != 48:
            raise EngineError("rec input height must be 48")
        if line_tab.dtype != torch.int32 or not line_tab.is_cuda or line_tab.numel() != 4 * B or not line_tab.is_contiguous():
            raise EngineError("line_tab must be a contiguous int32 device tensor [B, 4]")
        if not tokens_out.is_contiguous() or tokens_out.dtype != torch.float32:
            raise EngineError("tokens_out must be a contiguous float32 tensor")

        def launch():
            self._chk(self._l.rd_rec_backbone_forward_lines(self._h, x.data_ptr(), B, W_, line_tab.data_ptr(), tokens_out.data_ptr(), None, 0,
                                                            _stream_ptr()))
            self._log()
        self._guarded(launch)
        return tokens_out

    def rec_tail_tables(self, line_lengths, device, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The two int32 tables rd_rec_tail_forward wants, as one device tensor [2 * n_lines + n_tokens] (seg, then tokinfo).
        `out`: a device int32 buffer at least that long to fill instead of a new tensor (a view of its head is returned)."""
        seg_h, tokinfo_h = ragged_tables(np.asarray(line_lengths, dtype=np.int64))
        host = torch.from_numpy(np.concatenate([seg_h.reshape(-1), tokinfo_h])).pin_memory()
        if out is None:
            return host.to(device, non_blocking=True)
        view = out[: host.numel()]
        view.copy_(host, non_blocking=True)
        self._keep_host = getattr(self, "_keep_host", [])[-15:] + [host]      # the pinned source must outlive the asynchronous copy
        return view

    def rec_tail_forward(self, tokens: torch.Tensor, line_lengths, tables: Optional[torch.Tensor] = None,
                         max_tokens: Optional[int] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """tokens [n_tokens, dim] = the text lines back to back, `line_lengths` their token counts -> (idx, prob) [n_tokens].
        `tables`: rec_tail_tables(line_lengths) uploaded earlier (e.g. before the backbones were enqueued).  `max_tokens`: an
        upper bound of the longest line used as the plan key instead of the exact maximum (see `pad_tail_lengths`).  `out`:
        (idx int32 [n_tokens], prob float32 [n_tokens]) to write into."""
        lens = np.asarray(line_lengths, dtype=np.int64)
        n_tokens = int(lens.sum())
        longest = int(lens.max()) if max_tokens is None else int(max_tokens)
        if longest < int(lens.max()):
            raise EngineError("rec tail: max_tokens below the longest line")
        if tokens.numel() != n_tokens * self.rec_token_dim or lens.min() < 1 or lens.max() >= 32768:
            raise EngineError("rec tail: token count / line lengths mismatch")
        dev = tokens.device
        if tables is None:
            tables = self.rec_tail_tables(lens, dev)
        seg, tokinfo = tables[: 2 * len(lens)], tables[2 * len(lens):]
        if out is not None:
            idx, prob = out
            assert idx.numel() == n_tokens and prob.numel() == n_tokens and idx.dtype == torch.int32 and prob.dtype == torch.float32
        else:
            idx = torch.empty((n_tokens,), dtype=torch.int32, device=dev)
            prob = torch.empty((n_tokens,), dtype=torch.float32, device=dev)

        def launch():
            self._chk(self._l.rd_rec_tail_forward(self._h, tokens.data_ptr(), n_tokens, len(lens), longest, seg.data_ptr(),
                                                  tokinfo.data_ptr(), idx.data_ptr(), prob.data_ptr(), None, 0, _stream_ptr()))
            self._log()
        self._guarded(launch)
        self._keep = (tables,)          # the tables must outlive the asynchronous launch
        return idx, prob

    def backbone_forward(self, x: torch.Tensor) -> List[torch.Tensor]:
        x = self._prep(x)
        B, Cc, H, W_ = x.shape
        chans = (128, 512, 1024, 2048)
        feats = [self._out("feat%d" % s, (B, c, H // s, W_ // s), torch.float32, x.device)
                 for c, s in zip(chans, (4, 8, 16, 32))]
        arr = (C.c_void_p * 4)(*[f.data_ptr() for f in feats])

        def launch():
            self._chk(self._l.rd_backbone_forward(self._h, x.data_ptr(), B, H, W_, arr, None, 0, _stream_ptr()))
            self._log()
        self._guarded(launch)
        return feats

    def formula_encoder_forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B,1|3,H,W] -> encoder states [B, (H/32)*(W/32), 2048] (PPHGNetV2_B6_Formula.last_hidden_state)."""
        x = self._prep(x)
        B, Cc, H, W_ = x.shape
        out = torch.empty((B, (H // 32) * (W_ // 32), 2048), dtype=torch.float32, device=x.device)

        def launch():
            self._chk(self._l.rd_formula_encoder_forward(self._h, x.data_ptr(), B, Cc, H, W_, out.data_ptr(), None, 0, _stream_ptr()))
            self._log()
        self._guarded(launch)
        return out

    def formula_decode(self, enc: torch.Tensor, max_new_tokens: int) -> torch.Tensor:
        """enc [B,S,2048] -> token ids [B,L] int64 exactly as PPFormulaNet_Head.forward returns them."""
        enc = self._prep(enc)
        B, S, _ = enc.shape
        ids = torch.empty((B, max_new_tokens + 1), dtype=torch.int64, device=enc.device)
        n = C.c_int32(0)
        self._chk(self._l.rd_formula_decode(self._h, enc.data_ptr(), B, S, max_new_tokens, ids.data_ptr(), C.byref(n), _stream_ptr()))
        return ids[:, : n.value]

    def formula_decode_stream(self, enc: torch.Tensor, max_new_tokens: int, slots: int = 16, trace: Optional[dict] = None):
        """enc [N,S,2048] -> (ids [N, max_new_tokens + 1] int64, lens [N] int32, stats): the N formulas run through `slots` decode rows,
        a row whose formula ends takes the next one (rd_formula_decode_stream).  Row i is what `formula_decode` gives formula i - start
        token, tokens, EOS, PAD behind it - and lens[i] the columns that count.  N * S may be at most FORMULA_STREAM_MAX_TOKENS.
        `trace` (developer, rd_debug_formula_decode_stream): a dict with any of "logits" [N, max_new, V], "hidden" [N, max_new, 512]
        (float32) and "sched" [max_steps, slots, 2] (int32) device tensors, written inside the step."""
        enc = self._prep(enc)
        N, S, _ = enc.shape
        ids = torch.empty((N, max_new_tokens + 1), dtype=torch.int64, device=enc.device)
        lens = torch.empty((N,), dtype=torch.int32, device=enc.device)
        st = FormulaStreamStats()
        if trace is None:
            rc = self._l.rd_formula_decode_stream(self._h, enc.data_ptr(), N, S, max_new_tokens, slots, ids.data_ptr(), lens.data_ptr(),
                                                  C.byref(st), _stream_ptr())
        else:
            ptr = lambda k: trace[k].data_ptr() if trace.get(k) is not None else None
            sched = trace.get("sched")
            rc = self._l.rd_debug_formula_decode_stream(self._h, enc.data_ptr(), N, S, max_new_tokens, slots, ids.data_ptr(), lens.data_ptr(),
                                                        C.byref(st), _stream_ptr(), ptr("logits"), ptr("hidden"), ptr("sched"),
                                                        int(sched.shape[0]) if sched is not None else 0)
        self._chk(rc)
        return ids, lens, {"steps": st.steps, "live_slot_steps": st.live_slot_steps, "slots": st.slots, "admitted": st.admitted}

    @property
    def formula_max_new_tokens(self) -> int:
        return self._l.rd_formula_max_new_tokens(self._h)

    # ------------------------------------------------------------------ precision (include/rapiddoc_mi355.h)
    def set_precision(self, mode: str):
        """'auto' (default: split-fp16 channel mixers, fp32 MFMA elsewhere), 'fp32' (native fp32 MFMA only) or 'h3'."""
        self._chk(self._l.rd_set_precision(self._h, mode.encode()))
        self.precision = mode
        return self

    def _guarded(self, launch) -> None:
        """Run `launch` (enqueue one forward); in "sync" mode repeat it in native fp32 if a split kernel flagged an
        operand outside the fp16 range - a result is never silently wrong, whichever entry point produced it."""
        launch()
        if self.guard == "sync" and self.precision != "fp32" and self.range_overflow():
            self.set_precision("fp32")
            self.range_fallbacks += 1
            launch()

    def check_range_and_fallback(self) -> bool:
        """Deferred guard: True when forwards since the last check overflowed; the handle is then switched to fp32 and
        the CALLER must repeat those forwards."""
        if self.precision != "fp32" and self.range_overflow():
            self.set_precision("fp32")
            self.range_fallbacks += 1
            return True
        return False

    def range_overflow(self) -> bool:
        """True when a split-fp16 kernel met an operand outside the fp16 range since the last call (synchronises the
        current stream, clears the flag).  The results of those calls are invalid: switch to 'fp32' and repeat them."""
        rc = self._l.rd_range_status(self._h, _stream_ptr())
        if rc < 0:
            raise EngineError(self._l.rd_last_error(self._h).decode())
        return rc == 1

    # ------------------------------------------------------------------ profiling
    def plan_stats(self) -> dict:
        """{plans_built, graph_captures, graph_replays} of this handle since it was created (rd_plan_stats)."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._chk(self._l.rd_plan_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"plans_built": int(a.value), "graph_captures": int(b.value), "graph_replays": int(c.value)}

    def set_profiling(self, on: bool):
        self._chk(self._l.rd_set_profiling(self._h, 1 if on else 0))
        self._profiling = bool(on)

    def _log(self):
        if self._profiling:
            self.profile_log.extend(self.profile())

    def profile(self) -> List[dict]:
        return json.loads(self._l.rd_profile_json(self._h).decode())


def preproc_resize_norm(img_u8_hwc: torch.Tensor, out_hw: Tuple[int, int], mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0),
                        scale: float = 1.0 / 255.0, interp: int = 2, swap_rb: bool = False,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """u8 HWC device image -> normalised CHW float32 (PPPreProcess, pp_doclayout/pre_process.py:22-42)."""
    lib = _lib.load()
    assert img_u8_hwc.is_cuda and img_u8_hwc.dtype == torch.uint8 and img_u8_hwc.is_contiguous()
    H, W_, ch = img_u8_hwc.shape
    assert ch == 3
    OH, OW = out_hw
    if out is None:
        out = torch.empty((3, OH, OW), dtype=torch.float32, device=img_u8_hwc.device)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    rc = lib.rd_preproc_resize_norm(img_u8_hwc.device.index or 0, img_u8_hwc.data_ptr(), H, W_, OH, OW, m, s, scale,
                                    interp, 1 if swap_rb else 0, out.data_ptr(), _stream_ptr())
    if rc != 0:
        raise EngineError("rd_preproc_resize_norm failed")
    return out


def preproc_resize_norm_batch(imgs_u8_nhwc: torch.Tensor, out_hw: Tuple[int, int], mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0),
                              scale: float = 1.0 / 255.0, interp: int = 2, swap_rb: bool = False,
                              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`preproc_resize_norm` for a whole [P,H,W,3] u8 array in one launch -> [P,3,OH,OW] float32."""
    lib = _lib.load()
    assert imgs_u8_nhwc.is_cuda and imgs_u8_nhwc.dtype == torch.uint8 and imgs_u8_nhwc.is_contiguous() and imgs_u8_nhwc.dim() == 4
    P, H, W_, ch = imgs_u8_nhwc.shape
    assert ch == 3
    OH, OW = out_hw
    if out is None:
        out = torch.empty((P, 3, OH, OW), dtype=torch.float32, device=imgs_u8_nhwc.device)
    assert out.is_contiguous() and tuple(out.shape) == (P, 3, OH, OW)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    rc = lib.rd_preproc_resize_norm_batch(imgs_u8_nhwc.device.index or 0, imgs_u8_nhwc.data_ptr(), P, H, W_, OH, OW, m, s, scale,
                                          interp, 1 if swap_rb else 0, out.data_ptr(), _stream_ptr())
    if rc != 0:
        raise EngineError("rd_preproc_resize_norm_batch failed")
    return out


# rd_resize_source_desc: a source image that names its own address, pitch, sizes and destination (rd_preproc_resize_norm_sources)
RESIZE_SOURCE_DTYPE = np.dtype([("src", "<u8"), ("pitch", "<i8"), ("out_off", "<i8"), ("W", "<i4"), ("H", "<i4"), ("OW", "<i4"), ("OH", "<i4"),
                                ("reserved", "<i4", (2,))])


def pack_resize_sources(ptrs: Sequence[int], pitches: Sequence[int], hws: Sequence[Tuple[int, int]], out_hws: Sequence[Tuple[int, int]],
                        out_offs: Sequence[int]) -> np.ndarray:
    """Host only: one rd_resize_source_desc per source.  `ptrs[k]` / `pitches[k]`: device address of pixel (0, 0) and bytes between rows of
    source k, `hws[k]` = (H, W) its size, `out_hws[k]` = (OH, OW) its output size, `out_offs[k]` the offset in FLOATS of its planes."""
    n = len(ptrs)
    if not (len(pitches) == len(hws) == len(out_hws) == len(out_offs) == n):
        raise ValueError("pack_resize_sources: one pitch, size, output size and offset per source")
    descs = np.zeros(n, dtype=RESIZE_SOURCE_DTYPE)
    for k in range(n):
        (h, w), (oh, ow) = hws[k], out_hws[k]
        descs[k] = (int(ptrs[k]), int(pitches[k]), int(out_offs[k]), int(w), int(h), int(ow), int(oh), (0, 0))
    return descs


def resize_source_view(t: torch.Tensor) -> Tuple[int, int]:
    """(device address, row pitch in bytes) of a uint8 [H, W, 3] device image as rd_preproc_resize_norm_sources reads it: channels 1 byte
    and pixels 3 bytes apart, rows at a pitch of at least 3 * W - a window of a larger image is read where it lies."""
    if not (t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3 and t.shape[0] >= 1 and t.shape[1] >= 1):
        raise EngineError(f"a resize source must be a uint8 [H, W, 3] device image, got {t.dtype} {tuple(t.shape)} on {t.device}")
    h, w = int(t.shape[0]), int(t.shape[1])
    if not (t.stride(2) == 1 and (w == 1 or t.stride(1) == 3) and (h == 1 or t.stride(0) >= 3 * w)):
        raise EngineError(f"a resize source must have packed pixels and a row pitch of at least 3 * W, got strides {tuple(t.stride())}")
    return t.data_ptr(), (int(t.stride(0)) if h > 1 else 3 * w)


def launch_resize_sources(descs: np.ndarray, device: torch.device, out_ptr: int, out_floats: int, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0),
                          scale: float = 1.0 / 255.0, interp: int = 2, swap_rb: bool = False) -> None:
    """rd_preproc_resize_norm_sources on a descriptor array: its device copy is uploaded here (pinned, asynchronous, current stream).  Bad
    arguments raise EngineError with the library's message; nothing is launched then."""
    lib = _lib.load()
    descs = np.ascontiguousarray(descs, dtype=RESIZE_SOURCE_DTYPE)
    host = torch.empty(max(descs.nbytes, 16), dtype=torch.uint8, pin_memory=True)
    host[: descs.nbytes] = torch.from_numpy(descs.view(np.uint8).reshape(-1))
    dev = host.to(device, non_blocking=True)
    rc = lib.rd_preproc_resize_norm_sources(device.index or 0, descs.ctypes.data, dev.data_ptr(), len(descs), (C.c_float * 3)(*mean),
                                            (C.c_float * 3)(*std), scale, int(interp), 1 if swap_rb else 0, out_ptr, C.c_int64(int(out_floats)),
                                            _stream_ptr())
    if rc != 0:
        raise EngineError(lib.rd_create_error().decode())


def preproc_resize_norm_sources(sources: Sequence[torch.Tensor], out_hws: Sequence[Tuple[int, int]], mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0),
                                scale: float = 1.0 / 255.0, interp: int = 2, swap_rb: bool = False,
                                out: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """`preproc_resize_norm` for uint8 [H_k, W_k, 3] device images of DIFFERENT sizes, source k to out_hws[k] = (OH_k, OW_k), in ONE launch
    (rd_preproc_resize_norm_sources) -> one [3, OH_k, OW_k] float32 tensor per source, bit for bit what `preproc_resize_norm` gives for a
    contiguous copy.  A source may be a window of a larger image (row pitch above 3 * W).  `out`: one contiguous float32 [3, OH_k, OW_k]
    destination per source, anywhere on the sources' device (rows of per-shape batch tensors, say) as long as no two overlap; default:
    views of one new buffer.  Bad arguments raise EngineError; nothing is launched then."""
    n = len(sources)
    if n == 0:
        return []
    if len(out_hws) != n or (out is not None and len(out) != n):
        raise EngineError("preproc_resize_norm_sources: one output size (and one `out` tensor) per source")
    device = sources[0].device
    views = [resize_source_view(t) for t in sources]
    if any(t.device != device for t in sources):
        raise EngineError("preproc_resize_norm_sources: the sources must lie on one device")
    out_hws = [(int(oh), int(ow)) for oh, ow in out_hws]
    if out is None:
        offs = np.concatenate([[0], np.cumsum([3 * oh * ow for oh, ow in out_hws])]).astype(np.int64)
        flat = torch.empty(int(offs[-1]), dtype=torch.float32, device=device)
        out = [flat[int(o): int(o) + 3 * oh * ow].view(3, oh, ow) for o, (oh, ow) in zip(offs[:-1], out_hws)]
    for t, (oh, ow) in zip(out, out_hws):
        if not (t.is_cuda and t.device == device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (3, oh, ow)):
            raise EngineError(f"preproc_resize_norm_sources: an `out` tensor does not match [3, {oh}, {ow}] float32 on {device}")
    base = min(t.data_ptr() for t in out)          # one base address for the call: every destination is a float offset from it
    offs = [(t.data_ptr() - base) // 4 for t in out]
    out_floats = max(o + t.numel() for o, t in zip(offs, out))
    descs = pack_resize_sources([p for p, _ in views], [q for _, q in views], [(int(t.shape[0]), int(t.shape[1])) for t in sources], out_hws, offs)
    launch_resize_sources(descs, device, base, out_floats, mean, std, scale, interp, swap_rb)
    return list(out)


def preproc_resize_aa_norm(img_u8_hwc: torch.Tensor, out_hw: Tuple[int, int], mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), swap_rb: bool = False,
                           return_u8: bool = False, out: Optional[torch.Tensor] = None):
    """u8 HWC device image -> Pillow's antialiased bilinear resample (bit for bit) -> ((v / 255) - mean) / std -> CHW float32
    (rd_preproc_resize_aa_norm: transforms.Resize on a PIL image + ToTensor + Normalize, UniTable's TablePreprocess).  `return_u8`: returns
    (out, the resampled bytes [OH, OW, 3] uint8).  A size outside 1 .. 16384 raises EngineError; nothing is launched."""
    lib = _lib.load()
    if not (img_u8_hwc.is_cuda and img_u8_hwc.dtype == torch.uint8 and img_u8_hwc.is_contiguous() and img_u8_hwc.dim() == 3 and img_u8_hwc.shape[2] == 3):
        raise EngineError("preproc_resize_aa_norm: the image must be a contiguous uint8 [H, W, 3] device tensor")
    H, W_, _ = img_u8_hwc.shape
    OH, OW = (int(v) for v in out_hw)
    ok = 1 <= OH <= 16384 and 1 <= OW <= 16384
    if out is None:
        out = torch.empty((3, OH, OW) if ok else (0,), dtype=torch.float32, device=img_u8_hwc.device)
    elif tuple(out.shape) != (3, OH, OW) or out.dtype != torch.float32 or not out.is_contiguous():
        raise EngineError("preproc_resize_aa_norm: `out` does not match [3, OH, OW] float32")
    u8 = torch.empty((OH, OW, 3) if ok else (0,), dtype=torch.uint8, device=img_u8_hwc.device) if return_u8 else None
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    rc = lib.rd_preproc_resize_aa_norm(img_u8_hwc.device.index or 0, img_u8_hwc.data_ptr(), H, W_, OH, OW, m, s, 1 if swap_rb else 0,
                                       out.data_ptr(), u8.data_ptr() if return_u8 else None, _stream_ptr())
    if rc != 0:
        raise EngineError(lib.rd_create_error().decode())
    return (out, u8) if return_u8 else out


# ---------------------------------------------------------------------------------------------------------------- the formula pre-process
FORMULA_SIDE = 384
FORMULA_CROP_DTYPE = np.dtype([("base", "<u8"), ("pitch", "<i8"), ("w", "<i4"), ("h", "<i4")])            # rd_formula_crop


class FormulaPlan(C.Structure):
    """rd_formula_plan (include/rapiddoc_mi355.h)"""
    _fields_ = [(n, C.c_int32) for n in ("served", "resize_w", "resize_h", "thumb", "final_w", "final_h", "fx", "fy", "reduced_w", "reduced_h")] + \
               [("box_w", C.c_float), ("box_h", C.c_float), ("pad_x", C.c_int32), ("pad_y", C.c_int32)]


def formula_preproc_plan(w: int, h: int) -> FormulaPlan:
    """What follows from a margin box of w x h pixels (rd_formula_preproc_plan: host only, needs no GPU)."""
    p = FormulaPlan()
    if _lib.load().rd_formula_preproc_plan(int(w), int(h), C.byref(p)) != 0:
        raise EngineError("rd_formula_preproc_plan failed")
    return p


def _formula_view(t: torch.Tensor) -> Optional[torch.Tensor]:
    """the tensor as the kernels read it (a [H, W, 3] uint8 device window: channels and pixels packed, any row pitch), or None when the
    device path does not take it (grey-level, empty, beyond the bound)"""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3):
        return None
    H, W_ = int(t.shape[0]), int(t.shape[1])
    if not (1 <= H <= 16384 and 1 <= W_ <= 16384):
        return None
    if t.stride(2) != 1 or t.stride(1) != 3 or (H > 1 and t.stride(0) < 3 * W_):
        t = t.contiguous()
    return t


def formula_margin_boxes(crops: List[torch.Tensor]) -> torch.Tensor:
    """[n] device uint8 [H, W, 3] windows -> int32 [n, 4] (x0, y0, x1, y1) ON THE DEVICE: the margin box of every crop
    (rd_formula_margin_boxes, one launch).  The windows must be what `_formula_view` returns."""
    lib = _lib.load()
    dev = crops[0].device
    descs = _formula_descs(crops)
    boxes = torch.empty((len(crops), 4), dtype=torch.int32, device=dev)
    d_dev = torch.from_numpy(descs.view(np.uint8)).to(dev)
    if lib.rd_formula_margin_boxes(dev.index or 0, d_dev.data_ptr(), len(crops), boxes.data_ptr(), _stream_ptr()) != 0:
        raise EngineError(lib.rd_create_error().decode())
    return boxes


def _formula_descs(crops: List[torch.Tensor]) -> np.ndarray:
    descs = np.zeros(len(crops), dtype=FORMULA_CROP_DTYPE)
    for i, t in enumerate(crops):
        descs[i] = (t.data_ptr(), t.stride(0) if t.shape[0] > 1 else 3 * int(t.shape[1]), int(t.shape[1]), int(t.shape[0]))
    return descs


def formula_preprocess(crops: list, return_u8: bool = False):
    """The pre-process of PP-FormulaNet_plus for a list of device uint8 [H, W, 3] RGB crops (windows of a page batch are taken as they
    are, no copy) -> (x [n, 1, 384, 384] float32 on the device, routes): bit for bit what `formula_host.preprocess` gives.

    One launch finds every margin box, ONE device-to-host copy brings the [n, 4] boxes back (every later size follows from the box),
    then everything up to `x` is enqueued without another synchronisation.  routes[i]: "device", or "host" for a crop the device path
    declines - an intermediate beyond 16384 pixels, a grey-level or empty tensor, a numpy array: it is copied to the host, goes through
    `formula_host.preprocess` and its row is uploaded; "empty" when that returns None (the row is zero).  `return_u8`: also returns the
    padded uint8 images [n, 384, 384, 3] (rows of host-routed crops included)."""
    lib = _lib.load()
    n = len(crops)
    dev = next((c.device for c in crops if isinstance(c, torch.Tensor) and c.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    x = torch.zeros((n, 1, FORMULA_SIDE, FORMULA_SIDE), dtype=torch.float32, device=dev)
    u8 = torch.zeros((n, FORMULA_SIDE, FORMULA_SIDE, 3), dtype=torch.uint8, device=dev) if return_u8 else None
    routes = ["host"] * n
    views = [_formula_view(c) for c in crops]
    cand = [i for i, v in enumerate(views) if v is not None]
    if cand:
        boxes = formula_margin_boxes([views[i] for i in cand]).cpu().numpy()                 # the one device-to-host copy
        served = [k for k, b in enumerate(boxes) if formula_preproc_plan(int(b[2] - b[0]), int(b[3] - b[1])).served]
        if served:
            idx = [cand[k] for k in served]
            descs = _formula_descs([views[i] for i in idx])
            b = np.ascontiguousarray(boxes[served], dtype=np.int32)
            whole = len(idx) == n
            xo = x if whole else torch.empty((len(idx), 1, FORMULA_SIDE, FORMULA_SIDE), dtype=torch.float32, device=dev)
            uo = None if u8 is None else (u8 if whole else torch.empty((len(idx), FORMULA_SIDE, FORMULA_SIDE, 3), dtype=torch.uint8, device=dev))
            rc = lib.rd_formula_preproc_batch(dev.index or 0, descs.ctypes.data, b.ctypes.data, len(idx), xo.data_ptr(),
                                              uo.data_ptr() if uo is not None else None, _stream_ptr())
            if rc != 0:
                raise EngineError(lib.rd_create_error().decode())
            if not whole:
                at = torch.tensor(idx, dtype=torch.long, device=dev)
                x.index_copy_(0, at, xo)
                if u8 is not None:
                    u8.index_copy_(0, at, uo)
            for i in idx:
                routes[i] = "device"
    if any(r == "host" for r in routes):
        from . import formula_host
        for i, r in enumerate(routes):
            if r != "host":
                continue
            img = crops[i].cpu().numpy() if isinstance(crops[i], torch.Tensor) else np.asarray(crops[i])
            d = formula_host.decode_image(img) if img.size else None
            if d is None:
                routes[i] = "empty"
                continue
            x[i].copy_(torch.from_numpy(formula_host.to_network_input(d)[0]))
            if u8 is not None:
                u8[i].copy_(torch.from_numpy(d))
    return (x, routes, u8) if return_u8 else (x, routes)


# ---------------------------------------------------------------------------------------------------------------- region composition
REGION_MAX_POLY = 64                                                                                        # RD_REGION_MAX_POLY
REGION_DESC_DTYPE = np.dtype([("page", "<u8"), ("pitch", "<i8")] + [(n, "<i4") for n in (
    "page_w", "page_h", "x0", "y0", "x1", "y1", "paste_x", "paste_y", "poly_off", "poly_n", "box_off", "box_n")])      # rd_region_desc


class Region(NamedTuple):
    """One region of `region_canvases`: `page` a [H, W, 3] uint8 tensor (a window of a larger buffer is fine: pixels and channels packed,
    any row pitch), `rect` the UNclipped (x0, y0, x1, y1) in page coordinates, `paste` the canvas position of (x0, y0), `polygon` the
    region's polygon_points in page coordinates or None, `boxes` the integer mask boxes in CANVAS coordinates (clipped, non-empty)."""
    page: torch.Tensor
    rect: Tuple[int, int, int, int]
    paste: Tuple[int, int] = (0, 0)
    polygon: Optional[Sequence] = None
    boxes: Sequence[Sequence[int]] = ()


def region_polygon(polygon_points) -> np.ndarray:
    """polygon_points as the raster takes them: int32 [n, 2], truncated towards zero (crop_img's np.array(..., dtype=np.int32))."""
    return np.array(polygon_points, dtype=np.int32).reshape(-1, 2)


def pack_regions(groups: Sequence[Sequence[Region]]):
    """Host only: the descriptors of every region of every group, group after group, and the vertex and box lists they index ->
    (descs [total] REGION_DESC_DTYPE, pts int32 [*, 2], boxes int32 [*, 4], first descriptor of every group)."""
    total = sum(len(g) for g in groups)
    descs = np.zeros(total, dtype=REGION_DESC_DTYPE)
    pts: List[np.ndarray] = []
    boxes: List[Sequence[int]] = []
    firsts, k, n_pts = [], 0, 0
    for g in groups:
        firsts.append(k)
        for r in g:
            t = r.page
            if not (t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3 and t.stride(2) == 1 and t.stride(1) == 3):
                raise EngineError("region_canvases: a page must be a uint8 [H, W, 3] tensor with packed pixels")
            H, W_ = int(t.shape[0]), int(t.shape[1])
            poly = region_polygon(r.polygon) if r.polygon is not None and len(r.polygon) else np.zeros((0, 2), np.int32)
            descs[k] = (t.data_ptr(), t.stride(0) if H > 1 else 3 * W_, W_, H, *(int(v) for v in r.rect), int(r.paste[0]), int(r.paste[1]),
                        n_pts, len(poly), len(boxes), len(r.boxes))
            pts.append(poly)
            n_pts += len(poly)
            boxes.extend([int(v) for v in b] for b in r.boxes)
            k += 1
    return (descs, np.concatenate(pts).astype(np.int32).reshape(-1, 2) if pts else np.zeros((0, 2), np.int32),
            np.asarray(boxes, dtype=np.int32).reshape(-1, 4), firsts)


class RegionStage:
    """The descriptors of all size groups of a batch on the device: packed into ONE pinned staging buffer, uploaded by ONE asynchronous
    copy on the current stream; `region_canvases` then makes one launch per group out of it."""

    def __init__(self, groups: Sequence[Sequence[Region]], device):
        self.groups = [list(g) for g in groups]
        descs, pts, boxes, self.firsts = pack_regions(self.groups)
        parts = [descs.view(np.uint8).reshape(-1), pts.view(np.uint8).reshape(-1), boxes.view(np.uint8).reshape(-1)]
        offs, n = [], 0
        for part in parts:
            offs.append(n)
            n += (part.size + 15) // 16 * 16
        self.host = torch.empty(max(n, 16), dtype=torch.uint8, pin_memory=True)
        for o, part in zip(offs, parts):
            if part.size:
                self.host[o:o + part.size] = torch.from_numpy(part)
        self.dev = self.host.to(device, non_blocking=True)
        base = self.dev.data_ptr()
        self.descs_ptr, self.pts_ptr, self.boxes_ptr = base + offs[0], (base + offs[1]) if len(pts) else None, (base + offs[2]) if len(boxes) else None
        self.any_poly = [any(r.polygon is not None and len(r.polygon) for r in g) for g in self.groups]


def region_canvases(regions: Sequence[Region], group_hw: Tuple[int, int], want_masked: bool, stage: Optional[RegionStage] = None, group: int = 0):
    """The canvases of one size group, composed on the device (rd_region_canvases; include/rapiddoc_mi355.h has the semantics) ->
    (canv [n, gh, gw, 3] uint8, det_canv or None): `canv` the regions on white, `det_canv` - when `want_masked` - the same with every
    region's mask boxes at 255.  `stage` / `group`: the batch's RegionStage and this group's position in it; without one the group is
    staged by itself.  Bad arguments raise EngineError; nothing is launched."""
    lib = _lib.load()
    if stage is None:
        if not regions:
            raise EngineError("region_canvases: no regions")
        stage, group = RegionStage([regions], regions[0].page.device), 0
    n = len(stage.groups[group])
    gh, gw = int(group_hw[0]), int(group_hw[1])
    dev = stage.dev.device
    if n < 1 or gh < 1 or gw < 1 or not all(r.page.is_cuda and r.page.device == dev for r in stage.groups[group]):
        raise EngineError("region_canvases: needs at least one region, a canvas of at least 1 x 1 and pages on the staging device")
    canv = torch.empty((n, gh, gw, 3), dtype=torch.uint8, device=dev)
    det = torch.empty((n, gh, gw, 3), dtype=torch.uint8, device=dev) if want_masked else None
    ws_bytes = int(lib.rd_region_canvases_workspace(n, gh, gw)) if stage.any_poly[group] else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    rc = lib.rd_region_canvases(dev.index or 0, stage.descs_ptr + REGION_DESC_DTYPE.itemsize * stage.firsts[group], n, stage.pts_ptr, stage.boxes_ptr,
                                gh, gw, canv.data_ptr(), det.data_ptr() if det is not None else None, ws.data_ptr() if ws is not None else None,
                                ws_bytes, _stream_ptr())
    if rc != 0:
        raise EngineError(lib.rd_create_error().decode())
    return canv, det
