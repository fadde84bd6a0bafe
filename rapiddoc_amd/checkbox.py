"""Checkbox detection on the GPU: the reference's `checkbox_predict` (rapid_doc/utils/checkbox_det_cls.py, called at batch_analyze.py:
207-219 under checkbox_config["checkbox_enable"]) for a page batch that already lives on the device.

    box = Mi355Checkbox(device=0)
    PageAnalyzer(..., checkbox_fn=box, checkbox_enable=True)        # receives the page tensor itself, once per batch
    box.detect_pages(pages_rgb_dev)                                 # [P, H, W, 3] uint8 CUDA tensor -> per page the reference's dicts
    box(bgr_numpy)                                                  # the reference's own call shape; uploads the page

The image work runs in csrc/kernels_checkbox.hip (rd_checkbox_detect_device), the size filter, the contour rule, the classification and
the ordering in csrc/checkbox_host.cpp (rd_checkbox_finish).  Per batch two device-to-host copies: 32 bytes a page, then 584 bytes a
candidate (`last_d2h_bytes`).  A page that overflows its run or candidate buffer is repeated alone with the worst-case bound; the
result is the same.  docs/notebook/checkbox.md has the routes and the list of what is restated from OpenCV and not pinned."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .engine import EngineError, _stream_ptr

MAX_SIDE = 16384                      # RD_CHECKBOX_MAX_SIDE
ROI_ROWS = 70                         # RD_CHECKBOX_ROI_ROWS
WS_PARTS = 13                         # RD_CHECKBOX_WS_PARTS
RUNS_OVERFLOW, CANDS_OVERFLOW = 1, 2
PAGE_DTYPE = np.dtype([(n, "<i4") for n in ("n_runs", "flags", "n_comp", "n_cand", "first_key", "cand_off", "r0", "r1")])           # rd_checkbox_page
CAND_DTYPE = np.dtype([("key", "<i4"), ("tick", "<i4")] + [(n, "<i2") for n in ("x", "y", "w", "h", "rx", "ry", "rw", "rh")] +
                      [("roi", "<u8", (ROI_ROWS,))])                                                                                # rd_checkbox_cand
BOX_DTYPE = np.dtype([(n, "<i4") for n in ("x", "y", "w", "h", "ticked")])                                                           # rd_checkbox_box
WS_PART_NAMES = ("bin", "lines", "final", "row_cnt", "row_off", "runs", "parent", "key", "minx", "maxx", "miny", "maxy", "stage")


def default_max_runs(H: int, W: int) -> int:
    """runs of the complement of the line mask a page may hold before it is repeated with the worst case: sixteen a row"""
    return min(worst_case_runs(H, W), max(4096, 16 * H))


def worst_case_runs(H: int, W: int) -> int:
    return H * ((W + 1) // 2)


def workspace(P: int, H: int, W: int, max_runs: int, max_cand: int) -> Tuple[int, Dict[str, int]]:
    """bytes of device scratch and the byte offset of every part (rd_checkbox_workspace)"""
    offs = (C.c_size_t * WS_PARTS)()
    n = _lib.load().rd_checkbox_workspace(P, H, W, max_runs, max_cand, offs)
    if n == 0:
        raise EngineError(f"rd_checkbox_workspace: P = {P}, H = {H}, W = {W}, max_runs = {max_runs}, max_cand = {max_cand} is outside the bounds")
    return int(n), dict(zip(WS_PART_NAMES, (int(o) for o in offs)))


def run_device(pages: torch.Tensor, bgr: bool, max_runs: int, max_cand: int, ws: Optional[torch.Tensor] = None,
               hdr: Optional[torch.Tensor] = None, cands: Optional[torch.Tensor] = None):
    """Every kernel of the stage on the current stream, nothing copied: pages [P, H, W, 3] uint8 on the device -> (ws, hdr, cands), all
    uint8 device tensors (PAGE_DTYPE [P], CAND_DTYPE [P * max_cand]).  Buffers the caller hands in are used as they are."""
    if not (isinstance(pages, torch.Tensor) and pages.is_cuda and pages.dtype == torch.uint8 and pages.dim() == 4 and pages.shape[3] == 3):
        raise EngineError("checkbox detection takes a [P, H, W, 3] uint8 tensor on the device")
    pages = pages.contiguous()
    P, H, W, _ = (int(v) for v in pages.shape)
    nbytes, _offs = workspace(P, H, W, max_runs, max_cand)
    dev = pages.device
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if hdr is None:
        hdr = torch.empty(P * PAGE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    if cands is None:
        cands = torch.empty(P * max_cand * CAND_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    lib = _lib.load()
    rc = lib.rd_checkbox_detect_device(dev.index or 0, pages.data_ptr(), P, H, W, 1 if bgr else 0, max_runs, max_cand, ws.data_ptr(), ws.numel(),
                                       hdr.data_ptr(), cands.data_ptr(), _stream_ptr())
    if rc != 0:
        raise EngineError(lib.rd_create_error().decode())
    return ws, hdr, cands


def finish(records: np.ndarray, H: int, W: int) -> List[dict]:
    """one page's records (CAND_DTYPE, host) -> the reference's result list (rd_checkbox_finish; needs no GPU)"""
    records = np.ascontiguousarray(records, dtype=CAND_DTYPE)
    n = len(records)
    out = np.zeros(max(n, 1), dtype=BOX_DTYPE)
    n_out = C.c_int32(0)
    lib = _lib.load()
    rc = lib.rd_checkbox_finish(records.ctypes.data if n else None, n, H, W, out.ctypes.data, len(out), C.byref(n_out))
    if rc != 0:
        raise EngineError(lib.rd_create_error().decode())
    res = []
    for b in out[:n_out.value]:
        x, y, w, h = int(b["x"]), int(b["y"]), int(b["w"]), int(b["h"])
        res.append({"bbox": [x, y, x + w, y + h], "label": "Ticked" if b["ticked"] else "Unticked", "text": "☑" if b["ticked"] else "☐"})
    return res


class Mi355Checkbox:
    """`checkbox_fn` of analyze.PageAnalyzer that works on the device-resident page batch."""
    accepts_device_pages = True

    def __init__(self, device=0, max_runs: Optional[int] = None, max_cand: int = 256):
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.max_runs, self.max_cand = max_runs, max_cand
        self.last_d2h_bytes = 0
        self.last_records: List[np.ndarray] = []          # per page the device's records (CAND_DTYPE), for tests and tools
        self.last_headers: Optional[np.ndarray] = None    # PAGE_DTYPE [P] of the first pass (overflow flags as the device raised them)
        self._ws: Dict[tuple, torch.Tensor] = {}

    def _records(self, pages: torch.Tensor, bgr: bool, max_runs: int, max_cand: int):
        P, H, W, _ = (int(v) for v in pages.shape)
        key = (P, H, W, max_runs, max_cand)
        ws = self._ws.get(key)
        if ws is None:
            self._ws.clear()                               # one shape at a time: a page stream has one size
            ws = self._ws[key] = torch.empty(workspace(*key)[0], dtype=torch.uint8, device=pages.device)
        _ws, hdr_dev, cands_dev = run_device(pages, bgr, max_runs, max_cand, ws=ws)
        hdr = hdr_dev.cpu().numpy().view(PAGE_DTYPE)                                               # copy 1: 32 bytes a page
        total = int(np.minimum(hdr["n_cand"], max_cand).sum())
        recs = cands_dev[:total * CAND_DTYPE.itemsize].cpu().numpy().view(CAND_DTYPE) if total else np.zeros(0, CAND_DTYPE)   # copy 2
        self.last_d2h_bytes += hdr.nbytes + recs.nbytes
        return hdr, recs

    def _detect(self, pages: torch.Tensor, bgr: bool) -> List[List[dict]]:
        P, H, W, _ = (int(v) for v in pages.shape)
        if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
            raise EngineError(f"checkbox detection: page of {H} x {W} pixels, the bound is {MAX_SIDE}")
        self.last_d2h_bytes = 0
        max_runs = self.max_runs or default_max_runs(H, W)
        hdr, recs = self._records(pages, bgr, max_runs, self.max_cand)
        self.last_headers = hdr.copy()
        per_page = []
        for p in range(P):
            h = hdr[p]
            if h["flags"]:                                 # never silent: the page again, alone, with the worst-case bounds
                mr = worst_case_runs(H, W) if h["flags"] & RUNS_OVERFLOW else max_runs
                h2, r2 = self._records(pages[p:p + 1], bgr, mr, self.max_cand)
                if h2[0]["flags"] & CANDS_OVERFLOW:
                    h2, r2 = self._records(pages[p:p + 1], bgr, mr, int(h2[0]["n_cand"]))
                if h2[0]["flags"]:
                    raise EngineError(f"checkbox detection: page {p} still overflows with the worst-case bounds (flags {int(h2[0]['flags'])})")
                per_page.append(r2)
            else:
                per_page.append(recs[h["cand_off"]:h["cand_off"] + h["n_cand"]])
        self.last_records = per_page
        return [finish(r, H, W) for r in per_page]

    def detect_pages(self, pages_rgb_dev: torch.Tensor) -> List[List[dict]]:
        """[P, H, W, 3] uint8 RGB pages on the device -> per page the list `checkbox_predict` returns for that page"""
        return self._detect(pages_rgb_dev.contiguous(), bgr=False)

    def __call__(self, bgr: np.ndarray) -> List[dict]:
        """the reference's call: one BGR page as a numpy array (uploaded)"""
        page = torch.from_numpy(np.ascontiguousarray(bgr)).to(self.device)
        return self._detect(page[None], bgr=True)[0]
