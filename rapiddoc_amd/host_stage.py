"""Host images behind the plugin seam: the numpy crops an unmodified RapidDoc hands to a `custom_model` go to the device ONCE.

  plan_offsets        where every image lies in the staging buffer: 16-byte aligned, in order, zero-area images take no bytes (host only)
  pack_images         rd_stage_pack: the images' rows gathered into a caller's buffer at those offsets, on up to 16 threads (host only)
  HostImageStage      one pinned buffer and one device buffer, grown geometrically and re-used: `upload(images)` packs, then ONE
                      asynchronous host-to-device copy on the current stream; the result's `views[i]` is the device uint8 [h, w, 3] image
  pack_stage_descs    the rd_stage_desc array of every crop of every size group of a call (host only)
  stage_canvases      rd_stage_canvases: the white-padded canvases of all size groups in ONE launch

Users: analyze.RegionTextModel(host_images="stage") and formula_host.FormulaRecognizer(host_images="stage"); docs/notebook/plugin_seams.md
has the measurement."""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np

from . import _lib

ALIGN = 16
SWAP_RB = 1                                                                                                   # RD_STAGE_SWAP_RB
STAGE_DESC_DTYPE = np.dtype([("src", "<u8"), ("pitch", "<i8"), ("canvas", "<u8"), ("w", "<i4"), ("h", "<i4"), ("gh", "<i4"), ("gw", "<i4"),
                             ("flags", "<u4"), ("reserved", "<u4")])                                          # rd_stage_desc
MAX_THREADS = 16


class StageError(RuntimeError):
    pass


def as_stage_image(im) -> np.ndarray:
    """The array rd_stage_pack takes for `im`: uint8 [h, w, 3], channels 1 byte apart, pixels 3 bytes apart, rows at a pitch of at least
    3 * w - a window of a larger array stays a view; anything else (other dtypes, negative or permuted strides) is made contiguous."""
    a = np.asarray(im)
    if a.ndim != 3 or a.shape[2] != 3:
        raise StageError(f"a staged image must be [h, w, 3], got shape {a.shape}")
    if a.dtype != np.uint8:
        a = a.astype(np.uint8)
    h, w = a.shape[:2]
    if a.size and not (a.strides[2] == 1 and (w == 1 or a.strides[1] == 3) and (h == 1 or a.strides[0] >= 3 * w)):
        a = np.ascontiguousarray(a)
    return a


def plan_offsets(shapes: Sequence[Tuple[int, int]]) -> Tuple[List[int], int]:
    """(offset of every [h, w, 3] image, bytes of the buffer): offsets are multiples of 16 and ascending, images do not overlap, an image
    without pixels takes no bytes (its offset is where the next one starts)."""
    offs, n = [], 0
    for h, w in shapes:
        offs.append(n)
        n += (3 * int(h) * int(w) + ALIGN - 1) // ALIGN * ALIGN
    return offs, n


def pack_images(images: Sequence[np.ndarray], offsets: Sequence[int], dst_ptr: int, dst_bytes: int, n_threads: int = MAX_THREADS) -> None:
    """rd_stage_pack on arrays `as_stage_image` returned.  Bad arguments raise StageError; nothing is written then."""
    n = len(images)
    srcs = np.asarray([im.ctypes.data if im.size else 0 for im in images], dtype=np.uint64)
    pitches = np.asarray([im.strides[0] if im.shape[0] > 1 else 3 * im.shape[1] for im in images], dtype=np.int64)
    hs = np.asarray([im.shape[0] for im in images], dtype=np.int32)
    ws = np.asarray([im.shape[1] for im in images], dtype=np.int32)
    offs = np.asarray(offsets, dtype=np.int64)
    if len(offs) != n:
        raise StageError("one offset per image")
    rc = _lib.load().rd_stage_pack(srcs.ctypes.data, pitches.ctypes.data, hs.ctypes.data, ws.ctypes.data, offs.ctypes.data, n, dst_ptr,
                                   C.c_int64(int(dst_bytes)), int(n_threads))
    if rc != 0:
        raise StageError("rd_stage_pack: bad arguments (a NULL pointer, a negative size or offset, or an image that overruns the buffer)")


class Staged(NamedTuple):
    """One upload: `views[i]` the device uint8 [h_i, w_i, 3] image (a view into the stage's device buffer, valid until the stage's next
    upload), `offsets[i]` its byte offset from `base` (the buffer's device address), `shapes[i]` = (h_i, w_i)."""
    views: list
    offsets: List[int]
    shapes: List[Tuple[int, int]]
    base: int


class HostImageStage:
    """Host images -> device, one copy per call.

        stage = HostImageStage(device)
        staged = stage.upload(images)          # pack into the pinned buffer, ONE asynchronous copy on the current stream
        ... enqueue everything that reads staged.views ...
        stage.release()                        # the point behind the last consumer; the next upload waits for it

    Both buffers are re-used by the next upload and grow geometrically.  The pinned buffer is written by the HOST, so `upload` waits (on
    the host) for the event of the previous upload before it overwrites anything: the event `release` recorded behind the last consumer
    or, without a release, the one recorded right behind the copy (enough for consumers on the upload's stream, which the next copy is
    ordered behind anyway)."""

    def __init__(self, device, n_threads: int = MAX_THREADS):
        import torch
        self.tdev = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
        self.n_threads = int(n_threads)
        self._pin = None
        self._dev = None
        self._event = None
        self.uploads = 0

    def upload(self, images: Sequence, tail_bytes: int = 0) -> Staged:
        """`tail_bytes`: room the device buffer keeps BEHIND the uploaded images (from byte `sum of the aligned image sizes` on) for what
        the consumer writes next to them - ocr_model's warped line crops, addressed from the same base as the uploaded ones."""
        import torch
        arrs = [as_stage_image(im) for im in images]
        shapes = [(int(a.shape[0]), int(a.shape[1])) for a in arrs]
        offsets, total = plan_offsets(shapes)
        if self._event is not None:
            self._event.synchronize()                                     # the previous upload has left the pinned buffer and been consumed
            self._event = None
        if self._pin is None or self._pin.numel() < total:
            grown = max(total, 2 * (self._pin.numel() if self._pin is not None else 0), 1 << 16)
            self._pin = torch.empty(grown, dtype=torch.uint8, pin_memory=True)
            self._dev = torch.empty(max(grown, total + int(tail_bytes)), dtype=torch.uint8, device=self.tdev)
        elif self._dev.numel() < total + int(tail_bytes):
            self._dev = torch.empty(max(total + int(tail_bytes), 2 * self._dev.numel()), dtype=torch.uint8, device=self.tdev)
        pack_images(arrs, offsets, self._pin.data_ptr(), total, self.n_threads)
        if total:
            self._dev[:total].copy_(self._pin[:total], non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record(torch.cuda.current_stream(self.tdev))
        self.uploads += 1
        views = [self._dev[o: o + 3 * h * w].view(h, w, 3) for o, (h, w) in zip(offsets, shapes)]
        return Staged(views, offsets, shapes, self._dev.data_ptr())

    def release(self) -> None:
        """Call after the work that reads the last upload's views has been enqueued on the current stream."""
        import torch
        self._event = torch.cuda.Event()
        self._event.record(torch.cuda.current_stream(self.tdev))


def pack_stage_descs(base: int, offsets: Sequence[int], shapes: Sequence[Tuple[int, int]], groups: Sequence[Tuple[Tuple[int, int], Sequence[int]]],
                     canvas_ptrs: Sequence[int], swap_rb: bool = True) -> np.ndarray:
    """Host only: one rd_stage_desc per member of every size group, group after group.  `base` / `offsets` / `shapes`: a `Staged`'s;
    `groups[g]` = ((gh, gw), indices into the upload); `canvas_ptrs[g]` = device address of group g's [len, gh, gw, 3] canvas array."""
    descs = np.zeros(sum(len(m) for _hw, m in groups), dtype=STAGE_DESC_DTYPE)
    k = 0
    for ((gh, gw), members), canvas in zip(groups, canvas_ptrs):
        for j, i in enumerate(members):
            h, w = shapes[i]
            descs[k] = (int(base) + int(offsets[i]), 3 * w, int(canvas) + j * gh * gw * 3, w, h, gh, gw, SWAP_RB if swap_rb else 0, 0)
            k += 1
    return descs


def launch_stage_canvases(descs: np.ndarray, device) -> None:
    """rd_stage_canvases on a descriptor array: its device copy is uploaded here (pinned, asynchronous, current stream).  Bad arguments
    raise StageError; nothing is launched then."""
    import torch
    lib = _lib.load()
    descs = np.ascontiguousarray(descs, dtype=STAGE_DESC_DTYPE)
    host = torch.empty(max(descs.nbytes, 16), dtype=torch.uint8, pin_memory=True)
    host[: descs.nbytes] = torch.from_numpy(descs.view(np.uint8).reshape(-1))
    dev = host.to(device, non_blocking=True)
    rc = lib.rd_stage_canvases(device.index or 0, descs.ctypes.data, dev.data_ptr(), len(descs), torch.cuda.current_stream(device).cuda_stream)
    if rc != 0:
        raise StageError(lib.rd_create_error().decode())


def stage_canvases(staged: Staged, groups: Sequence[Tuple[Tuple[int, int], Sequence[int]]], swap_rb: bool = True) -> list:
    """The canvases of every size group - uint8 [len(members), gh, gw, 3], white, member j's image at (0, 0) of canvas j, channels reversed
    when `swap_rb` - composed from one upload by ONE rd_stage_canvases launch on the current stream."""
    import torch
    if not groups:
        return []
    device = staged.views[0].device
    canvases = [torch.empty((len(members), gh, gw, 3), dtype=torch.uint8, device=device) for (gh, gw), members in groups]
    descs = pack_stage_descs(staged.base, staged.offsets, staged.shapes, groups, [c.data_ptr() for c in canvases], swap_rb)
    launch_stage_canvases(descs, device)
    return canvases
