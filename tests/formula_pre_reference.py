"""Test helpers of the device formula pre-process: a numpy restatement of what `formula_host.decode_image` asks of Pillow (convert("L"),
Image.resize(BILINEAR), Image.thumbnail = round_aspect + reduce + BICUBIC over a float32 box, ImageOps.expand), the Python arithmetic
`rd_formula_preproc_plan` has to equal, and the loaders of the fixtures tests/golden/make_golden_formula_pre_device.py writes.  Python floats
are IEEE doubles and nothing here is fused or reassociated, so the tables are the ones Pillow computes."""
import json
import math
import zlib

import numpy as np

PRECISION_BITS = 22
SIDE = 384
MAX_SIDE = 16384                       # RD_RESIZE_AA_MAX_SIDE
BILINEAR, BICUBIC = 2, 3               # Pillow's numbering, RD_RESAMPLE_*

# (h, w) of the margin BOX of every fixture crop, in the order of the fixture file; None = the uniform patch (the whole crop is kept)
BOX_SIZES = [(60, 400), (37, 291), (100, 1000), (700, 9), (23, 157), (11, 1201), (301, 64), (200, 90), (50, 51), (13, 17), (50, 50), (401, 400),
             (1, 1), (1, 40), None, (5, 700), (3, 2000), (640, 16)]
# (700, 9) and (11, 1201) exercise factors 38 and a final height of 4, but their bilinear intermediates (384 x 29866, 41925 x 384) lie beyond
# MAX_SIDE like those of (5, 700) and (3, 2000): all four take the host route.  (640, 16) is the tall, large-factor case inside the bound
# (384 x 15360, factors 20 / 20), (1, 40) the flat one.
HOST_ROUTE_BOXES = {(700, 9), (11, 1201), (5, 700), (3, 2000)}
UNIFORM_HW = (33, 47)


# ---------------------------------------------------------------------------------------------------------------- the plan
def _round_aspect(number, key):
    return max(min(math.floor(number), math.ceil(number), key=key), 1)


def plan(w: int, h: int) -> dict:
    """everything that follows from a margin box of w x h pixels, as formula_host.decode_image and Pillow's Image.thumbnail /
    Image.resize(reducing_gap=2.0) compute it"""
    if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
        return {"served": 0}
    short, long_ = (w, h) if w <= h else (h, w)
    new_long = int(SIDE * long_ / short)
    W, H = (SIDE, new_long) if w <= h else (new_long, SIDE)
    p = {"resize_w": W, "resize_h": H, "thumb": int(W > SIDE or H > SIDE), "final_w": W, "final_h": H, "fx": 1, "fy": 1, "reduced_w": W,
         "reduced_h": H, "box_w": np.float32(W), "box_h": np.float32(H)}
    if p["thumb"]:
        x, y = SIDE, SIDE
        aspect = W / H
        if x / y >= aspect:
            x = _round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
        else:
            y = _round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
        fx, fy = int(W / x / 2.0) or 1, int(H / y / 2.0) or 1
        p.update(final_w=x, final_h=y, fx=fx, fy=fy)
        if fx > 1 or fy > 1:
            p.update(reduced_w=-(-W // fx), reduced_h=-(-H // fy), box_w=np.float32(W / fx), box_h=np.float32(H / fy))
    p["pad_x"], p["pad_y"] = (SIDE - p["final_w"]) // 2, (SIDE - p["final_h"]) // 2
    p["served"] = int(W <= MAX_SIDE and H <= MAX_SIDE)
    return p


PLAN_FIELDS = ("served", "resize_w", "resize_h", "thumb", "final_w", "final_h", "fx", "fy", "reduced_w", "reduced_h", "box_w", "box_h", "pad_x", "pad_y")


# ---------------------------------------------------------------------------------------------------------------- the resampler
def resample_coeffs(kind: int, n_in: int, box0: float, box1: float, n_out: int):
    """(bounds int32 [n_out, 2] = (first source index, taps), kk int32 [n_out, ksize], ksize) of one axis: Resample.c precompute_coeffs +
    normalize_coeffs_8bpc.  All outputs at once in float64 arrays: every element sees the scalar operations in Pillow's order, the
    weights are summed tap by tap from the left."""
    scale = (box1 - box0) / n_out
    fs = max(scale, 1.0)
    support = (2.0 if kind == BICUBIC else 1.0) * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = box0 + (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in) - xmin
    w = np.zeros((n_out, ksize), dtype=np.float64)
    total = np.zeros(n_out, dtype=np.float64)
    for x in range(ksize):
        t = np.abs((x + xmin - center + 0.5) * ss)
        if kind == BICUBIC:
            a = -0.5
            v = np.where(t < 1.0, ((a + 2.0) * t - (a + 3.0)) * t * t + 1, np.where(t < 2.0, (((t - 5) * t + 8) * t - 4) * a, 0.0))
        else:
            v = np.where(t < 1.0, 1.0 - t, 0.0)
        v = np.where(x < xmax, v, 0.0)
        w[:, x] = v
        total = np.where(x < xmax, total + v, total)
    w = np.where((total != 0.0)[:, None], w / np.where(total != 0.0, total, 1.0)[:, None], w)
    kk = np.where(w < 0, np.trunc(-0.5 + w * (1 << PRECISION_BITS)), np.trunc(0.5 + w * (1 << PRECISION_BITS))).astype(np.int32)
    kk[np.arange(ksize)[None, :] >= xmax[:, None]] = 0
    return np.stack([xmin, xmax], axis=1).astype(np.int32), kk, ksize


def _pass(img: np.ndarray, kind: int, box1: float, n_out: int) -> np.ndarray:
    """one pass along axis 0 of img [n_in, ...] uint8 over the box [0, box1); tap by tap over all outputs, a slab of columns at a time"""
    bounds, kk, ksize = resample_coeffs(kind, img.shape[0], 0.0, float(box1), n_out)
    lo, cnt = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    flat = img.reshape(img.shape[0], -1)
    out = np.empty((n_out, flat.shape[1]), dtype=np.uint8)
    step = max(1, (1 << 22) // n_out)
    for c0 in range(0, flat.shape[1], step):
        src = flat[:, c0: c0 + step].astype(np.int64)
        acc = np.full((n_out, src.shape[1]), 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for t in range(ksize):
            acc += np.where((t < cnt)[:, None], kk[:, t].astype(np.int64)[:, None] * src[np.minimum(lo + t, img.shape[0] - 1)], 0)
        assert int(np.abs(acc).max()) < 2 ** 31               # what the device holds in int32
        out[:, c0: c0 + step] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out.reshape((n_out,) + img.shape[1:])


def resample(img: np.ndarray, kind: int, ow: int, oh: int, box_w=None, box_h=None) -> np.ndarray:
    """img [H, W, C] uint8 -> [oh, ow, C]: horizontal pass, then vertical; a pass whose in == out over the full box does not run"""
    h, w = img.shape[:2]
    box_w, box_h = (w if box_w is None else box_w), (h if box_h is None else box_h)
    if w != ow or box_w != w:
        img = np.ascontiguousarray(_pass(np.ascontiguousarray(img.transpose(1, 0, 2)), kind, box_w, ow).transpose(1, 0, 2))
    if h != oh or box_h != h:
        img = _pass(img, kind, box_h, oh)
    return np.ascontiguousarray(img)


def reduce(img: np.ndarray, fx: int, fy: int) -> np.ndarray:
    """Image.reduce((fx, fy)) over the full image: a cell of n pixels (the last row and column hold fewer) is
    ((sum + n // 2) * int(2^32 / (256 n))) >> 24"""
    h, w = img.shape[:2]
    ys, xs = np.arange(0, h, fy), np.arange(0, w, fx)
    sums = np.add.reduceat(np.add.reduceat(img.astype(np.int64), ys, axis=0), xs, axis=1)
    n = np.outer(np.minimum(ys + fy, h) - ys, np.minimum(xs + fx, w) - xs)[..., None]
    m = ((1 << 32) / (256 * n)).astype(np.int64)              # int(2^32 / (256 n)): a double division, truncated
    v = (sums + n // 2) * m
    assert int(v.max()) < 2 ** 32                              # what the device holds in uint32
    return (v >> 24).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the pipeline
def grey_l(img: np.ndarray) -> np.ndarray:
    """Pillow's convert("L") of an RGB uint8 image"""
    a = img.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.int64)


def margin_box(img: np.ndarray):
    """(x0, y0, x1, y1) of formula_host._crop_margin, in integers"""
    L = grey_l(img)
    mn, mx = int(L.min()), int(L.max())
    if mx == mn:
        return 0, 0, img.shape[1], img.shape[0]
    ys, xs = np.nonzero((L - mn) * 255 < 200 * (mx - mn))
    return int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1


def decode(img: np.ndarray) -> np.ndarray:
    """uint8 [H, W, 3] -> uint8 [384, 384, 3]: formula_host.decode_image without Pillow"""
    x0, y0, x1, y1 = margin_box(img)
    p = plan(x1 - x0, y1 - y0)
    cur = resample(np.ascontiguousarray(img[y0:y1, x0:x1]), BILINEAR, p["resize_w"], p["resize_h"])
    if p["thumb"]:
        if p["fx"] > 1 or p["fy"] > 1:
            cur = reduce(cur, p["fx"], p["fy"])
        cur = resample(cur, BICUBIC, p["final_w"], p["final_h"], float(p["box_w"]), float(p["box_h"]))
    out = np.zeros((SIDE, SIDE, 3), dtype=np.uint8)
    out[p["pad_y"]: p["pad_y"] + cur.shape[0], p["pad_x"]: p["pad_x"] + cur.shape[1]] = cur
    return out


# ---------------------------------------------------------------------------------------------------------------- the fixtures
def make_crop(seed: int, box_hw):
    """A light patch (225 .. 255) with dark strokes (< 90) whose bounding box is exactly box_hw = (h, w), at a seeded offset inside a crop
    with seeded margins; None: a uniform patch.  Returns the crop uint8 [H, W, 3]."""
    rng = np.random.default_rng(1000 + seed)
    if box_hw is None:
        return np.full(UNIFORM_HW + (3,), 180, np.uint8)
    bh, bw = box_hw
    top, left, bottom, right = (int(v) for v in rng.integers(0, 7, 4))
    img = rng.integers(225, 256, (top + bh + bottom, left + bw + right, 3)).astype(np.uint8)
    box = img[top: top + bh, left: left + bw]
    for _ in range(10):
        yy, xx = int(rng.integers(0, bh)), int(rng.integers(0, bw))
        hh, ww = int(rng.integers(1, max(2, bh // 3 + 1))), int(rng.integers(1, max(2, bw // 3 + 1)))
        box[yy: yy + hh, xx: xx + ww] = rng.integers(0, 90, 3).astype(np.uint8)
    dark = lambda: rng.integers(0, 90, 3).astype(np.uint8)
    box[0, int(rng.integers(0, bw))] = dark()                  # one dark pixel on every side of the box: its size is exact
    box[bh - 1, int(rng.integers(0, bw))] = dark()
    box[int(rng.integers(0, bh)), 0] = dark()
    box[int(rng.integers(0, bh)), bw - 1] = dark()
    return img


def crc(a) -> int:
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def load_cases(golden_dir):
    """[{name, crop u8 [H, W, 3], box (x0, y0, x1, y1), route, u8 [384, 384, 3], input_crc32}] of the fixture files"""
    meta = json.loads((golden_dir / "formula_pre_device.json").read_text())
    z = [np.load(golden_dir / f) for f in meta["files"]]
    out = []
    for i, c in enumerate(meta["cases"]):
        crop = make_crop(c["seed"], tuple(c["box_hw"]) if c["box_hw"] else None)
        assert crc(crop) == c["crop_crc32"], c["name"]
        out.append({"name": c["name"], "crop": crop, "box": tuple(c["box"]), "route": c["route"], "u8": z[c["file"]][f"u8_{i}"], "input_crc32": c["input_crc32"]})
    return out
