"""The yardstick of the checkbox stage: rapid_doc/utils/checkbox_det_cls.py `checkbox_predict` restated in numpy, literally.

cv2 is not installed here, so every OpenCV call of that file is restated from OpenCV 4.x's published algorithm (named at each function;
PARITY UNPINNED, docs/notebook/checkbox.md lists them).  Nothing here uses the identities the kernels use: erosions and dilations are
minima and maxima over the structuring element, the closings are computed, components come from a union-find over pixel runs.
`fake_cv2()` offers the same functions under cv2's names so that tests/golden/make_golden_checkbox.py can run the reference's own file
on them.  No scipy at test time."""
import types
from collections import Counter

import numpy as np

# ------------------------------------------------------------------------------------------------------------------ colour, threshold

def bgr2gray(img):
    """cv2.cvtColor(BGR2GRAY) for u8: 15-bit fixed point (B 3735, G 19235, R 9798), rounded"""
    b, g, r = (img[..., k].astype(np.int64) for k in range(3))
    return ((3735 * b + 19235 * g + 9798 * r + 16384) >> 15).astype(np.uint8)


def threshold_binary(gray, thresh, maxval):
    return np.where(gray > thresh, maxval, 0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ morphology
def _windows(img, kh, kw, border):
    """every shift of `img` under a kh x kw element anchored at its centre, the outside filled with `border`"""
    ay, ax = kh // 2, kw // 2
    H, W = img.shape
    pad = np.full((H + kh - 1, W + kw - 1), border, np.uint8)
    pad[ay:ay + H, ax:ax + W] = img
    return [pad[dy:dy + H, dx:dx + W] for dy in range(kh) for dx in range(kw)]


def erode(img, kh, kw):
    """cv2.erode, rectangular element, default border: the outside never lowers the minimum"""
    return np.minimum.reduce(_windows(img, kh, kw, 255))


def dilate(img, kh, kw):
    """cv2.dilate, rectangular element, default border: the outside never raises the maximum"""
    return np.maximum.reduce(_windows(img, kh, kw, 0))


def morph_open(img, kh, kw):
    return dilate(erode(img, kh, kw), kh, kw)


def morph_close(img, kh, kw):
    return erode(dilate(img, kh, kw), kh, kw)


# ------------------------------------------------------------------------------------------------------------------ components
def _runs_of_row(row):
    d = np.diff(np.concatenate(([0], (row != 0).astype(np.int8), [0])))
    return np.flatnonzero(d == 1), np.flatnonzero(d == -1)        # [x0, x1)


def connected_components_with_stats(img):
    """cv2.connectedComponentsWithStats(img, connectivity=8, CV_32S) -> (n, labels, stats).  Label 0 is the zero pixels.  The others are
    numbered in the order OpenCV's block-based 8-connectivity labelers (BBDT / Spaghetti) hand out their first provisional labels, which
    flattenL keeps: ascending position, in block-raster order, of the component's first 2 x 2 block."""
    H, W = img.shape
    runs, parent = [], []
    prev = []

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for y in range(H):
        x0s, x1s = _runs_of_row(img[y])
        cur = []
        for x0, x1 in zip(x0s.tolist(), x1s.tolist()):
            i = len(runs)
            runs.append((y, x0, x1))
            parent.append(i)
            cur.append(i)
            for j in prev:                                    # 8-connected: [x0 - 1, x1 + 1) meets [px0, px1)
                _, px0, px1 = runs[j]
                if px0 < x1 + 1 and px1 > x0 - 1:
                    a, b = find(i), find(j)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
        prev = cur
    comps = {}
    for i, (y, x0, x1) in enumerate(runs):
        c = comps.setdefault(find(i), {"key": (1 << 30, 0), "x0": W, "x1": 0, "y0": H, "y1": 0, "area": 0, "runs": []})
        c["key"] = min(c["key"], (y // 2, x0 // 2))
        c["x0"], c["x1"] = min(c["x0"], x0), max(c["x1"], x1)
        c["y0"], c["y1"] = min(c["y0"], y), max(c["y1"], y + 1)
        c["area"] += x1 - x0
        c["runs"].append((y, x0, x1))
    ordered = sorted(comps.values(), key=lambda c: c["key"])
    labels = np.zeros((H, W), np.int32)
    stats = np.zeros((len(ordered) + 1, 5), np.int32)
    zero = img == 0
    if zero.any():
        ys, xs = np.nonzero(zero)
        stats[0] = (xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1, int(zero.sum()))
    for k, c in enumerate(ordered, 1):
        stats[k] = (c["x0"], c["y0"], c["x1"] - c["x0"], c["y1"] - c["y0"], c["area"])
        for y, x0, x1 in c["runs"]:
            labels[y, x0:x1] = k
    return len(ordered) + 1, labels, stats


def block_key(stats_row, labels, k):
    """the label-order key the device reports for component k: (y // 2) << 16 | x // 2 of its first 2 x 2 block"""
    ys, xs = np.nonzero(labels == k)
    return min(((int(y) // 2) << 16) | (int(x) // 2) for y, x in zip(ys, xs))


# ------------------------------------------------------------------------------------------------------------------ contours
_DX = (1, 1, 0, -1, -1, -1, 0, 1)          # OpenCV's 8-neighbour codes: 0 = E, 1 = NE, 2 = N, ... counter-clockwise, y down
_DY = (0, -1, -1, -1, 0, 1, 1, 1)


def _trace_outer_border(img, x0, y0):
    """Suzuki-Abe border following as OpenCV's contour fetcher walks an outer border, CHAIN_APPROX_NONE: the current point is written at
    every step."""
    H, W = img.shape

    def at(x, y):
        return 0 <= x < W and 0 <= y < H and img[y, x] != 0

    s = 4
    while True:
        s = (s - 1) & 7
        x1, y1 = x0 + _DX[s], y0 + _DY[s]
        if at(x1, y1) or s == 4:
            break
    if s == 4:
        return [(x0, y0)]
    out = []
    x3, y3 = x0, y0
    while True:
        while True:
            s += 1
            x4, y4 = x3 + _DX[s & 7], y3 + _DY[s & 7]
            if at(x4, y4):
                break
        s &= 7
        out.append((x3, y3))
        if (x4, y4) == (x0, y0) and (x3, y3) == (x1, y1):
            break
        x3, y3 = x4, y4
        s = (s + 4) & 7
    return out


def find_contours_external_none(img):
    """cv2.findContours(img, RETR_EXTERNAL, CHAIN_APPROX_NONE) -> list of [n, 1, 2] int32 (x, y), last found first.  External: the
    component's first pixel in raster order has the image frame, or background that is 4-connected to the frame, on its west."""
    img = np.asarray(img)
    H, W = img.shape
    fg = img != 0
    outside = np.zeros((H, W), bool)                       # background reached from the frame
    stack = [(y, x) for y in range(H) for x in (0, W - 1)] + [(y, x) for x in range(W) for y in (0, H - 1)]
    while stack:
        y, x = stack.pop()
        if not (0 <= y < H and 0 <= x < W) or fg[y, x] or outside[y, x]:
            continue
        outside[y, x] = True
        stack.extend(((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)))
    _n, labels, _stats = connected_components_with_stats(fg.astype(np.uint8))
    seen, found = set(), []
    for y in range(H):
        for x in np.flatnonzero(fg[y]).tolist():
            k = int(labels[y, x])
            if k in seen:
                continue
            seen.add(k)
            if x == 0 or outside[y, x - 1]:
                found.append(np.array(_trace_outer_border(img, x, y), np.int32).reshape(-1, 1, 2))
    return found[::-1]


# ------------------------------------------------------------------------------------------------------------------ the tick chain
def gaussian_blur5_u8(gray):
    """cv2.GaussianBlur(u8, (5, 5), 0): the fixed-point path, taps [1 4 6 4 1] / 16 on both axes, (S + 128) >> 8, BORDER_REFLECT_101"""
    k = np.array([1, 4, 6, 4, 1], np.int64)
    p = np.pad(gray.astype(np.int64), 2, mode="reflect")
    H, W = gray.shape
    rows = sum(k[d] * p[:, d:d + W] for d in range(5))
    S = sum(k[d] * rows[d:d + H, :] for d in range(5))
    return ((S + 128) >> 8).astype(np.uint8)


def mean_taps_f32():
    """getGaussianKernel(11, 2.0): exp(-(i - 5)^2 / (2 sigma^2)) normalised in double, then float32"""
    k = np.exp(-((np.arange(11) - 5.0) ** 2) / 8.0)
    return (k / k.sum()).astype(np.float32)


def adaptive_mean_gauss11(gray):
    """the `mean` image of cv2.adaptiveThreshold(ADAPTIVE_THRESH_GAUSSIAN_C, blockSize 11): the float32 image under the separable 11-tap
    Gaussian, BORDER_REPLICATE, rows then columns, each as the symmetric filter sums it - s = k0 x0; s += kj (x-j + xj) in float32 -
    rounded half-even to u8"""
    k = mean_taps_f32()
    H, W = gray.shape

    def symm(p, axis, n):
        take = (lambda d: p[:, d:d + n]) if axis == 1 else (lambda d: p[d:d + n, :])
        s = k[5] * take(5)
        for j in range(1, 6):
            s = s + k[5 + j] * (take(5 - j) + take(5 + j))
        return s.astype(np.float32)

    f = gray.astype(np.float32)
    rows = symm(np.pad(f, ((0, 0), (5, 5)), mode="edge"), 1, W)
    cols = symm(np.pad(rows, ((5, 5), (0, 0)), mode="edge"), 0, H)
    return np.clip(np.rint(cols), 0, 255).astype(np.uint8)


def adaptive_threshold_gauss_inv(gray, max_value, block_size, c):
    assert block_size == 11 and c == 2
    mean = adaptive_mean_gauss11(gray)
    return np.where(gray.astype(np.int32) - mean.astype(np.int32) <= -2, max_value, 0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ the reference's two functions
def detect_checkboxes(bgr):
    """checkbox_det_cls.py:6-31 -> (stats, img_bin_final, parts)"""
    gray = bgr2gray(bgr)
    img_bin = ~threshold_binary(gray, 150, 255)
    open_h, open_v = morph_open(img_bin, 1, 15), morph_open(img_bin, 15, 1)
    close_h, close_v = morph_close(img_bin, 1, 15), morph_close(img_bin, 15, 1)
    lines = (open_h & close_h) | (open_v & close_v)
    final = dilate(lines, 3, 3)
    _n, labels, stats = connected_components_with_stats(~final)
    return stats, final, {"bin": img_bin, "lines": lines, "labels": labels}


def roi_rect(x, y, w, h, w_img, h_img):
    """:43-49 in Python's own float arithmetic"""
    new_x = max(int(x - w * 0.1), 0)
    new_y = max(int(y - h * 0.1), 0)
    new_w = min(int(w * (1 + 0.1 + 0.1)), w_img - new_x)
    new_h = min(int(h * (1 + 0.1 + 0.3)), h_img - new_y)
    return new_x, new_y, new_w, new_h


def contour_rule_keeps(roi):
    """:53-72; an ROI without a contour point makes the reference raise - the candidate is rejected here"""
    all_ys = [int(pt[0][1]) for c in find_contours_external_none(roi) for pt in c]
    if not all_ys:
        return False
    ranked = sorted(Counter(all_ys).items(), key=lambda t: (-t[1], t[0]))
    bottom_y = max(y for y, _c in ranked[:2])
    return not (max(all_ys) - bottom_y >= 0.9)


def tick_count(bgr, x, y, w, h):
    """:74-83"""
    g = gaussian_blur5_u8(bgr2gray(bgr[y:y + h, x:x + w]))
    return int(np.count_nonzero(morph_open(adaptive_threshold_gauss_inv(g, 255, 11, 2), 3, 3)))


def checkbox_trace(bgr):
    """everything the device must reproduce bit for bit: the three masks, every component's (key, x, y, w, h) in label order, and per
    candidate (after stats[2:] and the size filter) the ROI rectangle, the ROI bytes, the tick count and the verdict"""
    stats, final, parts = detect_checkboxes(bgr)
    H, W = final.shape
    comps = [(block_key(stats[k], parts["labels"], k), *(int(v) for v in stats[k][:4])) for k in range(1, len(stats))]
    cands, result = [], []
    for k in range(2, len(stats)):
        x, y, w, h = (int(v) for v in stats[k][:4])
        if not (12 <= w <= 50 and 12 <= h <= 50 and 0.9 <= w / h <= 1.1):
            continue
        rx, ry, rw, rh = roi_rect(x, y, w, h, W, H)
        roi = final[ry:ry + rh, rx:rx + rw].copy()
        keeps = contour_rule_keeps(roi)
        tick = tick_count(bgr, x, y, w, h)
        ticked = tick / (w * h) > 0.2
        cands.append({"key": comps[k - 1][0], "box": (x, y, w, h), "roi_rect": (rx, ry, rw, rh), "roi": roi, "tick": tick, "keeps": keeps,
                      "ticked": ticked})
        if keeps:
            result.append({"bbox": [x, y, x + w, y + h], "label": "Ticked" if ticked else "Unticked", "text": "☑" if ticked else "☐"})
    return {"bin": parts["bin"], "lines": parts["lines"], "final": final, "comps": comps, "cands": cands, "result": result}


def checkbox_predict(bgr):
    return checkbox_trace(bgr)["result"]


def pack_words(mask):
    """[H, W] mask -> uint64 [H, ceil(W / 64)], bit i of word j = pixel 64 j + i (the device's layout)"""
    H, W = mask.shape
    WW = (W + 63) // 64
    bits = np.zeros((H, WW * 64), np.uint8)
    bits[:, :W] = mask != 0
    return np.packbits(bits.reshape(H, WW, 8, 8), axis=-1, bitorder="little").reshape(H, WW, 8).copy().view("<u8").reshape(H, WW)


# ------------------------------------------------------------------------------------------------------------------ cv2's names
def fake_cv2():
    """a module with the cv2 names checkbox_det_cls.py uses, every one of them a function of this file"""
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_BGR2GRAY, cv2.THRESH_BINARY, cv2.MORPH_OPEN, cv2.MORPH_CLOSE = 6, 0, 2, 3
    cv2.CV_32S, cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_NONE, cv2.ADAPTIVE_THRESH_GAUSSIAN_C, cv2.THRESH_BINARY_INV = 4, 0, 1, 1, 1

    def cvt_color(img, code):
        assert code == cv2.COLOR_BGR2GRAY
        return bgr2gray(img)

    def threshold(img, thresh, maxval, kind):
        assert kind == cv2.THRESH_BINARY
        return float(thresh), threshold_binary(img, thresh, maxval)

    def morphology_ex(img, op, kernel):
        assert kernel.all()
        return (morph_open if op == cv2.MORPH_OPEN else morph_close)(img, *kernel.shape)

    def cv_dilate(img, kernel, iterations=1):
        assert kernel.all() and iterations == 1
        return dilate(img, *kernel.shape)

    def ccws(img, connectivity=8, ltype=None):
        assert connectivity == 8
        n, labels, stats = connected_components_with_stats(img)
        return n, labels, stats, None

    def find_contours(img, mode, method):
        assert mode == cv2.RETR_EXTERNAL and method == cv2.CHAIN_APPROX_NONE
        return tuple(find_contours_external_none(img)), None

    def gaussian_blur(img, ksize, sigma):
        assert tuple(ksize) == (5, 5) and sigma == 0
        return gaussian_blur5_u8(img)

    def adaptive_threshold(img, max_value, method, kind, block_size, c):
        assert method == cv2.ADAPTIVE_THRESH_GAUSSIAN_C and kind == cv2.THRESH_BINARY_INV
        return adaptive_threshold_gauss_inv(img, max_value, block_size, c)

    cv2.cvtColor, cv2.threshold, cv2.morphologyEx, cv2.dilate = cvt_color, threshold, morphology_ex, cv_dilate
    cv2.connectedComponentsWithStats, cv2.findContours = ccws, find_contours
    cv2.GaussianBlur, cv2.adaptiveThreshold, cv2.countNonZero = gaussian_blur, adaptive_threshold, lambda m: int(np.count_nonzero(m))
    return cv2


# ------------------------------------------------------------------------------------------------------------------ pages
def _hash32(a):
    """an integer hash (xorshift-multiply) of uint64 values, vectorised; results in [0, 2^32)"""
    with np.errstate(over="ignore"):                       # arithmetic modulo 2^64 is the point
        a = np.asarray(a, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        a = (a ^ (a >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        a = (a ^ (a >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        a = a ^ (a >> np.uint64(31))
    return (a & np.uint64(0xFFFFFFFF)).astype(np.int64)


def draw_box(img, x, y, side_w, side_h, t=2, ink=30):
    """a dark frame whose OUTER rectangle is [x, x + side_w) x [y, y + side_h), t pixels thick"""
    img[y:y + side_h, x:x + side_w] = ink
    img[y + t:y + side_h - t, x + t:x + side_w - t] = 255


def draw_tick(img, x, y, side, thick, ink=20, margin=5):
    """a cross of `thick`-pixel strokes inside the frame at (x, y)"""
    n = side - 2 * margin
    for i in range(n):
        for d in range(thick):
            for xx, yy in ((x + margin + i + d, y + margin + i), (x + side - margin - 1 - i - d, y + margin + i)):
                if x + 3 <= xx < x + side - 3:
                    img[yy, xx] = ink


def form_page(seed, H=1684, W=1191):
    """a seeded RGB form page from the integer hash alone: light paper with per-channel noise, a grid of boxes of hashed sizes (some
    ticked, some with a rule under them), short dark dashes that are no lines, and two long rules"""
    idx = np.arange(H * W * 3, dtype=np.uint64) + np.uint64(seed) * np.uint64(1 << 40)
    page = (232 + (_hash32(idx) % 20)).astype(np.uint8).reshape(H, W, 3)
    grey = np.full((H, W), 255, np.uint8)
    k = 0
    for gy in range(60, H - 90, 127):
        for gx in range(40, W - 90, 173):
            hv = int(_hash32(np.uint64(seed * 1000003 + k)))
            k += 1
            kind = hv % 8
            side = 14 + (hv >> 3) % 44
            sw = side + ((hv >> 10) % 5 - 2 if kind == 5 else 0)
            x, y = gx + (hv >> 14) % 23, gy + (hv >> 20) % 17
            if kind == 7:                                            # text-like dashes
                for d in range(6):
                    grey[y + 3 * d, x:x + 5 + (hv >> (d + 4)) % 9] = 40
                continue
            draw_box(grey, x, y, max(sw, 8), side, t=2 + (hv >> 24) % 2)
            if kind in (1, 2) and side >= 20:
                draw_tick(grey, x, y, side, 2 + (hv >> 26) % 3)
            if kind == 3:
                grey[y + side + 2:y + side + 4, x + side // 2:x + side + 14] = 30       # a rule right under the box
    grey[30:32, 20:W - 20] = 30
    grey[H - 40:H - 38, 100:W // 2] = 30
    dark = grey < 128
    page[dark] = grey[dark][:, None] + (page[dark] % 7)
    return page
