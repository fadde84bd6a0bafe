"""Test helpers of the table path: a numpy restatement of Pillow's 8-bit antialiased bilinear resample (Resample.c: precompute_coeffs,
normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc) and the loaders of the fixtures tests/golden/make_golden_table_path.py
writes.  Python floats are IEEE doubles and nothing here is fused or reassociated, so the tables are the ones Pillow computes."""
import json
import math

import numpy as np

PRECISION_BITS = 22
PIL_SHAPES = ((600, 1000), (64, 80), (300, 448), (448, 300), (448, 448), (100, 1200), (7, 2300), (1501, 449), (447, 2011), (120, 300))


def aa_coeffs(n_in: int, n_out: int):
    """(bounds int32 [n_out, 2] = (first source index, taps), kk int32 [n_out, ksize], ksize) of one axis"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs                               # Pillow multiplies by the reciprocal
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    kk = np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w, total = [], 0.0
        for x in range(xmax):
            v = max(1.0 - abs((x + xmin - center + 0.5) * ss), 0.0)
            w.append(v)
            total += v                          # left to right
        for x in range(xmax):
            v = w[x] / total if total != 0.0 else w[x]
            kk[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5)
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def _pass(img: np.ndarray, n_out: int) -> np.ndarray:
    """one pass along axis 0 of img [n_in, ...] uint8"""
    bounds, kk, _ = aa_coeffs(img.shape[0], n_out)
    src = img.astype(np.int64)
    out = np.empty((n_out,) + img.shape[1:], dtype=np.uint8)
    for i in range(n_out):
        lo, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[i, :n].astype(np.int64), src[lo:lo + n], axes=(0, 0))
        assert int(np.abs(acc).max()) < 2 ** 31               # what the device holds in int32
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_aa_u8(img: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """img [H, W, C] uint8 -> [oh, ow, C] uint8: the horizontal pass first, then the vertical one; a pass whose in == out does not run"""
    h, w = img.shape[:2]
    if w != ow:
        img = np.ascontiguousarray(_pass(np.ascontiguousarray(img.transpose(1, 0, 2)), ow).transpose(1, 0, 2))
    if h != oh:
        img = _pass(img, oh)
    return np.ascontiguousarray(img)


def lcg_bytes(seed: int, shape) -> np.ndarray:
    """uint8 noise of the tests' own: the high byte of a 64-bit LCG (Knuth's MMIX constants), wrapping integer arithmetic only"""
    n = int(np.prod(shape))
    out = np.empty(n, dtype=np.uint8)
    s = (seed * 0x9E3779B97F4A7C15 + 1) & (2 ** 64 - 1)
    for i in range(n):
        s = (s * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        out[i] = s >> 56
    return out.reshape(shape)


def load_summary(golden_dir) -> dict:
    return json.loads((golden_dir / "summary_table_path.json").read_text())


def resample_cases(golden_dir):
    """[(name, input u8 [H, W, 3], OH, OW, expected u8 [OH, OW, 3])] of table_path_resample.npz; an input that is not stored is
    weights.synth_table_crop(seed, H, W), the recipe the fixture names"""
    from rapiddoc_amd import weights as W
    z = np.load(golden_dir / "table_path_resample.npz")
    out = []
    for name in [str(n) for n in z["names"]]:
        oh, ow = (int(v) for v in z[name + "_out"])
        if name + "_in" in z.files:
            src = z[name + "_in"]
        else:
            seed, h, w = (int(v) for v in z[name + "_recipe"])
            src = W.synth_table_crop(seed, h, w)
        out.append((name, src, oh, ow, z[name + "_exp"]))
    return out
