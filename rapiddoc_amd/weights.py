"""Weight containers for the MI355X engine.

The reference ships PP-OCRv6 weights as ``.safetensors`` files and loads them with
``safetensors.torch.load_file`` + ``load_state_dict`` (reference
``rapid_doc/model/ocr/torch.py:93-110``: a leading ``model.`` prefix is stripped).  The engine's C-ABI
``rd_load_weights`` takes exactly that byte image, so real weights drop in unchanged.

No real weights exist in the build container (``.MISSING_LARGE_BLOBS``), so tests and benchmarks use
*synthetic* weights generated deterministically from a manifest of (name, shape) pairs that was captured
from the reference's own ``state_dict()`` (``tests/golden/manifest_*.json``).  The generator is
numpy-only so the same bytes are produced in the build container (where golden outputs are minted with
the reference definitions) and on the GPU box.
"""
from __future__ import annotations

import json
import struct
import zlib
from pathlib import Path
from typing import Dict, Iterable, List, Tuple

import numpy as np

Manifest = List[Tuple[str, Tuple[int, ...], str]]

_LCNETV3_BRANCH_GAIN = (("blocks2", 0.65), ("blocks3", 0.65), ("blocks4", 0.6), ("blocks5", 0.6), ("blocks6", 0.7))
# opt-in extra factors per model kind (synth_state_dict(..., kind=...)), on top of the rules of synth_tensor; (name test, factor)
_KIND_GAINS = {
    # PP-OCRv5 mobile detector: the PPLCNetV3 damping above was set for the recogniser's 48-row maps; at page size the reference
    # saturates (features 1700, fuse 7900, `maps` nearly binary).  These keep the stage features O(2-25) and spread the shrink logit
    "ppocrv5_det_mobile": (
        (lambda n: n.startswith("backbone.blocks5.") and n.endswith(".conv.weight"), 0.85),
        (lambda n: n.startswith("backbone.blocks6.") and n.endswith(".conv.weight"), 0.8),
        (lambda n: n.startswith("backbone.layer_list.") and n.endswith(".weight"), 0.5),
        (lambda n: n == "head.binarize.conv3.weight", 3.0),
    ),
}
# Multilingual PP-OCRv3 / v4 mobile recogniser (MobileNetV1Enhance): a plain chain of Conv + BN + hardswish.  Under the plain rule it
# collapses onto its biases (std along the line 0.1-0.3 % of absmax) and a uniform gain explodes it; these per-layer factors on the
# convolutions (depthwise, pointwise per block) were calibrated to a block-output absmax of about 8 on a 2 x 320 input
_MV1E_BLOCK_GAINS = ((0.7, 1.3), (0.6, 1.3), (1.6, 1.2), (1.6, 1.4), (1.1, 1.4), (0.7, 2.2), (1.0, 2.2), (0.9, 1.2), (1.1, 2.0), (1.1, 1.6),
                     (0.5, 2.5), (0.8, 2.8), (1.2, 4.0))


def _mv1e_gains():
    rules = [(lambda n: n == "backbone.conv1._conv.weight", 2.2), (lambda n: n == "head.fc.weight", 30.0)]
    for i, (dw, pw) in enumerate(_MV1E_BLOCK_GAINS):
        rules.append((lambda n, i=i: n == "backbone.block_list.%d._depthwise_conv._conv.weight" % i, dw))
        rules.append((lambda n, i=i: n == "backbone.block_list.%d._pointwise_conv._conv.weight" % i, pw))
    return tuple(rules)


_KIND_GAINS["ppocr_rec_mv1e"] = _mv1e_gains()
# PP-OCRv3 multilingual detector (MobileNetV3 large scale 0.5 without SE): the residual blocks at 1/16 add up (stage features 50-100, `fuse`
# 300 under the plain rule); damping their linear layers keeps the stage features O(5-30), and the last transposed convolution is spread so
# that the shrink logit fills (0, 1) at page size
_KIND_GAINS["ppocrv3_det_mobile"] = (
    (lambda n: n.startswith("backbone.stages.2.") and n.endswith(".linear_conv.conv.weight"), 0.7),
    (lambda n: n.startswith("backbone.stages.3.") and n.endswith(".linear_conv.conv.weight"), 0.7),
    (lambda n: n == "head.binarize.conv3.weight", 3.0),
)
# Text-line direction classifier (MobileNetV3 small scale 0.35 + ClsHead): under the plain rule the two logits stay together and the
# softmax answers 0.46-0.47 for every line.  The gain on the head spreads the logit difference across lines; the additive term on the
# head's bias (_KIND_OFFSETS: (name test, per-element values)) centres it, so that both labels and both sides of the 0.9 threshold occur
_KIND_GAINS["ppocr_cls_mobile"] = (
    (lambda n: n == "head.fc.weight", 300.0),
)
# PP-OCRv4 server detector / recogniser (PPHGNet_small): under the plain rule every ESE gate of the backbone sits near 0.5 (pre-sigmoid
# logits of std 0.2 - 0.9) and a wrong gate would hardly show in the outputs.  A gain per HG_Block on `att.conv.weight` brings the logits
# of every block to a std of 1.2 - 1.9 on the fixtures' inputs (tests/golden/summary_v4_server.json records them); the biases keep the plain draw
_KIND_GAINS["ppocrv4_server"] = tuple(
    (lambda n, blk=blk: n == "backbone.%s.att.conv.weight" % blk, g)
    for blk, g in (("stages.0.blocks.0", 2.0), ("stages.1.blocks.0", 3.0), ("stages.2.blocks.0", 4.0), ("stages.2.blocks.1", 6.0),
                   ("stages.3.blocks.0", 5.0)))
_KIND_OFFSETS = {
    "ppocr_cls_mobile": (
        (lambda n: n == "head.fc.bias", (-11.6, 11.6)),
    ),
}
_NORM_TOKENS = (".normalization.", ".norm.", ".bn.", "layer_norm", ".norm1.", ".norm2.")


def load_manifest(path) -> Manifest:
    raw = json.loads(Path(path).read_text())
    return [(n, tuple(s), d) for n, s, d in raw]


def _is_norm(name: str) -> bool:
    if any(tok in name for tok in _NORM_TOKENS):
        return True
    # `head.encoder.norm.weight` style (LightSVTR final LayerNorm)
    stem = name.rsplit(".", 1)[0]
    return stem.endswith(".norm") or stem.endswith("norm")


def synth_tensor(name: str, shape: Tuple[int, ...], dtype: str, seed: int) -> np.ndarray:
    """One synthetic tensor, a pure function of (name, shape, seed)."""
    rng = np.random.default_rng([seed, zlib.crc32(name.encode())])
    leaf = name.rsplit(".", 1)[-1]
    if leaf == "num_batches_tracked":
        return np.zeros(shape, dtype=np.int64)
    if leaf == "running_mean":
        return rng.normal(0.0, 0.1, shape).astype(np.float32)
    if leaf == "running_var":
        return rng.uniform(0.5, 1.5, shape).astype(np.float32)
    if len(shape) <= 1 and leaf == "weight" and _is_norm(name):
        return rng.uniform(0.8, 1.2, shape).astype(np.float32)
    if leaf == "bias":
        return rng.normal(0.0, 0.05, shape).astype(np.float32)
    if leaf in ("scale",):
        return rng.uniform(0.8, 1.2, shape).astype(np.float32)
    if leaf == "weight" and len(shape) >= 2:
        fan_in = int(np.prod(shape[1:]))
        # ConvTranspose2d stores [Cin, Cout, kh, kw]; its fan-in is Cin.
        if "conv_up" in name or "conv_final" in name:
            fan_in = shape[0]
        # gain 1.6 (most convs here are linear or followed by a residual add); the second point-wise conv
        # of a residual mixer is damped so that 20+ stacked blocks keep activations O(1..10).
        std = (1.6 / max(fan_in, 1)) ** 0.5
        if ".channel_conv2." in name or ".aggregation_excitation_conv." in name or ".mlp.fc2." in name:
            std *= 0.5
        if name == "head.head.weight":  # CTC classifier: spread the logits so argmax varies over time
            std *= 6.0
        if name == "head.ctc_head.fc.weight":  # PP-OCRv5 server CTC classifier: its neck output is nearly flat, 30x opens the top-2 gaps
            std *= 30.0
        # PP-OCRv5 server detector: with the plain rule both logits of PFHeadLocal stay near 0 and `maps` is flat (0.44-0.67); these two
        # gains spread the shrink and the cbn logits so that the map fills (0, 1)
        if name == "head.binarize.conv3.weight":
            std *= 10.0
        if name == "head.cbn_layer.last_1.weight":
            std *= 100.0
        # PP-OCRv5 mobile recogniser (PPLCNetV3): every layer is a sum of 4-6 branches under a hardswish, which is quadratic below 3, so
        # the plain rule explodes (1e7 by blocks6) and one global damping collapses the net onto its biases; a factor per block group
        # on the branch convolutions keeps every group's activations O(10)
        if name.endswith(".conv.weight") and (".conv_kxk." in name or ".conv_1x1." in name):
            for group, f in _LCNETV3_BRANCH_GAIN:
                if name.startswith("backbone." + group + "."):
                    std *= f
        return rng.normal(0.0, std, shape).astype(np.float32)
    return rng.normal(0.0, 0.05, shape).astype(np.float32)


def synth_state_dict(manifest: Manifest, seed: int = 0, kind: str = None) -> Dict[str, np.ndarray]:
    """`kind`: opt-in gains of one model kind (_KIND_GAINS); without it every tensor is synth_tensor's, whatever the manifest."""
    state = {name: synth_tensor(name, shape, dtype, seed) for name, shape, dtype in manifest}
    if kind is not None:
        if kind not in _KIND_GAINS:
            raise ValueError(f"no synthetic-weight gains are defined for kind {kind!r}")
        for name, arr in state.items():
            if arr.dtype != np.float32 or arr.ndim < 2:
                continue
            for applies, f in _KIND_GAINS[kind]:
                if applies(name):
                    state[name] = (arr * np.float32(f)).astype(np.float32)
        for name, arr in state.items():
            for applies, add in _KIND_OFFSETS.get(kind, ()):
                if applies(name):
                    state[name] = (arr + np.asarray(add, dtype=np.float32).reshape(arr.shape)).astype(np.float32)
    return state


def synth_cls_lines(seed: int, b: int, h: int = 48, w: int = 192) -> Tuple[np.ndarray, np.ndarray]:
    """Synthetic classifier input [b,3,h,w] in [-1, 1] and its content widths: line i carries noise of its own brightness and contrast over
    its first widths[i] columns (12 ... w, ragged) and the zero right-padding of the classifier's pre-process behind them.  A pure
    function of the arguments (numpy only), so that a fixture stores the recipe instead of the tensor."""
    rng = np.random.default_rng([seed, b, h, w])
    lo = min(12, w)
    widths = np.linspace(lo, w, b).round().astype(np.int64) if b > 1 else np.array([w], dtype=np.int64)
    widths = widths[rng.permutation(b)]
    x = np.zeros((b, 3, h, w), dtype=np.float32)
    for i in range(b):
        mean, contrast = rng.uniform(-0.6, 0.6), rng.uniform(0.1, 0.8)
        tint = rng.uniform(-0.15, 0.15, (3, 1, 1))
        u = rng.uniform(-1.0, 1.0, (3, h, int(widths[i])))
        x[i, :, :, : widths[i]] = np.clip(mean + tint + contrast * u, -1.0, 1.0).astype(np.float32)
    return x, widths


def synth_normal_image(seed: int, b: int, h: int, w: int) -> np.ndarray:
    """Synthetic normalised image batch [b,3,h,w], standard normal (the UniTable pre-process divides by the ImageNet std, so a real input is
    of that scale).  A pure function of the arguments (numpy only), so that a fixture stores the recipe instead of the tensor."""
    return np.random.default_rng([seed, b, h, w]).standard_normal((b, 3, h, w)).astype(np.float32)


def _mix64(v: np.ndarray) -> np.ndarray:
    """splitmix64's finaliser on uint64 arrays (wrapping integer arithmetic: the same bits on every machine and numpy version)"""
    v = (v ^ (v >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    v = (v ^ (v >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return v ^ (v >> np.uint64(31))


def synth_table_crop(seed: int, h: int, w: int) -> np.ndarray:
    """Synthetic table crop [h,w,3] uint8 (BGR or RGB, as the caller reads it): a near-white page, ruled lines every 37 rows / 113 columns,
    and in every cell text-like bars (9 rows high, ragged runs, per-pixel texture of 48 grey levels) with a faint tint per channel.  A pure
    function of the arguments built on an integer hash of its own (no numpy Generator stream), so that a fixture stores the recipe."""
    with np.errstate(over="ignore"):
        yy, xx = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
        s = np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        pix = _mix64(s + yy * np.uint64(0x100000001B3) + xx)                       # per pixel
        run = _mix64(s + (yy // np.uint64(14)) * np.uint64(7919) + (xx // np.uint64(23)) + np.uint64(1 << 40))       # per 14 x 23 block
    img = np.full((h, w), 246, dtype=np.int64) + (pix & np.uint64(7)).astype(np.int64)
    bar = ((yy % np.uint64(14)) >= np.uint64(3)) & ((yy % np.uint64(14)) < np.uint64(12)) & ((run & np.uint64(3)) != np.uint64(0))
    ink = 20 + ((pix >> np.uint64(8)) % np.uint64(48)).astype(np.int64) + ((run >> np.uint64(4)) % np.uint64(90)).astype(np.int64)
    img = np.where(bar, ink, img)
    rule = ((yy % np.uint64(37)) == np.uint64(0)) | ((xx % np.uint64(113)) < np.uint64(2))
    img = np.where(rule, 12, img)
    out = np.stack([np.clip(img + t, 0, 255) for t in (0, -3, 4)], axis=-1)
    return np.ascontiguousarray(out.astype(np.uint8))


def synth_memory(seed: int, b: int, s: int, d: int = 768) -> np.ndarray:
    """Synthetic encoder output [b,s,d], standard normal (a LayerNorm output is of that scale).  A pure function of the arguments."""
    return np.random.default_rng([seed, b, s, d]).standard_normal((b, s, d)).astype(np.float32)


def checksum(state: Dict[str, np.ndarray]) -> float:
    """Order-independent float64 checksum used to pin the generator across machines."""
    tot = 0.0
    for name in sorted(state):
        tot += float(np.asarray(state[name], dtype=np.float64).sum())
    return tot


_ST_DTYPES = {"float32": "F32", "int64": "I64", "float16": "F16", "int32": "I32", "uint8": "U8"}
_ST_NP = {v: k for k, v in _ST_DTYPES.items()}


def to_safetensors_bytes(state: Dict[str, np.ndarray], skip_int: bool = False) -> bytes:
    """Serialise to the safetensors byte image (8-byte LE header length, JSON header, raw data)."""
    header = {}
    chunks = []
    off = 0
    for name, arr in state.items():
        arr = np.asarray(arr, order="C")          # (np.ascontiguousarray would turn a 0-d tensor - num_batches_tracked - into shape [1])
        if skip_int and arr.dtype.kind in "iu":
            continue
        raw = arr.tobytes()
        header[name] = {
            "dtype": _ST_DTYPES[str(arr.dtype)],
            "shape": list(arr.shape),
            "data_offsets": [off, off + len(raw)],
        }
        chunks.append(raw)
        off += len(raw)
    hjson = json.dumps(header, separators=(",", ":")).encode()
    pad = (8 - len(hjson) % 8) % 8
    hjson += b" " * pad
    return struct.pack("<Q", len(hjson)) + hjson + b"".join(chunks)


def from_safetensors_bytes(blob: bytes) -> Dict[str, np.ndarray]:
    (hlen,) = struct.unpack("<Q", blob[:8])
    header = json.loads(blob[8 : 8 + hlen])
    base = 8 + hlen
    out = {}
    for name, meta in header.items():
        if name == "__metadata__":
            continue
        b, e = meta["data_offsets"]
        arr = np.frombuffer(blob[base + b : base + e], dtype=_ST_NP[meta["dtype"]]).reshape(meta["shape"])
        out[name] = arr
    return out


def strip_model_prefix(state: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """Reference ``torch.py:105-110``: drop a leading ``model.`` from every key."""
    if any(k.startswith("model.") for k in state):
        return {k[len("model."):] if k.startswith("model.") else k: v for k, v in state.items()}
    return state
