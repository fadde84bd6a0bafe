"""Helpers the per-kind tests share (tests/test_gpu_det_server.py, test_gpu_det_mobile.py, test_gpu_det_v3_mobile.py, test_gpu_v5_server.py,
test_gpu_v5_mobile.py, test_gpu_rec_mv1e.py, test_gpu_cls_mobile.py and their tests/test_*_host.py counterparts).  A plain module, imported
the way tests/dec_reference.py is; what differs between two kinds in what it computes stays in that kind's file."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from rapiddoc_amd import ocr_host
from rapiddoc_amd import weights as W

GUARD = 4096                 # floats behind an output buffer that must come back untouched
SENTINEL = 12345.0
RELU, HSWISH = 1, 2          # the activation codes of the MobileNetV3 developer entries


# ---------------------------------------------------------------------------------------------------------------- weights, engines, fixtures
def synth_state(golden_dir, kind, /, **kw):
    """The synthetic state dict (seed 0) of tests/golden/manifest_<kind>.json; kw: synth_state_dict's, e.g. kind= for the opt-in gains"""
    return W.synth_state_dict(W.load_manifest(golden_dir / f"manifest_{kind}.json"), 0, **kw)


def engine_cache(kind, guard="off", state=None):
    """-> engine(golden_dir, precision="auto", *key): one RdEngine of `kind` per (precision, *key), kept in a dictionary that belongs to
    this call - one per test module.  RD_PRECISION is read when the handle is created, so it is set around that and put back.
    `state(golden_dir, *key)` makes the weights (default: synth_state of the kind)."""
    engines = {}

    def engine(golden_dir, precision="auto", *key):
        from rapiddoc_amd.engine import RdEngine
        if (precision, *key) not in engines:
            old = os.environ.get("RD_PRECISION")
            os.environ["RD_PRECISION"] = precision
            try:
                st = state(golden_dir, *key) if state else synth_state(golden_dir, kind)
                engines[(precision, *key)] = RdEngine(kind, guard=guard).load_weights(st)
            finally:
                if old is None:
                    del os.environ["RD_PRECISION"]
                else:
                    os.environ["RD_PRECISION"] = old
        return engines[(precision, *key)]
    return engine


def golden_x(g):
    """The input of a fixture: stored, or its recipe (uniform in [-1, 1] from the stored seed)"""
    if "x" in g.files:
        return g["x"]
    assert str(g["x_kind"]) == "pm1"
    return np.random.default_rng(int(g["x_seed"])).uniform(-1.0, 1.0, tuple(int(v) for v in g["x_shape"])).astype(np.float32)


def bound(ref, tol):
    return tol * max(1.0, float(np.abs(ref).max()))


def check_det_fixture(eng, golden_dir, tag, label, prefix, neck_channels, name, tol):
    """A detector against tests/golden/<prefix>_seed0_<tag>.npz: `maps` within tol, the neck output `fuse` [B,neck_channels,H/4,W/4] within
    bound(ref, tol); `name` and `label` go into the printed line"""
    g = np.load(golden_dir / f"{prefix}_seed0_{tag}.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    maps, fuse = eng.det_forward(x, want_neck=True)
    plain = eng.det_forward(x)
    assert torch.equal(plain, maps)                                   # the debug output does not move the result
    maps, fuse = maps.cpu().numpy(), fuse.cpu().numpy()
    B, _, H, W_ = x.shape
    assert maps.shape == (B, 1, H, W_) and fuse.shape == (B, neck_channels, H // 4, W_ // 4)
    ps, cs, fps = int(g["maps_ps"]), int(g["fuse_cs"]), int(g["fuse_ps"])
    e_maps = float(np.abs(maps[:, :, ::ps, ::ps] - g["maps"]).max())
    ref_fuse = g["fuse"]
    e_fuse = float(np.abs(fuse[:, ::cs, ::fps, ::fps] - ref_fuse).max())
    b_fuse = bound(ref_fuse, tol)
    print(f"\n[{name} {tag} {label}] max-abs errors: maps {e_maps:.3e} (bound {tol:.0e}), fuse {e_fuse:.3e} (bound {b_fuse:.3e}, "
          f"max |ref| {float(np.abs(ref_fuse).max()):.1f})")
    assert not eng.range_overflow()
    assert e_maps <= tol
    assert e_fuse <= b_fuse


def write_weights(tmp_path, stem, state):
    """`state` as <tmp_path>/<stem>.safetensors with the names a session file carries (`model.` in front)"""
    p = tmp_path / f"{stem}.safetensors"
    p.write_bytes(W.to_safetensors_bytes({"model." + k: v for k, v in state.items()}))
    return p


# ---------------------------------------------------------------------------------------------------------------- float64 restatements
def hswish64(t):
    return t * torch.clamp(t + 3.0, 0.0, 6.0) / 6.0


def act64(t, a):
    return F.relu(t) if a == RELU else hswish64(t) if a == HSWISH else t


# ---------------------------------------------------------------------------------------------------------------- operands of a kernel alone
def strided(t, ld):
    """t [N,H,W,C] -> the same values as a view of a [N,H,W,ld] buffer whose padding channels hold the sentinel"""
    buf = torch.full((*t.shape[:3], ld), SENTINEL, device=t.device)
    buf[..., :t.shape[3]] = t
    return buf


def out_buffer(N, OH, OW, Cn, yld):
    """An output [N,OH,OW,yld] prefilled with NaN, the sentinel in its padding channels and in a guard band behind it"""
    n_out = N * OH * OW * yld
    buf = torch.full((n_out + GUARD,), float("nan"), device="cuda")
    buf[n_out:] = SENTINEL
    view = buf[:n_out].view(N, OH, OW, yld)
    view[..., Cn:] = SENTINEL
    return buf, view, n_out


def check_out(buf, view, n_out, Cn):
    torch.cuda.synchronize()
    assert bool((buf[n_out:] == SENTINEL).all()), "the guard band behind the output was written"
    assert bool((view[..., Cn:] == SENTINEL).all()), "the padding channels of the output were written"
    y = view[..., :Cn]
    assert not bool(torch.isnan(y).any()), "an output element was not written"
    return y


def line_launch(lines, W_launch):
    """Lines [1,3,48,w] -> one zero-padded [n,3,48,W_launch] tensor, the line table on the device, the token offsets."""
    from rapiddoc_amd.engine import rec_line_table
    x = torch.zeros((len(lines), 3, 48, W_launch), device="cuda")
    for i, ln in enumerate(lines):
        x[i, :, :, : ln.shape[3]] = ln[0]
    T = [ocr_host.rec_seq_len(ln.shape[3]) for ln in lines]
    first = np.concatenate([[0], np.cumsum(T)[:-1]])
    tab = torch.from_numpy(rec_line_table([ln.shape[3] for ln in lines], first)).cuda()
    return x, tab, T, first


def rand_lines(widths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand((1, 3, 48, w), generator=g) * 2 - 1).cuda() for w in widths]
