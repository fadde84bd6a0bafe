"""GPU: the PP-OCRv3 multilingual detector (`model_kind "ppocrv3_det_mobile"`: MobileNetV3 large scale 0.5 without SE + RSEFPN + DBHead)
against the fixtures minted from the reference's own modules (tests/golden/make_golden_det_v3_mobile.py), on both block routes
(RD_MBV3_FUSED), its launch invariance, the two kernels of csrc/kernels_mbv3.hip alone against float64, the range guard, and the session /
page pipeline on top of it.  (Folds, kind selection and the float64 restatement of the folded graph: tests/test_det_v3_mobile_host.py.)

Bounds: `maps` 1e-3 max-abs; the neck output and the stage features 1e-3 * max(1, max |ref|) (the project's bounds, tests/test_gpu_det_mobile.py);
a kernel alone against float64 2e-5 * max(1, max |ref|), the project's depthwise bound.  For the fused block that bound is doubled to
twice the UNFUSED route's own measured error on the same operands (fp32 matrix kernels + the depthwise kernel) only where that error is
itself above half of it; the fused error is never compared with itself.  Figures are printed before they are asserted (run with -s)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kind_helpers import HSWISH, RELU, act64, check_out, engine_cache, golden_x, out_buffer, strided, synth_state, write_weights
from rapiddoc_amd import _lib
from rapiddoc_amd import weights as W

pytestmark = pytest.mark.gpu
TOL = 1e-3
KIND = "ppocrv3_det_mobile"
TAGS = ["b2_h64_w96", "b1_h160_w224", "b3_h96_w352", "b1_h960_w704"]
STAGE_CH = (16, 24, 56, 480)


def _state(golden_dir, kind=KIND, gains=None):
    return synth_state(golden_dir, kind, kind=gains if gains else (KIND if kind == KIND else None))


_engine = engine_cache(KIND, state=_state)


def _check_against_fixture(eng, golden_dir, tag, label):
    g = np.load(golden_dir / f"det3m_seed0_{tag}.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    B, _, H, W_ = x.shape
    # every output is handed over prefilled with NaN and must come back fully written
    out = torch.full((B, 1, H, W_), float("nan"), device="cuda")
    maps, fuse, stages = eng.det_forward(x, out=out, want_stages=True)
    assert maps is out
    maps2, fuse2 = eng.det_forward(x, want_neck=True)
    plain = eng.det_forward(x)
    assert torch.equal(plain, maps) and torch.equal(maps2, maps) and torch.equal(fuse2, fuse)      # the debug outputs do not move the result
    assert fuse.shape == (B, 96, H // 4, W_ // 4)
    assert [tuple(s.shape) for s in stages] == [(B, c, H // r, W_ // r) for c, r in zip(STAGE_CH, (4, 8, 16, 32))]
    got = {"maps": maps, "fuse": fuse, **{f"stage{i}": s for i, s in enumerate(stages)}}
    assert not eng.range_overflow()
    msgs, bad = [], []
    for name, y in got.items():
        assert not bool(torch.isnan(y).any()), f"{name}: an output element was not written"
        ref = g[name]
        cs = int(g[name + "_cs"]) if name != "maps" else 1
        ps = int(g[name + "_ps"])
        e = float(np.abs(y.cpu().numpy()[:, ::cs, ::ps, ::ps] - ref).max())
        bound = TOL if name == "maps" else TOL * max(1.0, float(np.abs(ref).max()))
        msgs.append(f"{name} {e:.3e} (bound {bound:.3e})")
        if not e <= bound:
            bad.append(name)
    print(f"\n[det v3 mobile {tag} {label}] max-abs errors: " + ", ".join(msgs))
    assert not bad, bad


@pytest.mark.parametrize("precision", ["auto", "fp32"])
@pytest.mark.parametrize("tag", TAGS)
def test_whole_network_matches_the_reference_fixtures(golden_dir, tag, precision):
    _check_against_fixture(_engine(golden_dir, precision), golden_dir, tag, precision)


def test_whole_network_in_h3_mode(golden_dir):
    _check_against_fixture(_engine(golden_dir, "h3"), golden_dir, "b2_h64_w96", "h3")


_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
from pathlib import Path
import test_gpu_det_v3_mobile as T
from rapiddoc_amd.engine import RdEngine
gd = Path({golden!r})
eng = RdEngine(T.KIND, guard="off").load_weights(T._state(gd))
eng.set_profiling(True)
eng.profile_log.clear()
T._check_against_fixture(eng, gd, {tag!r}, "RD_MBV3_FUSED=" + {route!r})
kinds = [r["kind"] for r in eng.profile_log]
print("BLOCKS", sum(k == "mbv3_block" for k in kinds), "DW", sum(k.startswith("mbv3_dw") for k in kinds))
"""


@pytest.mark.parametrize("route", ["0", "1"])
def test_whole_network_on_either_hardswish_depthwise_route(golden_dir, monkeypatch, route):
    """RD_MBV3_DW2D=0|1 (read per plan) puts the hardswish depthwise layers with C % 16 == 0 (96, 96, 240, 336, 336, 480, 480) on
    mbv3_dw_kernel / on the LDS-staged lcv3_dw2d_kernel; both meet the fixture; C = 104 and 120 are always direct."""
    from rapiddoc_amd.engine import RdEngine
    monkeypatch.setenv("RD_MBV3_DW2D", route)
    monkeypatch.setenv("RD_PRECISION", "auto")
    eng = RdEngine(KIND, guard="off").load_weights(_state(golden_dir))
    _check_against_fixture(eng, golden_dir, "b1_h160_w224", "RD_MBV3_DW2D=" + route)
    eng.set_profiling(True)
    eng.profile_log.clear()
    eng.det_forward(torch.zeros((1, 3, 160, 224), device="cuda"))
    staged = [r["shape"].rsplit("_C", 1)[1] for r in eng.profile_log if r["kind"].startswith("mbv3_dw") and "/lds2d" in r["cfg"]]
    assert staged == (["96", "96", "240", "336", "336", "480", "480"] if route == "1" else [])


@pytest.mark.parametrize("route,tag,poison", [("0", "b1_h160_w224", "0"), ("1", "b1_h160_w224", "1"), ("1", "b3_h96_w352", "0")])
def test_whole_network_on_either_block_route_in_a_fresh_process(golden_dir, route, tag, poison):
    """RD_MBV3_FUSED=0|1 puts every block the fused kernel can take on one route: six fused blocks (those of the 1/2, 1/4 and 1/8 levels
    with mid <= 64) and nine unfused, or fifteen unfused.  Both meet the fixture; one case runs with the arena poisoned."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _CHILD.format(root=root, tests=os.path.join(root, "tests"), golden=str(golden_dir), tag=tag, route=route)
    env = dict(os.environ, RD_MBV3_FUSED=route, RD_PRECISION="auto", RD_POISON_ARENA=poison)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    counts = [ln for ln in r.stdout.splitlines() if ln.startswith("BLOCKS")][-1].split()
    # (every forward of the check is logged: three forwards)
    assert (int(counts[1]) // 3, int(counts[3]) // 3) == ((6, 9) if route == "1" else (0, 15))


@pytest.mark.parametrize("precision", ["auto", "fp32"])
def test_an_image_does_not_depend_on_the_launch_it_rides_in(golden_dir, precision):
    eng = _engine(golden_dir, precision)
    g = np.load(golden_dir / "det3m_seed0_b3_h96_w352.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    m3, f3 = eng.det_forward(x, want_neck=True)
    m3, f3 = m3.clone(), f3.clone()
    m1, f1 = eng.det_forward(x[1:2].contiguous(), want_neck=True)
    assert torch.equal(m1[0], m3[1]) and torch.equal(f1[0], f3[1])


@pytest.mark.parametrize("fused", [None, "1"])
def test_routes_follow_the_layer_not_the_batch_or_the_page(golden_dir, monkeypatch, fused):
    from rapiddoc_amd.engine import RdEngine
    if fused is None:
        monkeypatch.delenv("RD_MBV3_FUSED", raising=False)
    else:
        monkeypatch.setenv("RD_MBV3_FUSED", fused)
    eng = RdEngine(KIND, guard="off").load_weights(_state(golden_dir))     # (plans are built under this setting)

    def ops(shape):
        eng.set_profiling(True)
        eng.profile_log.clear()
        eng.det_forward(torch.zeros(shape, device="cuda"))
        got = [(r["name"], r["kind"], r["cfg"]) for r in eng.profile_log]
        eng.set_profiling(False)
        return got

    a = ops((1, 3, 64, 96))
    assert a == ops((3, 3, 64, 96)) == ops((1, 3, 160, 224)) == ops((2, 3, 96, 352))
    blocks = [n for n, k, c in a if k == "mbv3_block"]
    # (the defaults of the A/B table, docs/notebook/v3_mobile_det.md, are those six blocks too)
    assert blocks == [f"backbone.stages.{s}.{i}" for s, i in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2))]
    assert [c for n, k, c in a if k == "mbv3_block"][0] == "k3s1/relu/inact/res"      # block 0 activates conv1's output on load
    assert not any(k == "lcv3_act" and i < 3 for i, (n, k, c) in enumerate(a))        # ... so the separate pass is gone
    assert len(blocks) + sum(k.startswith("mbv3_dw") for n, k, c in a) == 15


# ---------------------------------------------------------------------------------------------------------------- the kernels alone
def _debug_dw(x, w, b, K, S, pre_act, post_act, xld=None, yld=None, max_blocks=0):
    fn = _lib.load().rd_debug_mbv3_dw
    N, H, W_, Cn = x.shape
    xld, yld = xld or Cn, yld or Cn
    OH, OW = (H - 1) // S + 1, (W_ - 1) // S + 1
    xb = strided(x, xld)
    buf, view, n_out = out_buffer(N, OH, OW, Cn, yld)
    wk = w.reshape(Cn, K * K).t().contiguous()                           # [K*K][C]
    ms = fn(N, H, W_, Cn, K, S, pre_act, post_act, xld, yld, 0, max_blocks, xb.data_ptr(), wk.data_ptr(), b.data_ptr(), buf.data_ptr())
    assert ms >= 0, "the kernel does not serve this geometry"
    return check_out(buf, view, n_out, Cn)


def _dw_ref(x, w, b, K, S, pre_act, post_act):
    xd = act64(x.permute(0, 3, 1, 2).double(), pre_act)
    y = F.conv2d(F.pad(xd, (K // 2,) * 4), w.double(), b.double(), stride=S, groups=x.shape[3])
    return act64(y, post_act).permute(0, 2, 3, 1)


@pytest.mark.parametrize("K,S", [(3, 1), (3, 2), (5, 1), (5, 2)])
@pytest.mark.parametrize("H,W_,Cn", [(2, 3, 336), (9, 35, 8), (17, 33, 40), (12, 70, 104)])
def test_depthwise_kernel_matches_fp64(H, W_, Cn, K, S):
    """N = 2, inputs spanning +-4, every pairing of the on-load activation (none / ReLU / hardswish) with the epilogue's, contiguous and
    with row strides above C.  Bound 2e-5 * max(1, max |ref|)."""
    N = 2
    g = torch.Generator(device="cuda").manual_seed(H * 1000 + Cn + 10 * K + S)
    x = torch.rand((N, H, W_, Cn), device="cuda", generator=g) * 8 - 4
    w = (torch.rand((Cn, 1, K, K), device="cuda", generator=g) - 0.5) * (1.2 / K)
    b = torch.rand((Cn,), device="cuda", generator=g) - 0.5
    for pre_act in (0, RELU, HSWISH):
        for post_act in (0, RELU, HSWISH):
            ref = _dw_ref(x, w, b, K, S, pre_act, post_act)
            bound = 2e-5 * max(1.0, ref.abs().max().item())
            for xld, yld in ((Cn, Cn), (Cn + 8, Cn + 4)):
                y = _debug_dw(x, w, b, K, S, pre_act, post_act, xld, yld)
                e = (y.double() - ref).abs().max().item()
                print(f"\n[mbv3 dw {N}x{H}x{W_}x{Cn} k{K} s{S} pre {pre_act} post {post_act} ld {xld}/{yld}] max |y - fp64| {e:.3e} (bound {bound:.3e})")
                assert y.shape == ref.shape and e < bound


@pytest.mark.parametrize("K,S", [(3, 1), (5, 2)])
def test_depthwise_kernel_grid_stride_loop(K, S):
    """The launch caps its grid at 65536 workgroups and walks the rest in a grid-stride loop; no map of a test reaches that cap (the 32-page
    bench shape does not either), so the cap is lowered to 3 and to 1 workgroups here: 2 x 12 x 70 x 104 is 11 / 6 workgroups' worth of work.
    Bit for bit the uncapped launch's result."""
    g = torch.Generator(device="cuda").manual_seed(7 + K)
    x = torch.rand((2, 12, 70, 104), device="cuda", generator=g) * 8 - 4
    w = (torch.rand((104, 1, K, K), device="cuda", generator=g) - 0.5) * (1.2 / K)
    b = torch.rand((104,), device="cuda", generator=g) - 0.5
    full = _debug_dw(x, w, b, K, S, HSWISH, HSWISH).clone()
    assert (full.double() - _dw_ref(x, w, b, K, S, HSWISH, HSWISH)).abs().max().item() < 2e-5 * max(1.0, full.abs().max().item())
    for cap in (3, 1):
        assert torch.equal(_debug_dw(x, w, b, K, S, HSWISH, HSWISH, max_blocks=cap), full)


def _debug_conv(x, w, b, act, res=None):
    """The unfused route's 1x1 layers on the fp32 matrix kernel (rd_debug_conv without split weights): x [N,H,W,Cin] contiguous"""
    fn = _lib.load().rd_debug_conv
    N, H, W_, Cin = x.shape
    Cout = w.shape[0]
    y = torch.full((N, H, W_, Cout), float("nan"), device="cuda")
    used = C.c_int(0)
    ms = fn(N, H, W_, Cin, Cout, 1, 1, 1, 0, 0, 0, 0, act, 0, x.data_ptr(), w.data_ptr(), None, None, b.data_ptr(), res.data_ptr() if res is not None else None,
            y.data_ptr(), C.addressof(used))
    torch.cuda.synchronize()
    assert ms >= 0
    return y


def _debug_block(x, p, K, S, act, in_hswish, shortcut, xld, yld):
    fn = _lib.load().rd_debug_mbv3_block
    N, H, W_, cin = x.shape
    mid, cout = p["we"].shape[0], p["wl"].shape[0]
    OH, OW = (H - 1) // S + 1, (W_ - 1) // S + 1
    xb = strided(x, xld)
    buf, view, n_out = out_buffer(N, OH, OW, cout, yld)
    ms = fn(N, H, W_, cin, mid, cout, K, S, act, int(in_hswish), int(shortcut), xld, yld, 0, xb.data_ptr(), p["we"].data_ptr(), p["be"].data_ptr(),
            p["wd_k"].data_ptr(), p["bd"].data_ptr(), p["wl"].data_ptr(), p["bl"].data_ptr(), buf.data_ptr())
    assert ms >= 0, "the kernel does not serve this geometry"
    return check_out(buf, view, n_out, cout)


def _block_ref(x, p, K, S, act, in_hswish, shortcut, halo_act_bias=False):
    """float64: expand -> activation -> zero padding -> depthwise -> activation -> linear -> shortcut.  `halo_act_bias`: the wrong
    reading, where the padding of the depthwise layer holds act(expand bias) - to show that the test tells the two apart."""
    xd = x.permute(0, 3, 1, 2).double()
    if in_hswish:
        xd = act64(xd, HSWISH)
    mid = p["we"].shape[0]
    e = act64(F.conv2d(xd, p["we"].double()[:, :, None, None], p["be"].double()), act)
    P = K // 2
    ep = F.pad(e, (P, P, P, P))
    if halo_act_bias:
        fill = act64(p["be"].double(), act)[None, :, None, None].expand_as(ep).clone()
        fill[:, :, P:-P, P:-P] = e
        ep = fill
    d = act64(F.conv2d(ep, p["wd"].double(), p["bd"].double(), stride=S, groups=mid), act)
    y = F.conv2d(d, p["wl"].double()[:, :, None, None], p["bl"].double())
    return (y + xd if shortcut else y).permute(0, 2, 3, 1)


def _unfused_route(x, p, K, S, act, in_hswish, shortcut):
    """The engine's unfused route in fp32 on the same operands: [hardswish pass] -> 1x1 (ReLU in the epilogue, or hardswish on the
    depthwise kernel's load) -> mbv3_dw_kernel -> 1x1 + shortcut."""
    xa = (x * torch.clamp(x + 3.0, 0.0, 6.0) * (1.0 / 6.0)) if in_hswish else x
    xa = xa.contiguous()
    e = _debug_conv(xa, p["we"], p["be"], 1 if act == RELU else 0)
    d = _debug_dw(e, p["wd"], p["bd"], K, S, 0 if act == RELU else HSWISH, act).contiguous()
    return _debug_conv(d, p["wl"], p["bl"], 0, res=xa if shortcut else None)


# k, stride, cin, mid, cout, in_hswish: the five block geometries of the 1/2, 1/4 and 1/8 levels; block 0 with and without the on-load hardswish
BLOCK_GEOMS = [(3, 1, 8, 8, 8, True), (3, 1, 8, 8, 8, False), (3, 2, 8, 32, 16, False), (3, 1, 16, 40, 16, False), (5, 2, 16, 40, 24, False),
               (5, 1, 24, 64, 24, False)]


@pytest.mark.parametrize("H,W_", [(2, 3), (9, 35), (17, 33)])
@pytest.mark.parametrize("K,S,cin,mid,cout,in_hswish", BLOCK_GEOMS)
def test_block_kernel_matches_fp64(K, S, cin, mid, cout, in_hswish, H, W_):
    N = 2
    g = torch.Generator(device="cuda").manual_seed(H * 1000 + mid + 10 * K + S)
    r = lambda *s: torch.rand(s, device="cuda", generator=g)
    x = r(N, H, W_, cin) * 8 - 4
    p = {"we": (r(mid, cin) - 0.5) * (3.0 / cin ** 0.5), "be": r(mid) + 0.5,          # nonzero, positive expand bias: act(bias) != 0
         "wd": (r(mid, 1, K, K) - 0.5) * (1.2 / K), "bd": r(mid) - 0.5,
         "wl": (r(cout, mid) - 0.5) * (3.0 / mid ** 0.5), "bl": r(cout) - 0.5}
    p["wd_k"] = p["wd"].reshape(mid, K * K).t().contiguous()
    shortcut = S == 1 and cin == cout
    for act in (RELU, HSWISH):
        ref = _block_ref(x, p, K, S, act, in_hswish, shortcut)
        bound = 2e-5 * max(1.0, ref.abs().max().item())
        e_unfused = (_unfused_route(x, p, K, S, act, in_hswish, shortcut).double() - ref).abs().max().item()
        if e_unfused > bound / 2:
            bound = 2 * e_unfused
        wrong = _block_ref(x, p, K, S, act, in_hswish, shortcut, halo_act_bias=True)
        assert (wrong[:, 0] - ref[:, 0]).abs().max().item() > 100 * bound          # a halo filled with act(bias) would show at the border
        for xld, yld in ((cin, cout), (cin + 8, cout + 4)):
            y = _debug_block(x, p, K, S, act, in_hswish, shortcut, xld, yld)
            e = (y.double() - ref).abs().max().item()
            print(f"\n[mbv3 block k{K} s{S} {cin}-{mid}-{cout} act {act} inact {int(in_hswish)} {N}x{H}x{W_} ld {xld}/{yld}] max |y - fp64|: fused {e:.3e}, "
                  f"unfused fp32 {e_unfused:.3e} (bound {bound:.3e}, max |ref| {ref.abs().max().item():.2f})")
            assert y.shape == ref.shape and e < bound
            assert (y[:, 0].double() - ref[:, 0]).abs().max().item() < bound and (y[:, :, -1].double() - ref[:, :, -1]).abs().max().item() < bound


def test_block_kernel_refuses_what_it_does_not_serve():
    x = torch.zeros((1, 4, 4, 24), device="cuda")
    z = lambda *s: torch.zeros(s, device="cuda")
    p = {"we": z(120, 24), "be": z(120), "wd": z(120, 1, 3, 3), "wd_k": z(9, 120), "bd": z(120), "wl": z(40, 120), "bl": z(40)}
    with pytest.raises(AssertionError, match="does not serve"):
        _debug_block(x, p, 3, 2, HSWISH, False, False, 24, 40)            # mid 120 at 3x3 / 2: 147 KB of LDS
    p = {"we": z(8, 24), "be": z(8), "wd": z(8, 1, 3, 3), "wd_k": z(9, 8), "bd": z(8), "wl": z(16, 8), "bl": z(16)}
    _debug_block(x, p, 3, 1, RELU, False, False, 24, 16)
    with pytest.raises(AssertionError, match="does not serve"):
        _debug_block(x, p, 3, 1, RELU, False, True, 24, 16)               # a shortcut with cin != cout
    with pytest.raises(AssertionError, match="does not serve"):
        _debug_block(x, p, 3, 1, 0, False, False, 24, 16)                 # no activation named
    with pytest.raises(AssertionError, match="does not serve"):
        _debug_block(x, p, 3, 1, RELU, False, False, 26, 16)              # pixels not 16-byte aligned


# ---------------------------------------------------------------------------------------------------------------- guard, session, pipeline
def test_range_guard_falls_back_to_the_fp32_mode_bit_for_bit(golden_dir, monkeypatch):
    """ins_conv.1's weight times 1e6 puts the level-1 neck feature beyond the fp16 range; the neck's 3x3 convolutions that read it are
    split layers in `auto`."""
    from rapiddoc_amd.engine import RdEngine
    monkeypatch.setenv("RD_PRECISION", "auto")
    big = dict(_state(golden_dir))
    big["neck.ins_conv.1.in_conv.weight"] = big["neck.ins_conv.1.in_conv.weight"] * np.float32(1e6)
    g = np.load(golden_dir / "det3m_seed0_b2_h64_w96.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    ref = RdEngine(KIND, guard="off").load_weights(big).set_precision("fp32").det_forward(x)
    assert bool(torch.isfinite(ref).all())
    raw = RdEngine(KIND, guard="off").load_weights(big)
    raw.det_forward(x)
    assert raw.range_overflow() and not raw.range_overflow()          # raised once, cleared by the read
    eng = RdEngine(KIND).load_weights(big)                            # default guard="sync": the forward itself falls back
    got = eng.det_forward(x)
    assert eng.precision == "fp32" and eng.range_fallbacks == 1
    assert torch.equal(got, ref)


@pytest.mark.parametrize("stem", ["multi_PP-OCRv3_det_mobile", "en_PP-OCRv3_det_mobile"])
def test_session_from_cfg_resolves_the_kind_by_stem(tmp_path, golden_dir, stem):
    from rapiddoc_amd.session import Mi355DetSession
    p = write_weights(tmp_path, stem, _state(golden_dir))
    sess = Mi355DetSession.from_cfg({"model_path": str(p)})
    assert sess.kind == KIND and sess.engine.kind == KIND
    g = np.load(golden_dir / "det3m_seed0_b2_h64_w96.npz")
    y = sess(golden_x(g))
    ps = int(g["maps_ps"])
    assert type(y) is np.ndarray and y.shape == (2, 1, 64, 96) and y.dtype == np.float32
    e = float(np.abs(y[:, :, ::ps, ::ps] - g["maps"]).max())
    print(f"\n[det v3 mobile session {stem}] max |maps - reference| = {e:.3e}")
    assert e <= TOL


def test_page_pipeline_with_this_detector_and_a_multilingual_recogniser(golden_dir):
    from rapiddoc_amd.engine import RdEngine
    from rapiddoc_amd.pages import synth_batch
    from rapiddoc_amd.pipeline import PagePipeline
    from rapiddoc_amd.session import Mi355DetSession
    REC = "ppocr_rec_mv1e"
    st_det = _state(golden_dir)
    st_rec = W.synth_state_dict(W.load_manifest(golden_dir / "manifest_ppocr_rec_mv1e_latin.json"), 0, kind=REC)
    with pytest.raises(ValueError):
        PagePipeline({KIND: st_det, "ppocrv5_det_mobile": _state(golden_dir, "ppocrv5_det_mobile", gains="ppocrv5_det_mobile"), REC: st_rec})
    pipe = PagePipeline({KIND: st_det, REC: st_rec}, n_rec_streams=2)
    assert pipe.det_kind == KIND and pipe.det.kind == KIND and pipe.rec_kind == REC
    pages_np, _boxes = synth_batch(3, 2)
    pages = torch.from_numpy(pages_np).cuda()
    maps, det_hw = pipe.det_forward(pages)
    maps = maps.clone()
    assert not pipe.det.check_range_and_fallback()
    x = pipe.det_preprocess(pages)[0]
    assert maps.shape == (2, 1, *det_hw) and torch.equal(maps, RdEngine(KIND).load_weights(st_det).det_forward(x))
    sess = Mi355DetSession(W.to_safetensors_bytes(st_det))
    assert sess.kind == KIND and np.array_equal(sess(x.cpu().numpy()), maps.cpu().numpy())      # the session's map, bit for bit
    page_hw = tuple(pages_np.shape[1:3])
    dev = pipe.boxes_from_maps_device(maps, page_hw)
    host = pipe.boxes_from_maps(maps.cpu().numpy(), page_hw)
    assert len(dev) == len(host) == 2
    for a, b in zip(dev, host):
        assert a.shape == b.shape and np.array_equal(a, b)
