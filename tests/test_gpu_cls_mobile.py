"""GPU: the text-line direction classifier (`model_kind "ppocr_cls_mobile"`: MobileNetV3 small scale 0.35 with squeeze-excite + ClsHead)
against the fixtures minted from the reference's own modules (tests/golden/make_golden_cls_mobile.py) on both routes (RD_CLS_FUSED=0: the
chain of separate operators, 1: cls_line_kernel, the whole network in one launch), the kernels of csrc/kernels_mbv3s.hip alone against
float64, launch invariance, the device-side 180-degree turn, and the session / page pipeline on top of it.  (Manifest, kind selection and the
float64 restatement of the folded graph: tests/test_cls_mobile_host.py, whose oracle this file shares.)

Bounds: probabilities 1e-3 absolute; logits, pooled features and block outputs 1e-3 * max(1, max |ref|) (the project's fixture bounds); a
kernel alone against float64 2e-5 * max(1, max |ref|), the bound kernels_mbv3 is held to.  Figures are printed before they are asserted
(run with -s)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kind_helpers import HSWISH, RELU, act64, check_out, engine_cache, out_buffer, strided, write_weights
from rapiddoc_amd import _lib
from rapiddoc_amd import weights as W
from test_cls_mobile_host import KIND, STEM, block64, golden_x, hsig_paddle64, oracle64, state

pytestmark = pytest.mark.gpu
TOL = 1e-3
KTOL = 2e-5
TAGS = ["b7_h48_w192", "b1_h48_w192", "b3_h40_w100"]
THRESH, NEAR = 0.9, 1e-3

# one engine per (precision, route): RD_CLS_FUSED is read when a plan is built, and every plan of such a handle is built inside `_with_route`
_engine = engine_cache(KIND, state=lambda golden_dir, _fused: state(golden_dir))


class _with_route:
    def __init__(self, fused):
        self.fused = fused

    def __enter__(self):
        self.old = os.environ.get("RD_CLS_FUSED")
        os.environ["RD_CLS_FUSED"] = self.fused

    def __exit__(self, *a):
        if self.old is None:
            del os.environ["RD_CLS_FUSED"]
        else:
            os.environ["RD_CLS_FUSED"] = self.old


def _ops(eng, shape):
    eng.set_profiling(True)
    eng.profile_log.clear()
    eng.cls_forward(torch.zeros(shape, device="cuda"))
    got = [(r["name"], r["kind"], r["cfg"]) for r in eng.profile_log]
    eng.set_profiling(False)
    return got


# ---------------------------------------------------------------------------------------------------------------- fixtures through the C-ABI
@pytest.mark.parametrize("precision", ["auto", "fp32"])
@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("tag", TAGS)
def test_whole_network_matches_the_reference_fixtures(golden_dir, tag, fused, precision):
    eng = _engine(golden_dir, precision, fused)
    g = np.load(golden_dir / f"cls_seed0_{tag}.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    B = x.shape[0]
    with _with_route(fused):
        out = torch.full((B, 2), float("nan"), device="cuda")       # handed over prefilled with NaN: must come back fully written
        prob, aux, stages = eng.cls_forward(x, out=out, want_stages=True)
        assert prob is out
        prob2, aux2 = eng.cls_forward(x, want_aux=True)
        plain = eng.cls_forward(x)
        kinds = [k for _n, k, _c in _ops(eng, tuple(x.shape))]
    assert torch.equal(plain, prob) and torch.equal(prob2, prob) and torch.equal(aux2, aux)      # the debug outputs do not move the result
    assert ("cls_line" in kinds) == (fused == "1") and (len(kinds) == 1) == (fused == "1")       # 48 x 192 and 40 x 100 both fit the fused kernel
    assert not eng.range_overflow()
    got = {"prob": prob, "logits": aux[:, :2], "feat": aux[:, 2:], "b0": stages[0], "b3": stages[1], "b8": stages[2], "b10": stages[3]}
    msgs, bad = [], []
    for name, y in got.items():
        assert not bool(torch.isnan(y).any()), f"{name}: an output element was not written"
        ref = g[name]
        assert tuple(y.shape) == ref.shape, (name, tuple(y.shape), ref.shape)
        e = float(np.abs(y.cpu().numpy().astype(np.float64) - ref).max())
        bound = TOL if name == "prob" else TOL * max(1.0, float(np.abs(ref).max()))
        msgs.append(f"{name} {e:.3e} (bound {bound:.3e})")
        if not e <= bound:
            bad.append(name)
    print(f"\n[cls mobile {tag} {precision} RD_CLS_FUSED={fused}] max-abs errors: " + ", ".join(msgs))
    assert not bad, bad
    # labels and >= 0.9 decisions on every line outside the generator's left-out set
    summary = json.loads((golden_dir / "summary_cls_mobile.json").read_text())
    left = set(summary["fixtures"][tag]["left_out"])
    assert len(left) * 10 <= B or B < 10 and not left
    p, r = prob.cpu().numpy(), g["prob"]
    for i in range(B):
        if i in left:
            continue
        assert (p[i, 1] > p[i, 0]) == (r[i, 1] > r[i, 0]) and (p[i, 1] >= THRESH) == (r[i, 1] >= THRESH), (tag, i, p[i], r[i])


def test_the_48_line_draw_gives_the_generators_decisions(golden_dir):
    """The generator's spread conditions were asserted over the 7-line fixture plus this draw; its probabilities are in the summary."""
    summary = json.loads((golden_dir / "summary_cls_mobile.json").read_text())
    d = summary["draw48"]
    x, _ = W.synth_cls_lines(int(d["x_seed"]), 48, 48, 192)
    ref = np.asarray(d["p1"])
    left = set(d["left_out"])
    assert len(left) * 10 <= 48
    for fused in ("0", "1"):
        with _with_route(fused):
            p = _engine(golden_dir, "auto", fused).cls_forward(torch.from_numpy(x).cuda()).cpu().numpy()
        e = float(np.abs(p[:, 1] - ref).max())
        print(f"\n[cls mobile draw48 RD_CLS_FUSED={fused}] max |p1 - reference| = {e:.3e}")
        assert e <= TOL
        keep = [i for i in range(48) if i not in left]
        assert np.array_equal((p[keep, 1] > p[keep, 0]), ref[keep] > 0.5) and np.array_equal(p[keep, 1] >= THRESH, ref[keep] >= THRESH)


def test_geometry_that_leaves_an_empty_map_is_explained(golden_dir):
    from rapiddoc_amd.engine import EngineError
    for fused in ("0", "1"):
        eng = _engine(golden_dir, "auto", fused)
        with _with_route(fused):
            for shape in ((1, 3, 32, 192), (1, 3, 48, 2)):
                with pytest.raises(EngineError, match="empty map"):
                    eng.cls_forward(torch.zeros(shape, device="cuda"))
            assert eng.workspace_bytes(2, 48, 192) > 0 and eng.workspace_bytes(2, 48, 192, 1) > 0


# ---------------------------------------------------------------------------------------------------------------- invariance
@pytest.mark.parametrize("fused,precision", [("1", "auto"), ("1", "fp32"), ("0", "fp32")])
def test_a_line_does_not_depend_on_the_launch_it_rides_in(golden_dir, fused, precision):
    eng = _engine(golden_dir, precision, fused)
    g = np.load(golden_dir / "cls_seed0_b7_h48_w192.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    with _with_route(fused):
        p7, a7 = eng.cls_forward(x, want_aux=True)
        p7, a7 = p7.clone(), a7.clone()
        p1, a1 = eng.cls_forward(x[3:4].contiguous(), want_aux=True)
        p2, a2 = eng.cls_forward(x[2:4].contiguous(), want_aux=True)
    assert torch.equal(p1[0], p7[3]) and torch.equal(a1[0], a7[3])
    assert torch.equal(p2[1], p7[3]) and torch.equal(a2[1], a7[3])


@pytest.mark.parametrize("fused", ["0", "1"])
def test_op_list_follows_the_network_not_the_batch(golden_dir, fused):
    eng = _engine(golden_dir, "auto", fused)
    with _with_route(fused):
        a = _ops(eng, (1, 3, 48, 192))
        assert a == _ops(eng, (2, 3, 48, 192)) == _ops(eng, (7, 3, 48, 192))
    kinds = [k for _n, k, _c in a]
    if fused == "1":
        assert kinds == ["cls_line"]
        return
    assert kinds.count("cls_tail") == 1 and kinds[0] == "stem3x3s2" and "cls_line" not in kinds
    assert sum(k.startswith("mbv3s_dw") for k in kinds) == 11 and kinds.count("se_fc") == 9 and kinds.count("scale") == 9
    assert sum(k == "conv1x1" for k in kinds) == 23               # 11 expand + 11 linear + conv2


# ---------------------------------------------------------------------------------------------------------------- the kernels alone
MAPS = [(2, 3), (3, 35), (6, 33), (12, 70)]
# (cin, mid, cout, k, row stride, squeeze-excite, act, shortcut)
KBLOCKS = [(8, 8, 8, 3, 2, True, RELU, False), (8, 32, 8, 3, 1, False, RELU, True), (16, 88, 16, 5, 1, True, HSWISH, True),
           (16, 104, 32, 5, 2, True, HSWISH, False), (32, 200, 32, 5, 1, True, HSWISH, True)]


def _debug_dw(x, w, b, K, SH, pre_act, post_act, xld=None, yld=None, max_blocks=0):
    fn = _lib.load().rd_debug_mbv3s_dw
    N, H, W_, Cn = x.shape
    xld, yld = xld or Cn, yld or Cn
    OH = (H - 1) // SH + 1
    xb = strided(x, xld)
    buf, view, n_out = out_buffer(N, OH, W_, Cn, yld)
    wk = w.reshape(Cn, K * K).t().contiguous()                           # [K*K][C]
    ms = fn(N, H, W_, Cn, K, SH, 1, pre_act, post_act, xld, yld, 0, max_blocks, xb.data_ptr(), wk.data_ptr(), b.data_ptr(), buf.data_ptr())
    assert ms >= 0, "the kernel does not serve this geometry"
    return check_out(buf, view, n_out, Cn)


def _dw_ref(x, w, b, K, SH, pre_act, post_act):
    xd = act64(x.permute(0, 3, 1, 2).double(), pre_act)
    y = F.conv2d(xd, w.double(), b.double(), stride=(SH, 1), padding=K // 2, groups=x.shape[3])
    return act64(y, post_act).permute(0, 2, 3, 1)


@pytest.mark.parametrize("K,SH,Cn,pre_act,post_act", [(3, 2, 8, 0, RELU), (3, 1, 32, 0, RELU), (5, 1, 88, HSWISH, HSWISH), (5, 2, 104, HSWISH, HSWISH),
                                                      (5, 1, 200, HSWISH, HSWISH), (3, 2, 24, RELU, 0)])
def test_depthwise_kernel_matches_fp64(K, SH, Cn, pre_act, post_act):
    """mbv3s_dw_kernel<K, SH, 1>: N = 2, inputs spanning +-4, the four maps, contiguous and with row strides above C."""
    for H, W_ in MAPS:
        g = torch.Generator(device="cuda").manual_seed(H * 1000 + Cn + 10 * K + SH)
        x = torch.rand((2, H, W_, Cn), device="cuda", generator=g) * 8 - 4
        w = (torch.rand((Cn, 1, K, K), device="cuda", generator=g) - 0.5) * (1.2 / K)
        b = torch.rand((Cn,), device="cuda", generator=g) - 0.5
        ref = _dw_ref(x, w, b, K, SH, pre_act, post_act)
        bound = KTOL * max(1.0, ref.abs().max().item())
        for xld, yld in ((Cn, Cn), (Cn + 8, Cn + 4)):
            y = _debug_dw(x, w, b, K, SH, pre_act, post_act, xld, yld)
            e = (y.double() - ref).abs().max().item()
            print(f"\n[mbv3s dw 2x{H}x{W_}x{Cn} k{K} s({SH},1) pre {pre_act} post {post_act} ld {xld}/{yld}] max |y - fp64| {e:.3e} (bound {bound:.3e})")
            assert y.shape == ref.shape and e < bound


def test_depthwise_kernel_declines_what_it_does_not_serve():
    fn = _lib.load().rd_debug_mbv3s_dw
    t = torch.zeros(4096, device="cuda")
    for Cn, K, SH, SW in ((12, 3, 1, 1), (8, 7, 1, 1), (8, 3, 3, 1), (8, 3, 1, 2)):
        assert fn(1, 4, 4, Cn, K, SH, SW, 0, 0, Cn, Cn, 0, 0, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr()) < 0
    assert fn(1, 4, 4, 8, 3, 1, 1, 0, 0, 8, 8, 0, 0, t.data_ptr() + 4, t.data_ptr(), t.data_ptr(), t.data_ptr()) < 0      # misaligned view


@pytest.mark.parametrize("K,SH", [(3, 2), (5, 1)])
def test_depthwise_kernel_grid_stride_loop(K, SH):
    """max_blocks 1 and 3 against the uncapped launch, bit for bit: 2 x 12 x 70 x 104 is 6 - 12 workgroups' worth of work."""
    g = torch.Generator(device="cuda").manual_seed(7 + K)
    x = torch.rand((2, 12, 70, 104), device="cuda", generator=g) * 8 - 4
    w = (torch.rand((104, 1, K, K), device="cuda", generator=g) - 0.5) * (1.2 / K)
    b = torch.rand((104,), device="cuda", generator=g) - 0.5
    full = _debug_dw(x, w, b, K, SH, HSWISH, HSWISH).clone()
    assert (full.double() - _dw_ref(x, w, b, K, SH, HSWISH, HSWISH)).abs().max().item() < KTOL * max(1.0, full.abs().max().item())
    for cap in (3, 1):
        assert torch.equal(_debug_dw(x, w, b, K, SH, HSWISH, HSWISH, max_blocks=cap), full)


def _block_weights(cin, mid, cout, K, se, seed):
    """Folded weights of one block.  The squeeze-excite's second bias spans +-6, so that 0.2 v + 0.5 leaves [0, 1] on both sides for some
    channels and stays inside for others."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.rand(s, device="cuda", generator=g) - 0.5
    p = dict(we=r(mid, cin) * (2.4 / cin ** 0.5), be=r(mid), wd=r(mid, 1, K, K) * (2.4 / K), bd=r(mid), wl=r(cout, mid) * (2.4 / mid ** 0.5), bl=r(cout))
    if se:
        cr = mid // 4
        p.update(w1=r(cr, mid) * (2.0 / mid ** 0.5), b1=r(cr), w2=r(mid, cr) * (2.0 / cr ** 0.5), b2=r(mid) * 12.0)
    return p


def _block_ref(x, p, K, SH, act, se, shortcut, gate_fn=hsig_paddle64, halo_act_bias=False):
    """float64, through the host test's block64; halo_act_bias: the WRONG block whose depthwise padding holds act(be) instead of zero"""
    a = "relu" if act == RELU else "hswish"
    d = lambda t: t.double().cpu()
    xn = d(x).permute(0, 3, 1, 2)
    sew = (d(p["w1"]), d(p["b1"]), d(p["w2"]), d(p["b2"])) if se else None
    we, wl = d(p["we"])[:, :, None, None], d(p["wl"])[:, :, None, None]
    if not halo_act_bias:
        y, gate = block64(xn, we, d(p["be"]), d(p["wd"]), d(p["bd"]), wl, d(p["bl"]), K, SH, a, sew, shortcut, gate_fn)
        return y.permute(0, 2, 3, 1), gate
    P = K // 2
    e = F.conv2d(F.pad(xn, (P, P, P, P)), we, d(p["be"]))
    e = F.relu(e) if act == RELU else e * torch.clamp(e + 3.0, 0.0, 6.0) / 6.0
    dd = F.conv2d(e, d(p["wd"]), d(p["bd"]), stride=(SH, 1), groups=e.shape[1])
    dd = F.relu(dd) if act == RELU else dd * torch.clamp(dd + 3.0, 0.0, 6.0) / 6.0
    if se:
        gate = gate_fn(F.relu(dd.mean(dim=(2, 3)) @ sew[0].t() + sew[1]) @ sew[2].t() + sew[3])
        dd = dd * gate[:, :, None, None]
    y = F.conv2d(dd, wl, d(p["bl"]))
    return (xn + y if shortcut else y).permute(0, 2, 3, 1), None


def _debug_block(route, x, p, K, SH, act, se, shortcut, xld, yld):
    fn = _lib.load().rd_debug_mbv3s_block
    N, H, W_, cin = x.shape
    mid, cout = p["we"].shape[0], p["wl"].shape[0]
    OH = (H - 1) // SH + 1
    xb = strided(x, xld)
    buf, view, n_out = out_buffer(N, OH, W_, cout, yld)
    wd = p["wd"].reshape(mid, K * K).t().contiguous()
    keep = [p["we"].contiguous(), p["wl"].contiguous()] + ([p["w1"].contiguous(), p["w2"].contiguous()] if se else [])
    ptr = lambda k: p[k].data_ptr() if k in p else None
    ms = fn(route, N, H, W_, cin, mid, cout, K, SH, act, 1 if se else 0, 1 if shortcut else 0, xld, yld, 0, xb.data_ptr(), keep[0].data_ptr(), ptr("be"),
            wd.data_ptr(), ptr("bd"), keep[2].data_ptr() if se else None, ptr("b1"), keep[3].data_ptr() if se else None, ptr("b2"), keep[1].data_ptr(),
            ptr("bl"), buf.data_ptr())
    assert ms >= 0, "the route does not serve this geometry"
    return check_out(buf, view, n_out, cout)


@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("blk", range(len(KBLOCKS)))
def test_block_matches_fp64_on_either_route(blk, route):
    """One inverted-residual block through rd_debug_mbv3s_block: route 0 = the operators the plan chains, route 1 = the block as
    cls_line_kernel runs it.  N = 2, inputs in +-4, the four maps, contiguous views and row strides above C.  On the float64 side: the
    gate is clamped at 0 for some channels, at 1 for others and strictly inside for the rest; a depthwise halo of act(bias) instead of zero
    and a gate with torch's 1 / 6 slope both miss by many bounds."""
    cin, mid, cout, K, SH, se, act, shortcut = KBLOCKS[blk]
    p = _block_weights(cin, mid, cout, K, se, 100 + blk)
    shares = np.zeros(3)
    for H, W_ in MAPS:
        g = torch.Generator(device="cuda").manual_seed(H * 100 + W_ + blk)
        x = torch.rand((2, H, W_, cin), device="cuda", generator=g) * 8 - 4
        ref, gate = _block_ref(x, p, K, SH, act, se, shortcut)
        bound = KTOL * max(1.0, ref.abs().max().item())
        wrong_halo = (_block_ref(x, p, K, SH, act, se, shortcut, halo_act_bias=True)[0] - ref).abs().max().item()
        assert wrong_halo > 10 * bound, (wrong_halo, bound)
        if se:
            shares += [float((gate == 0).sum()), float((gate == 1).sum()), float(((gate > 0) & (gate < 1)).sum())]
            wrong_gate = (_block_ref(x, p, K, SH, act, se, shortcut, gate_fn=lambda t: torch.clamp(t / 6.0 + 0.5, 0.0, 1.0))[0] - ref).abs().max().item()
            assert wrong_gate > 10 * bound, (wrong_gate, bound)
        for xld, yld in ((cin, cout), (cin + 8, cout + 4)):
            y = _debug_block(route, x, p, K, SH, act, se, shortcut, xld, yld)
            e = (y.double().cpu() - ref).abs().max().item()
            print(f"\n[mbv3s block {cin}-{mid}-{cout} k{K} s({SH},1) route {route} 2x{H}x{W_} ld {xld}/{yld}] max |y - fp64| {e:.3e} (bound {bound:.3e}; "
                  f"halo of act(bias) misses by {wrong_halo:.2e})")
            assert tuple(y.shape) == tuple(ref.shape) and e < bound
    if se:
        assert (shares > 0).all(), shares


def test_fused_block_declines_what_it_cannot_hold():
    """cls_block_kernel keeps at least 4 expanded channels of the whole input map in 72 KB of LDS: a map above 4608 pixels goes to route 0"""
    cin, mid, cout, K, SH, se, act, shortcut = KBLOCKS[1]
    p = _block_weights(cin, mid, cout, K, se, 5)
    x = torch.zeros((1, 50, 100, cin), device="cuda")
    fn = _lib.load().rd_debug_mbv3s_block
    y = torch.zeros((1, 50, 100, cout), device="cuda")
    wd = p["wd"].reshape(mid, K * K).t().contiguous()
    args = lambda route: (route, 1, 50, 100, cin, mid, cout, K, SH, act, 0, 1, cin, cout, 0, x.data_ptr(), p["we"].data_ptr(), p["be"].data_ptr(), wd.data_ptr(),
                          p["bd"].data_ptr(), None, None, None, None, p["wl"].data_ptr(), p["bl"].data_ptr(), y.data_ptr())
    assert fn(*args(1)) < 0 and fn(*args(0)) >= 0 and fn(*args(2)) < 0


def test_a_width_the_fused_kernel_cannot_hold_takes_the_separate_operators(golden_dir):
    """48 x 800: conv1's map is 24 x 400 = 9600 pixels, above the 4608 the slice buffer holds at 4 channels: cls_line_plan declines, the
    plan is the unfused chain even under RD_CLS_FUSED=1, and equals the RD_CLS_FUSED=0 result bit for bit."""
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (2, 3, 48, 800)).astype(np.float32)).cuda()
    with _with_route("1"):
        e1 = _engine(golden_dir, "fp32", "1")
        kinds = [k for _n, k, _c in _ops(e1, tuple(x.shape))]
        p1 = e1.cls_forward(x).clone()
    assert "cls_line" not in kinds and kinds.count("cls_tail") == 1
    with _with_route("0"):
        p0 = _engine(golden_dir, "fp32", "0").cls_forward(x).clone()
    assert torch.equal(p0, p1)
    ref = oracle64(state(golden_dir), x.cpu().numpy())["prob"]
    assert float(np.abs(p0.cpu().numpy() - ref).max()) <= TOL


# ---------------------------------------------------------------------------------------------------------------- the 180-degree turn
LINE_DTYPE = np.dtype([("page", "<i4"), ("out_w", "<i4"), ("crop_w", "<i4"), ("crop_h", "<i4"), ("rot90", "<i4"), ("scratch_off", "<i4"), ("m", "<f8", (9,))])


def test_flip_kernel_turns_the_flagged_crops_only(golden_dir):
    from rapiddoc_amd.pipeline import cls_flip_rule
    sizes = [(1, 1), (1, 7), (5, 4), (37, 211), (5, 4), (1, 7), (37, 211), (1, 1)]           # (h, w)
    g = np.load(golden_dir / "cls_seed0_b7_h48_w192.npz")
    fp = g["prob"].astype(np.float32)
    order = np.argsort(fp[:, 1])
    # fixture probabilities around the threshold, plus the exact threshold as a score (>= turns) and one float below it (does not)
    thresh = float(np.float32(0.5) * (fp[order[-2], 1] + fp[order[-3], 1]))
    prob = np.stack([fp[order[-1]], fp[order[-2]], fp[order[-3]], fp[order[0]], fp[order[-1]], fp[order[1]],
                     np.float32([1 - thresh, thresh]), np.float32([1 - thresh, np.nextafter(np.float32(thresh), np.float32(0))])]).astype(np.float32)
    want = cls_flip_rule(prob, thresh)
    assert want.tolist() == [True, True, False, False, True, False, True, False]
    rng = np.random.default_rng(11)
    gap = 48                                                   # bytes between crops, which nobody may touch
    descs = np.zeros(len(sizes), dtype=LINE_DTYPE)
    off, crops = gap, []
    for i, (h, w) in enumerate(sizes):
        descs[i]["crop_w"], descs[i]["crop_h"], descs[i]["scratch_off"], descs[i]["rot90"] = w, h, off, i % 2
        crops.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        off += (h * w * 3 + 15) // 16 * 16 + gap
    host = rng.integers(0, 256, off, dtype=np.uint8)
    for d, c in zip(descs, crops):
        host[d["scratch_off"]: d["scratch_off"] + c.size] = c.reshape(-1)
    expect = host.copy()
    for d, c, f in zip(descs, crops, want):
        if f:
            expect[d["scratch_off"]: d["scratch_off"] + c.size] = c[::-1, ::-1].reshape(-1)
    scratch = torch.from_numpy(host).cuda()
    descs_dev = torch.from_numpy(descs.view(np.uint8)).cuda()
    prob_dev = torch.from_numpy(prob).cuda()
    flipped = torch.full((len(sizes),), -1, dtype=torch.int32, device="cuda")
    rc = _lib.load().rd_line_flip180_batch(0, descs_dev.data_ptr(), len(sizes), prob_dev.data_ptr(), thresh, scratch.data_ptr(), flipped.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert flipped.cpu().numpy().tolist() == want.astype(np.int32).tolist()
    assert np.array_equal(scratch.cpu().numpy(), expect)       # flipped crops byte for byte; unflagged crops and the gaps untouched
    rc = _lib.load().rd_line_flip180_batch(0, descs_dev.data_ptr(), len(sizes), prob_dev.data_ptr(), thresh, scratch.data_ptr(), flipped.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(scratch.cpu().numpy(), host)       # turning twice is the identity
    assert _lib.load().rd_line_flip180_batch(0, descs_dev.data_ptr(), 0, prob_dev.data_ptr(), thresh, scratch.data_ptr(), flipped.data_ptr(), None) == 0


# ---------------------------------------------------------------------------------------------------------------- session, dispatch
def test_session_from_a_file_and_dispatch(tmp_path, golden_dir, monkeypatch):
    import sys
    import types
    from rapiddoc_amd import session as S
    path = write_weights(tmp_path, STEM, state(golden_dir))
    sess = S.Mi355ClsSession.from_cfg({"model_path": str(path)})
    assert sess.kind == KIND and sess.engine.kind == KIND
    g = np.load(golden_dir / "cls_seed0_b7_h48_w192.npz")
    y = sess(golden_x(g))
    assert type(y) is np.ndarray and y.shape == (7, 2) and y.dtype == np.float32
    e = float(np.abs(y - g["prob"]).max())
    print(f"\n[cls mobile session] max |prob - reference| = {e:.3e}")
    assert e <= TOL and np.allclose(y.sum(axis=1), 1.0, atol=1e-6)
    mods = {"rapidocr": types.ModuleType("rapidocr"), "rapidocr.inference_engine": types.ModuleType("rapidocr.inference_engine"),
            "rapidocr.inference_engine.torch": types.ModuleType("rapidocr.inference_engine.torch")}
    mods["rapidocr"].__path__ = mods["rapidocr.inference_engine"].__path__ = []
    mods["rapidocr.inference_engine.torch"].TorchInferSession = object
    for k, v in mods.items():
        monkeypatch.setitem(sys.modules, k, v)
    S.install_into_rapidocr()
    d = mods["rapidocr.inference_engine.torch"].TorchInferSession
    s2 = d({"task_type": "TaskType.CLS", "model_path": str(path)})
    assert isinstance(s2, S.Mi355ClsSession) and np.array_equal(s2(golden_x(g)), y)
    for cls, name in ((S.Mi355DetSession, "det"), (S.Mi355RecSession, "rec")):
        monkeypatch.setattr(cls, "from_cfg", classmethod(lambda c, cfg, name=name: name))
    assert d({"task_type": "det", "model_path": "x.safetensors"}) == "det" and d({"task_type": "rec", "model_path": "x.safetensors"}) == "rec"


# ---------------------------------------------------------------------------------------------------------------- page pipeline
def _pages_with_turned_lines():
    """Two synthetic pages of six rendered lines each; four of the twelve are drawn turned by 180 degrees"""
    from rapiddoc_amd.pages import synth_page
    from rapiddoc_amd.pipeline import boxes_to_quads
    pages, quads = [], []
    for i, turned in ((11, (1, 4)), (12, (0, 3))):
        page, boxes = synth_page(i, n_lines=6)
        for j in turned:
            x0, y0, x1, y1 = (int(v) for v in boxes[j])
            page[y0:y1, x0:x1] = page[y0:y1, x0:x1][::-1, ::-1].copy()
        pages.append(page)
        quads.append(boxes_to_quads(boxes))
    return np.stack(pages), quads


def test_page_pipeline_turns_the_lines_the_classifier_flags(golden_dir):
    from rapiddoc_amd.pipeline import PagePipeline, cls_flip_rule
    states = {"ppocrv6_det": W.synth_state_dict(W.load_manifest(golden_dir / "manifest_ppocrv6_det.json"), 0),
              "ppocrv6_rec": W.synth_state_dict(W.load_manifest(golden_dir / "manifest_ppocrv6_rec.json"), 0)}
    st_cls = state(golden_dir)
    pages_np, quads = _pages_with_turned_lines()
    pages = torch.from_numpy(pages_np).cuda()
    with pytest.raises(ValueError):
        PagePipeline(states, n_rec_streams=2, use_cls=True)

    def run(pipe):
        pipe.keep_rec_inputs = True
        res = pipe.run_batch(pages, quads_per_page=quads)
        torch.cuda.synchronize()
        rec_in = {}
        for entry in pipe.last_rec_batches:
            for j, i in enumerate(np.asarray(entry[0]).tolist()):
                rec_in[int(i)] = entry[1][j].clone()
        return res, rec_in

    off = PagePipeline(states, n_rec_streams=2)
    assert off.use_cls is False and off.cls_engines == []
    res_off, rec_off = run(off)
    assert all(r.cls is None for r in res_off) and len(rec_off) == 12
    descs, batch_base, starts = off.last_rec_descs
    scratch_off = off._crop_scratch.cpu().numpy().copy()

    # a first pass with the stage on and a threshold nothing reaches: the classifier's own inputs -> the float64 oracle
    probe = PagePipeline({**states, KIND: st_cls}, n_rec_streams=2, use_cls=True, cls_thresh=2.0)
    res_probe, rec_probe = run(probe)
    assert all(torch.equal(rec_probe[i], rec_off[i]) for i in range(12))              # nothing turned: every bit as with the stage off
    assert [c[0] for r in res_probe for c in r.cls] == [False] * 12
    cls_in = {}
    for ids, xc in probe.last_cls_inputs:
        assert tuple(xc.shape[1:]) == (3, 48, 192)
        for j, i in enumerate(np.asarray(ids).tolist()):
            cls_in[int(i)] = xc[j].cpu().numpy()
    xc_all = np.stack([cls_in[i] for i in range(12)])
    # rendered page lines sit far on one side of the fixture head (p1 = 0.9999 ...): the stand-in head of this test is the fixture's with its
    # bias moved by the oracle's median logit difference over these lines, so that both labels occur
    lg = oracle64(st_cls, xc_all)["logits"]
    st_pipe = dict(st_cls)
    st_pipe["head.fc.bias"] = (st_cls["head.fc.bias"] - np.float32([0.0, np.median(lg[:, 1] - lg[:, 0])])).astype(np.float32)
    oracle = oracle64(st_pipe, xc_all)["prob"]
    p1 = oracle[:, 1]
    ones = np.sort(p1[p1 > 0.5])
    assert len(ones) >= 2, "the stand-in weights call fewer than two of the twelve lines turned"
    # the oracle's median score of the label-1 lines; with an odd count the median IS a line's score, so the threshold goes half-way to the next one
    thresh = float(np.median(ones)) if len(ones) % 2 == 0 else float(0.5 * (ones[len(ones) // 2] + ones[len(ones) // 2 + 1]))
    assert np.abs(p1 - thresh).min() > NEAR and np.abs(p1 - 0.5).min() > NEAR, (p1, thresh)
    want = cls_flip_rule(oracle, thresh)
    assert 0 < want.sum() < (p1 > 0.5).sum() + 1 and want.sum() < 12
    print(f"\n[cls mobile pipeline] oracle p1 {np.round(p1, 4).tolist()}, threshold {thresh:.6f}, turned {np.flatnonzero(want).tolist()}")

    on = PagePipeline({**states, KIND: st_pipe}, n_rec_streams=2, use_cls=True, cls_thresh=thresh)
    res_on, rec_on = run(on)
    got = [c for r in res_on for c in r.cls]
    assert [c[0] for c in got] == want.tolist()                                       # PageResult.cls = the oracle's decisions
    assert [c[1] for c in got] == (p1 > 0.5).astype(int).tolist()
    assert np.abs(np.asarray([c[2] for c in got]) - oracle.max(axis=1)).max() <= TOL
    d_on, base_on, starts_on = on.last_rec_descs
    assert np.array_equal(d_on, descs) and np.array_equal(base_on, batch_base)        # the same lines in the same launches
    # expected rec inputs: the stage-off run's uint8 crops, the flagged ones turned in numpy BEFORE the resize, through the same resize call
    keep_ids = np.concatenate([np.asarray(e[0]) for e in off.last_rec_batches])
    flip_scratch = scratch_off.copy()
    for b in range(len(starts) - 1):
        for j in range(int(starts[b]), int(starts[b + 1])):
            if want[int(keep_ids[j])]:
                d = descs[j]
                o, n = int(batch_base[b]) + int(d["scratch_off"]), int(d["crop_w"]) * int(d["crop_h"]) * 3
                flip_scratch[o: o + n] = flip_scratch[o: o + n].reshape(int(d["crop_h"]), int(d["crop_w"]), 3)[::-1, ::-1].reshape(-1)
    fs = torch.from_numpy(flip_scratch).cuda()
    descs_dev = torch.from_numpy(descs.view(np.uint8)).cuda()
    for b, entry in enumerate(off.last_rec_batches):
        nb, wpad = entry[1].shape[0], entry[1].shape[3]
        exp = torch.empty((nb, 3, 48, wpad), device="cuda")
        rc = _lib.load().rd_line_resize_norm_batch(0, descs_dev.data_ptr() + int(starts[b]) * LINE_DTYPE.itemsize, nb, fs.data_ptr() + int(batch_base[b]), 48, wpad, 1,
                                                   exp.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == 0
        for j, i in enumerate(np.asarray(entry[0]).tolist()):
            assert torch.equal(rec_on[int(i)], exp[j]), (i, bool(want[i]))
            assert torch.equal(rec_on[int(i)], rec_off[int(i)]) == (not want[i])      # flagged lines moved, all others are bit-identical
    # the stage-off pipeline, run again behind the two others in this process: its strings and scores are what they were
    res_again, rec_again = run(off)
    assert [[(t, s) for _q, t, s in r.lines] for r in res_again] == [[(t, s) for _q, t, s in r.lines] for r in res_off]
    assert all(torch.equal(rec_again[i], rec_off[i]) for i in range(12))
    with pytest.raises(ValueError):
        on.rec_forward_sources([(pages, quads)], want_words=True)
