"""GPU: the PP-OCRv5 mobile detector (`model_kind "ppocrv5_det_mobile"`: PPLCNetV3 scale 0.75 det + RSEFPN + DBHead) against the fixtures
minted from the reference's own modules (tests/golden/make_golden_det_mobile.py), its launch invariance, the two depthwise kernels of its
backbone alone against float64 (csrc/kernels_lcv3.hip direct, csrc/kernels_lcv3_det.hip LDS-staged), the stride-2 layers' missing
activation, the range guard, and the session / page pipeline on top of it.  (The load-time folds are checked on the CPU:
tests/test_det_mobile_host.py.)

Bounds: `maps` 1e-3 max-abs, the project's stated bound (tests/test_gpu_parity.py); the neck output 1e-3 * max(1, max |ref|), as
tests/test_gpu_det_server.py; a kernel alone against float64 2e-5 * max(1, max |ref|) (the project's bound for its direct convolutions).
Figures are printed before they are asserted (run with -s to see them)."""
import numpy as np
import pytest
import torch

from kind_helpers import GUARD, SENTINEL, check_det_fixture, engine_cache, golden_x, hswish64, synth_state, write_weights
from rapiddoc_amd import _lib
from rapiddoc_amd import weights as W

pytestmark = pytest.mark.gpu
TOL = 1e-3
KIND = "ppocrv5_det_mobile"
TAGS = ["b2_h64_w96", "b1_h160_w224", "b3_h96_w352", "b1_h960_w704"]


def _state(golden_dir, kind=KIND):
    return synth_state(golden_dir, kind, kind=KIND if kind == KIND else None)


_engine = engine_cache(KIND, state=_state)


def _check_against_fixture(eng, golden_dir, tag, label):
    check_det_fixture(eng, golden_dir, tag, label, prefix="det5m", neck_channels=96, name="det mobile", tol=TOL)


@pytest.mark.parametrize("precision", ["auto", "fp32"])
@pytest.mark.parametrize("tag", TAGS)
def test_whole_network_matches_the_reference_fixtures(golden_dir, tag, precision):
    _check_against_fixture(_engine(golden_dir, precision), golden_dir, tag, precision)


def test_whole_network_in_h3_mode(golden_dir):
    _check_against_fixture(_engine(golden_dir, "h3"), golden_dir, "b2_h64_w96", "h3")


@pytest.mark.parametrize("route", ["0", "1"], ids=["direct", "lds2d"])
def test_whole_network_on_either_depthwise_route(golden_dir, monkeypatch, route):
    """RD_LCV3_DW2D=0|1 (read per plan) puts every depthwise layer on one route; both meet the fixture, whichever is a layer's default."""
    from rapiddoc_amd.engine import RdEngine
    monkeypatch.setenv("RD_LCV3_DW2D", route)
    monkeypatch.setenv("RD_PRECISION", "auto")
    eng = RdEngine(KIND, guard="off").load_weights(_state(golden_dir))
    eng.set_profiling(True)
    eng.profile_log.clear()
    _check_against_fixture(eng, golden_dir, "b1_h160_w224", "route " + route)
    dw = [r for r in eng.profile_log if r["kind"].startswith("lcv3_dw")]
    assert len(dw) >= 14 and all(("/lds2d" in r["cfg"]) == (route == "1") for r in dw), [r["cfg"] for r in dw]


def test_stride_2_layers_are_not_activated_and_routes_follow_the_layer(golden_dir):
    """The reference skips the activation of a LearnableRepLayer whose stride is the integer 2 (blocks3.0, 4.0, 5.0, 6.0): those four
    depthwise ops carry `/noact`, the other ten do not; and the route of every layer is the same at two batch sizes and two page sizes."""
    eng = _engine(golden_dir, "auto")

    def ops(shape):
        eng.set_profiling(True)
        eng.profile_log.clear()
        eng.det_forward(torch.zeros(shape, device="cuda"))
        got = [(r["name"], r["cfg"]) for r in eng.profile_log if r["kind"].startswith("lcv3_dw")]
        eng.set_profiling(False)
        return got

    a = ops((1, 3, 64, 96))
    assert len(a) == 14
    noact = [n for n, c in a if c.endswith("/noact")]
    assert noact == [f"backbone.blocks{i}.0.dw_conv.fold.weight" for i in (3, 4, 5, 6)]
    assert a == ops((3, 3, 64, 96)) == ops((1, 3, 160, 224))
    # the per-layer defaults of the A/B table (docs/notebook/v5_mobile_det.md): the staged kernel everywhere but the three 3x3 / stride-2 layers
    direct = [n for n, c in a if "/direct" in c]
    assert direct == [f"backbone.blocks{i}.0.dw_conv.fold.weight" for i in (3, 4, 5)]
    assert all("/lds2d" in c for n, c in a if n not in direct)


def test_a_file_without_the_unused_act_lab_of_the_stride_2_layers_loads(golden_dir):
    """The engine never asks for `dw_conv.act.lab.*` of a stride-2 layer: without those eight tensors the result is the same, bit for bit."""
    from rapiddoc_amd.engine import RdEngine
    st = _state(golden_dir)
    drop = [f"backbone.blocks{i}.0.dw_conv.act.lab.{leaf}" for i in (3, 4, 5, 6) for leaf in ("scale", "bias")]
    assert all(k in st for k in drop)
    slim = {k: v for k, v in st.items() if k not in drop}
    x = torch.from_numpy(golden_x(np.load(golden_dir / "det5m_seed0_b2_h64_w96.npz"))).cuda()
    got = RdEngine(KIND, guard="off").load_weights(slim).det_forward(x)
    assert torch.equal(got, _engine(golden_dir, "auto").det_forward(x))


@pytest.mark.parametrize("precision", ["auto", "fp32"])
def test_an_image_does_not_depend_on_the_launch_it_rides_in(golden_dir, precision):
    eng = _engine(golden_dir, precision)
    g = np.load(golden_dir / "det5m_seed0_b3_h96_w352.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    m3, f3 = eng.det_forward(x, want_neck=True)
    m3, f3 = m3.clone(), f3.clone()
    m1, f1 = eng.det_forward(x[1:2].contiguous(), want_neck=True)
    assert torch.equal(m1[0], m3[1]) and torch.equal(f1[0], f3[1])


# ---------------------------------------------------------------------------------------------------------------- the depthwise kernels alone
def _debug_dw(x, w, b, K, S, pre_act, post_act, aff, route):
    """One layer through rd_debug_lcv3_dw_det (api_debug.cpp).  route 0: lcv3_dw_kernel, 1: lcv3_dw2d_kernel.  The output buffer is prefilled
    with NaN and followed by a guard band that must come back untouched."""
    lib = _lib.load()
    fn = lib.rd_debug_lcv3_dw_det
    N, H, W_, Cn = x.shape
    OH, OW = (H + 2 * (K // 2) - K) // S + 1, (W_ + 2 * (K // 2) - K) // S + 1
    n_out = N * OH * OW * Cn
    buf = torch.full((n_out + GUARD,), float("nan"), device="cuda")
    buf[n_out:] = SENTINEL
    wk = w.reshape(Cn, K * K).t().contiguous()                          # [K*K][C]
    a = np.asarray(aff, dtype=np.float32)
    ms = fn(N, H, W_, Cn, K, S, int(pre_act), int(post_act), route, 0, a.ctypes.data, x.data_ptr(), wk.data_ptr(), b.data_ptr(), buf.data_ptr())
    torch.cuda.synchronize()
    assert ms >= 0, "the route does not serve this geometry"
    assert bool((buf[n_out:] == SENTINEL).all()), "the guard band behind the output was written"
    y = buf[:n_out].view(N, OH, OW, Cn)
    assert not bool(torch.isnan(y).any()), "an output element was not written"
    return y


def _dw_ref(x, w, b, K, S, pre_act, post_act, aff, pad_value=None):
    """float64: activation + affine on the elements inside the map, THEN the zero padding of the convolution.  `pad_value`: the wrong
    reading, where the padding is activated too (hardswish(0) = 0, so it becomes pre_b) - to show that the test tells the two apart."""
    import torch.nn.functional as F
    xd = x.permute(0, 3, 1, 2).double()
    if pre_act:
        xd = aff[0] * hswish64(xd) + aff[1]
    P = K // 2
    xd = F.pad(xd, (P, P, P, P), value=0.0 if pad_value is None else pad_value)
    y = F.conv2d(xd, w.double(), b.double(), stride=S, groups=x.shape[3])
    if post_act:
        y = aff[2] * hswish64(y) + aff[3]
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("K,S", [(3, 1), (3, 2), (5, 1), (5, 2)])
@pytest.mark.parametrize("H,W_,Cn", [
    (2, 3, 384),      # the 1/32 map of a 64 x 96 page: smaller than the halo and than a tile on every side; 24 channel slices
    (9, 35, 16),      # C = 16: one slice, the narrowest map of the network; two row tiles and two column tiles, both ragged; odd H and W
    (17, 33, 48),     # C = 48: three slices, no power of two; one column past a tile; odd H and W under stride 2
    (12, 70, 192),    # three column tiles at stride 1, two at stride 2
])
def test_depthwise_kernels_match_fp64(H, W_, Cn, K, S):
    """Both routes against float64 conv2d, N = 2, inputs spanning +-4, with and without the on-load hardswish + affine and the epilogue's.
    Bound 2e-5 * max(1, max |ref|) per route; the two routes agree within twice that."""
    N = 2
    g = torch.Generator(device="cuda").manual_seed(H * 1000 + Cn + 10 * K + S)
    x = torch.rand((N, H, W_, Cn), device="cuda", generator=g) * 8 - 4
    w = (torch.rand((Cn, 1, K, K), device="cuda", generator=g) - 0.5) * (1.2 / K)
    b = torch.rand((Cn,), device="cuda", generator=g) - 0.5
    aff = (1.1, 0.3, 0.9, -0.2)                                          # pre_s, pre_b (nonzero: padding activated to pre_b would show), post_s, post_b
    for pre_act in (0, 1):
        for post_act in (0, 1):
            ref = _dw_ref(x, w, b, K, S, pre_act, post_act, aff)
            bound = 2e-5 * max(1.0, ref.abs().max().item())
            ys = [_debug_dw(x, w, b, K, S, pre_act, post_act, aff, route) for route in (0, 1)]
            errs = [(y.double() - ref).abs().max().item() for y in ys]
            d = (ys[0] - ys[1]).abs().max().item()
            print(f"\n[lcv3 dw {N}x{H}x{W_}x{Cn} k{K} s{S} pre {pre_act} post {post_act}] max |y - fp64|: direct {errs[0]:.3e}, lds2d {errs[1]:.3e} "
                  f"(bound {bound:.3e}, max |ref| {ref.abs().max().item():.2f}); |direct - lds2d| {d:.3e}")
            assert ys[0].shape == ref.shape
            assert errs[0] < bound and errs[1] < bound
            assert d < 2 * bound
            if pre_act:
                # a border output equals the zero-padded reference, and the reference with the padding at pre_b is far from it
                wrong = _dw_ref(x, w, b, K, S, pre_act, post_act, aff, pad_value=aff[1])
                assert (wrong[:, 0] - ref[:, 0]).abs().max().item() > 100 * bound
                for y in ys:
                    assert (y[:, 0].double() - ref[:, 0]).abs().max().item() < bound
                    assert (y[:, :, 0].double() - ref[:, :, 0]).abs().max().item() < bound
                    assert (y[:, -1].double() - ref[:, -1]).abs().max().item() < bound
                    assert (y[:, :, -1].double() - ref[:, :, -1]).abs().max().item() < bound


def test_the_staged_route_refuses_what_it_does_not_serve():
    x = torch.zeros((1, 4, 4, 8), device="cuda")
    w = torch.zeros((8, 1, 3, 3), device="cuda")
    b = torch.zeros((8,), device="cuda")
    with pytest.raises(AssertionError, match="does not serve"):
        _debug_dw(x, w, b, 3, 1, 0, 0, (1, 0, 1, 0), 1)                  # C = 8: below a 16-channel slice
    _debug_dw(x, w, b, 3, 1, 0, 0, (1, 0, 1, 0), 0)                      # the direct kernel takes it


def test_a_stride_2_block_matches_fp64_from_the_state_dict(golden_dir):
    """blocks3.0 from the synthetic state dict in float64, as the reference's forward reads: dw_conv = lab(sum of branches), NO activation and
    NO act.lab (stride == 2), then pw_conv = act.lab(hardswish(lab(sum of branches))).  The engine's form: the folded depthwise layer
    through the debug entry with post_act = 0, the folded pointwise layer as a matrix product, then the consumer's hardswish + affine."""
    import torch.nn.functional as F
    st = {k: torch.from_numpy(v) for k, v in _state(golden_dir).items()}
    blob = W.to_safetensors_bytes(_state(golden_dir))
    lib = _lib.load()
    fn = lib.rd_debug_derived_tensor

    def derived(name, shape):
        out = np.full(shape, np.nan, np.float32)
        assert fn(KIND.encode(), blob, len(blob), name.encode(), out.ctypes.data, out.size) == out.size
        return torch.from_numpy(out).cuda()

    def bn(t, q):
        g, be, m, v = (st[f"{q}.{n}"].double()[None, :, None, None] for n in ("weight", "bias", "running_mean", "running_var"))
        return (t - m) / torch.sqrt(v + 1e-5) * g + be

    def rep_layer(t, p, stride, groups, k, act):
        out = 0
        for i in range(4):
            out = out + bn(F.conv2d(t, st[f"{p}.conv_kxk.{i}.conv.weight"].double(), stride=stride, padding=k // 2, groups=groups), f"{p}.conv_kxk.{i}.bn")
        if k > 1:
            out = out + bn(F.conv2d(t, st[f"{p}.conv_1x1.conv.weight"].double(), stride=stride, groups=groups), f"{p}.conv_1x1.bn")
        assert f"{p}.identity.weight" not in st
        out = out * st[f"{p}.lab.scale"].double() + st[f"{p}.lab.bias"].double()
        if act:
            out = hswish64(out) * st[f"{p}.act.lab.scale"].double() + st[f"{p}.act.lab.bias"].double()
        return out

    p = "backbone.blocks3.0"
    x = torch.rand((2, 13, 22, 32), generator=torch.Generator().manual_seed(30)) * 8 - 4
    xd = x.permute(0, 3, 1, 2).double()
    mid = rep_layer(xd, p + ".dw_conv", 2, 32, 3, act=False)              # stride == 2: `if self.stride != 2: out = self.act(out)`
    ref = rep_layer(mid, p + ".pw_conv", 1, 1, 1, act=True).permute(0, 2, 3, 1)
    wrong = rep_layer(rep_layer(xd, p + ".dw_conv", 2, 32, 3, act=True), p + ".pw_conv", 1, 1, 1, act=True).permute(0, 2, 3, 1)

    dw_w, dw_b = derived(p + ".dw_conv.fold.weight", (32, 1, 3, 3)), derived(p + ".dw_conv.fold.bias", (32,))
    pw_w, pw_b = derived(p + ".pw_conv.fold.weight", (48, 32)), derived(p + ".pw_conv.fold.bias", (48,))
    bound = 2e-5 * max(1.0, ref.abs().max().item())
    for route in (0, 1):
        t = _debug_dw(x.cuda(), dw_w, dw_b, 3, 2, 0, 0, (1, 0, 1, 0), route)
        e_mid = (t.double().cpu() - mid.permute(0, 2, 3, 1)).abs().max().item()
        y = t.double() @ pw_w.double().t() + pw_b.double()
        y = (hswish64(y) * float(st[p + ".pw_conv.act.lab.scale"]) + float(st[p + ".pw_conv.act.lab.bias"])).cpu()
        e = (y - ref).abs().max().item()
        print(f"\n[blocks3.0 route {route}] max |dw - fp64| = {e_mid:.3e}, max |block - fp64| = {e:.3e} (bound {bound:.3e}, max |ref| {ref.abs().max().item():.2f}); "
              f"with the unused act.lab applied the block would be off by {(wrong - ref).abs().max().item():.3e}")
        assert e_mid < 2e-5 * max(1.0, mid.abs().max().item())
        assert e < bound
    assert (wrong - ref).abs().max().item() > 100 * bound


# ---------------------------------------------------------------------------------------------------------------- guard, session, pipeline
def test_range_guard_falls_back_to_the_fp32_mode_bit_for_bit(golden_dir, monkeypatch):
    """layer_list.1's bias times 1e7 puts the level-1 neck feature (the folded 1x1's output, ~1e5..1e6) beyond the fp16 range; the neck's
    3x3 convolutions that read it are split layers in `auto`."""
    from rapiddoc_amd.engine import RdEngine
    monkeypatch.setenv("RD_PRECISION", "auto")
    big = dict(_state(golden_dir))
    big["backbone.layer_list.1.bias"] = big["backbone.layer_list.1.bias"] * np.float32(1e7)
    g = np.load(golden_dir / "det5m_seed0_b2_h64_w96.npz")
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


def test_session_from_cfg_resolves_the_kind_by_stem(tmp_path, golden_dir):
    from rapiddoc_amd.session import Mi355DetSession
    p = write_weights(tmp_path, "ch_PP-OCRv5_det_mobile", _state(golden_dir))
    sess = Mi355DetSession.from_cfg({"model_path": str(p)})
    assert sess.kind == KIND and sess.engine.kind == KIND
    g = np.load(golden_dir / "det5m_seed0_b2_h64_w96.npz")
    y = sess(golden_x(g))
    ps = int(g["maps_ps"])
    assert type(y) is np.ndarray and y.shape == (2, 1, 64, 96) and y.dtype == np.float32
    e = float(np.abs(y[:, :, ::ps, ::ps] - g["maps"]).max())
    print(f"\n[det mobile session] max |maps - reference| = {e:.3e}")
    assert e <= TOL


def test_page_pipeline_with_the_mobile_detector(golden_dir):
    from rapiddoc_amd.engine import RdEngine
    from rapiddoc_amd.pages import synth_batch
    from rapiddoc_amd.pipeline import PagePipeline, boxes_to_quads
    REC = "ppocrv5_rec_mobile"
    st_det, st_v6, st_rec = _state(golden_dir), _state(golden_dir, "ppocrv6_det"), _state(golden_dir, REC)
    with pytest.raises(ValueError):
        PagePipeline({KIND: st_det, "ppocrv6_det": st_v6, REC: st_rec})
    with pytest.raises(ValueError):
        PagePipeline({KIND: st_det, "ppocrv5_det_server": _state(golden_dir, "ppocrv5_det_server"), REC: st_rec})
    with pytest.raises(ValueError):
        PagePipeline({REC: st_rec})
    pipe = PagePipeline({KIND: st_det, REC: st_rec}, n_rec_streams=2)
    assert pipe.det_kind == KIND and pipe.det.kind == KIND and pipe.rec_kind == REC
    pages_np, boxes = synth_batch(3, 2)
    pages = torch.from_numpy(pages_np).cuda()
    maps, det_hw = pipe.det_forward(pages)
    maps = maps.clone()
    assert not pipe.det.check_range_and_fallback()
    x = pipe.det_preprocess(pages)[0]
    assert maps.shape == (2, 1, *det_hw) and torch.equal(maps, RdEngine(KIND).load_weights(st_det).det_forward(x))
    # the DB post-process does not care which network drew the map: device path == host path, box for box
    page_hw = tuple(pages_np.shape[1:3])
    dev = pipe.boxes_from_maps_device(maps, page_hw)
    host = pipe.boxes_from_maps(maps.cpu().numpy(), page_hw)
    assert len(dev) == len(host) == 2
    for a, b in zip(dev, host):
        assert a.shape == b.shape and np.array_equal(a, b)
    # recognition behind it: given quads, the strings are those of the same recogniser behind the v6 detector
    quads = [boxes_to_quads(np.asarray(b)[:8]) for b in boxes]
    res = pipe.run_batch(pages, quads)
    assert [len(r.lines) for r in res] == [8, 8]
    pipe6 = PagePipeline({"ppocrv6_det": st_v6, REC: st_rec}, n_rec_streams=2)
    assert pipe6.det_kind == "ppocrv6_det"
    res6 = pipe6.run_batch(pages, quads)
    assert [[t for _q, t, _s in r.lines] for r in res] == [[t for _q, t, _s in r.lines] for r in res6]
