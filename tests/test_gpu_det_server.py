"""GPU: the PP-OCRv5 server detector (`model_kind "ppocrv5_det_server"`: PPHGNetV2-B4 + LKPAN with IntraCL + PFHeadLocal) against the
fixtures minted from the reference's own modules (tests/golden/make_golden_det_server.py), its launch invariance, the direct 9x9
convolution (csrc/kernels_conv9x9_h1.hip) and the fused local tail (csrc/kernels_det_local.hip) alone against float64, the range guard, and the session / page pipeline on top of it.

Bounds: `maps` 1e-3 max-abs, the project's stated bound (tests/test_gpu_parity.py); the neck output 1e-3 * max(1, max |ref|), the form
tests/test_gpu_rec_lines.py uses; a kernel alone against float64 2e-5 (the project's bound for its direct convolutions).  Figures are
printed before they are asserted (run with -s to see them)."""
import ctypes as C

import numpy as np
import pytest
import torch

from kind_helpers import check_det_fixture, engine_cache, golden_x, synth_state, write_weights
from rapiddoc_amd import _lib

pytestmark = pytest.mark.gpu
TOL = 1e-3
KIND = "ppocrv5_det_server"
TAGS = ["b2_h64_w96", "b1_h160_w224", "b3_h96_w352", "b1_h960_w704"]


def _state(golden_dir, kind=KIND):
    return synth_state(golden_dir, kind)


_engine = engine_cache(KIND)


def _check_against_fixture(eng, golden_dir, tag, label):
    check_det_fixture(eng, golden_dir, tag, label, prefix="det5s", neck_channels=256, name="det server", tol=TOL)


@pytest.mark.parametrize("precision", ["auto", "fp32"])
@pytest.mark.parametrize("tag", TAGS)
def test_whole_network_matches_the_reference_fixtures(golden_dir, tag, precision):
    _check_against_fixture(_engine(golden_dir, precision), golden_dir, tag, precision)


def test_whole_network_in_h3_mode(golden_dir):
    _check_against_fixture(_engine(golden_dir, "h3"), golden_dir, "b2_h64_w96", "h3")


@pytest.mark.parametrize("precision", ["auto", "fp32"])
def test_an_image_does_not_depend_on_the_launch_it_rides_in(golden_dir, precision):
    eng = _engine(golden_dir, precision)
    g = np.load(golden_dir / "det5s_seed0_b3_h96_w352.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    m3, f3 = eng.det_forward(x, want_neck=True)
    m3, f3 = m3.clone(), f3.clone()
    m1, f1 = eng.det_forward(x[1:2].contiguous(), want_neck=True)
    assert torch.equal(m1[0], m3[1]) and torch.equal(f1[0], f3[1])


# ---------------------------------------------------------------------------------------------------------------- the 9x9 kernel alone
def _debug_conv9(x_nhwc, w_oihw, bias, act, res, route):
    """One 9x9 / pad 4 convolution through rd_debug_conv (api_debug.cpp): route 4 forces the direct kernel (kernels_conv9x9_h1.hip), 0 leaves the
    layer on the generic k x k split implicit GEMM.  Returns (y NHWC, the route the call reports)."""
    lib = _lib.load()
    N, H, W_, Cin = x_nhwc.shape
    Cout = w_oihw.shape[0]
    K = 81 * Cin
    wf = w_oihw.permute(0, 2, 3, 1).reshape(Cout, K).contiguous()          # k = (kh * 9 + kw) * Cin + ci
    hi = wf.half()
    lo = ((wf - hi.float()) * 2048.0).half()
    Kp = (K + 31) // 32 * 32
    wh = torch.zeros((Cout, Kp), dtype=torch.float16, device="cuda"); wh[:, :K] = hi
    wl = torch.zeros((Cout, Kp), dtype=torch.float16, device="cuda"); wl[:, :K] = lo
    y = torch.full((N, H, W_, Cout), float("nan"), device="cuda")
    used = C.c_int(route)
    lib.rd_debug_conv(N, H, W_, Cin, Cout, 9, 9, 1, 4, 4, 4, 4, act, 0, x_nhwc.data_ptr(), wf.data_ptr(), wh.data_ptr(), wl.data_ptr(),
                      bias.data_ptr() if bias is not None else None, res.data_ptr() if res is not None else None, y.data_ptr(), C.byref(used))
    torch.cuda.synchronize()
    return y, used.value


@pytest.mark.parametrize("N,H,W_,Cin,extras", [
    (2, 2, 3, 256, False),       # the 1/32 map of a 64 x 96 page: smaller than the halo on every side at once, 16 channel passes
    (1, 9, 35, 64, False),       # two row tiles, two column tiles, both ragged
    (2, 17, 33, 256, False),     # three row tiles, the last one a single row; one column past a tile
    (3, 12, 70, 64, True),       # bias + ReLU + residual; three column tiles
])
def test_direct_9x9_conv_matches_fp64(N, H, W_, Cin, extras):
    """kernels_conv9x9_h1.hip against torch conv2d in float64, operand ranges of test_direct_conv_matches_fp64 (tests/test_gpu_parity.py)."""
    import torch.nn.functional as F
    g = torch.Generator(device="cuda").manual_seed(N * 1000 + Cin)
    x = torch.rand((N, H, W_, Cin), device="cuda", generator=g) * 2 - 1
    w = (torch.rand((64, Cin, 9, 9), device="cuda", generator=g) - 0.5) * 0.2
    b = (torch.rand((64,), device="cuda", generator=g) - 0.5) if extras else None
    res = torch.rand((N, H, W_, 64), device="cuda", generator=g) if extras else None
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double() if extras else None, padding=4)
    if extras:
        ref = torch.relu(ref) + res.permute(0, 3, 1, 2).double()
    y, used = _debug_conv9(x, w, b, 1 if extras else 0, res, 4)
    assert used == 4, "the direct 9x9 kernel did not take this geometry"
    err = (y.permute(0, 3, 1, 2).double() - ref).abs().max().item()
    bound = 2e-5 * max(1.0, ref.abs().max().item())
    print(f"\n[direct 9x9 {N}x{H}x{W_} {Cin}->64{' +bias+relu+res' if extras else ''}] max |y - fp64| = {err:.3e} (bound {bound:.3e}, max |ref| {ref.abs().max().item():.1f})")
    assert err < bound


# ---------------------------------------------------------------------------------------------------------------- the fused tail alone
def _debug_det_local(f, shrink, w3, b3, w1, b1, split):
    lib = _lib.load()
    fn = lib.rd_debug_det_local
    N, H, W_ = shrink.shape
    y = torch.empty((N, H, W_), device="cuda")
    rng = C.c_int(0)
    ms = fn(N, H, W_, 1 if split else 0, 0, f.data_ptr(), shrink.data_ptr(), w3.data_ptr(), b3.data_ptr(), w1.data_ptr(), float(b1), y.data_ptr(),
            C.byref(rng))
    torch.cuda.synchronize()
    assert ms >= 0
    return y, rng.value


def _tail_case(shape, seed):
    """f NHWC (post-ReLU: >= 0), shrink in (0, 1) at twice the size, last_3 [64, 65, 3, 3] (channel 0 = shrink), last_1 scaled so that
    the float64 cbn logits span about +-4 around the bias."""
    import torch.nn.functional as F
    N, FH, FW, _ = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    f = torch.rand(shape, device="cuda", generator=g)
    shrink = torch.rand((N, 2 * FH, 2 * FW), device="cuda", generator=g) * 0.998 + 0.001
    w3 = (torch.rand((64, 65, 3, 3), device="cuda", generator=g) - 0.5) * 0.2
    b3 = torch.rand((64,), device="cuda", generator=g) - 0.5
    w1 = torch.rand((64,), device="cuda", generator=g) - 0.5
    cat = torch.cat([shrink[:, None].double(), F.interpolate(f.permute(0, 3, 1, 2).double(), scale_factor=2, mode="nearest")], dim=1)
    hidden = torch.relu(F.conv2d(cat, w3.double(), b3.double(), padding=1))
    lin = (hidden * w1.double()[None, :, None, None]).sum(dim=1)
    # (the hidden tensor is >= 0, so the raw sums are one-sided: scale and bias map their range onto [-4, 4])
    scale = 8.0 / float(lin.max() - lin.min())
    w1 = (w1 * scale).contiguous()
    b1 = float(np.float32(-4.0 - scale * float(lin.min())))
    logit = (hidden * w1.double()[None, :, None, None]).sum(dim=1) + b1
    ref = 0.5 * (shrink.double() + torch.sigmoid(logit))
    return f, shrink, w3, b3, w1, b1, ref, float(logit.min()), float(logit.max())


@pytest.mark.parametrize("split", [True, False], ids=["split", "fp32"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 64), (1, 17, 41, 64), (3, 8, 33, 64)])
def test_fused_local_tail_matches_fp64(shape, split):
    f, shrink, w3, b3, w1, b1, ref, lo, hi = _tail_case(shape, 100 + shape[1])
    y, rng = _debug_det_local(f, shrink, w3, b3, w1, b1, split)
    err = float((y.double() - ref).abs().max())
    print(f"\n[det local tail {shape} {'split' if split else 'fp32'}] logits {lo:.2f} .. {hi:.2f}; max |map - fp64| = {err:.3e} (bound 2e-05)")
    assert rng == 0
    assert lo < -2.0 and hi > 2.0
    assert err < 2e-5


def test_fused_local_tail_matches_the_unfused_arithmetic():
    """The same layers as separate fp32 operators (concat, 3x3, ReLU, 1x1, sigmoid, mean): the fused kernel may differ from them by its own
    distance to float64 (2e-5, above) plus theirs, which is measured here."""
    import torch.nn.functional as F
    f, shrink, w3, b3, w1, b1, ref, _lo, _hi = _tail_case((1, 17, 41, 64), 117)
    cat = torch.cat([shrink[:, None], F.interpolate(f.permute(0, 3, 1, 2), scale_factor=2, mode="nearest")], dim=1)
    old = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    try:
        hidden = torch.relu(F.conv2d(cat, w3, b3, padding=1))
        unf = 0.5 * (shrink + torch.sigmoid(F.conv2d(hidden, w1.view(1, 64, 1, 1)) + b1)[:, 0])
    finally:
        torch.backends.cudnn.allow_tf32 = old
    e_unf = float((unf.double() - ref).abs().max())
    for split in (True, False):
        y, _ = _debug_det_local(f, shrink, w3, b3, w1, b1, split)
        d = float((y - unf).abs().max())
        print(f"\n[det local tail vs unfused, {'split' if split else 'fp32'}] max |fused - unfused| = {d:.3e}; unfused vs fp64 {e_unf:.3e}")
        assert d < 2e-5 + e_unf


# ---------------------------------------------------------------------------------------------------------------- guard, session, pipeline
def test_range_guard_falls_back_to_the_fp32_mode_bit_for_bit(golden_dir, monkeypatch):
    from rapiddoc_amd.engine import RdEngine
    monkeypatch.setenv("RD_PRECISION", "auto")
    big = dict(_state(golden_dir))
    big["backbone.stem.stem1.conv.weight"] = big["backbone.stem.stem1.conv.weight"] * 3e5
    g = np.load(golden_dir / "det5s_seed0_b2_h64_w96.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    ref = RdEngine(KIND, guard="off").load_weights(big).set_precision("fp32").det_forward(x)
    raw = RdEngine(KIND, guard="off").load_weights(big)
    raw.det_forward(x)
    assert raw.range_overflow() and not raw.range_overflow()          # raised once, cleared by the read
    eng = RdEngine(KIND).load_weights(big)                            # default guard="sync": the forward itself falls back
    got = eng.det_forward(x)
    assert eng.precision == "fp32" and eng.range_fallbacks == 1
    assert torch.equal(got, ref)


def test_session_from_cfg_resolves_the_kind_by_stem(tmp_path, golden_dir):
    from rapiddoc_amd.session import Mi355DetSession
    p = write_weights(tmp_path, "ch_PP-OCRv5_det_server", _state(golden_dir))
    sess = Mi355DetSession.from_cfg({"model_path": str(p)})
    assert sess.kind == KIND and sess.engine.kind == KIND
    g = np.load(golden_dir / "det5s_seed0_b2_h64_w96.npz")
    y = sess(golden_x(g))
    ps = int(g["maps_ps"])
    assert type(y) is np.ndarray and y.shape == (2, 1, 64, 96) and y.dtype == np.float32
    e = float(np.abs(y[:, :, ::ps, ::ps] - g["maps"]).max())
    print(f"\n[det server session] max |maps - reference| = {e:.3e}")
    assert e <= TOL


def test_page_pipeline_with_the_server_detector(golden_dir):
    from rapiddoc_amd.engine import RdEngine
    from rapiddoc_amd.pages import synth_batch
    from rapiddoc_amd.pipeline import PagePipeline, boxes_to_quads
    st_det, st_v6, st_rec = _state(golden_dir), _state(golden_dir, "ppocrv6_det"), _state(golden_dir, "ppocrv6_rec")
    with pytest.raises(ValueError):
        PagePipeline({KIND: st_det, "ppocrv6_det": st_v6, "ppocrv6_rec": st_rec})
    with pytest.raises(ValueError):
        PagePipeline({"ppocrv6_rec": st_rec})
    pipe = PagePipeline({KIND: st_det, "ppocrv6_rec": st_rec}, n_rec_streams=2)
    assert pipe.det_kind == KIND and pipe.det.kind == KIND
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
    # recognition behind it: given quads, the strings are those of the v6-detector pipeline
    quads = [boxes_to_quads(np.asarray(b)[:8]) for b in boxes]
    res = pipe.run_batch(pages, quads)
    assert [len(r.lines) for r in res] == [8, 8]
    pipe6 = PagePipeline({"ppocrv6_det": st_v6, "ppocrv6_rec": st_rec}, n_rec_streams=2)
    assert pipe6.det_kind == "ppocrv6_det"
    res6 = pipe6.run_batch(pages, quads)
    assert [[t for _q, t, _s in r.lines] for r in res] == [[t for _q, t, _s in r.lines] for r in res6]
