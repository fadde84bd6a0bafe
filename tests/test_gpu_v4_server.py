"""GPU: the PP-OCRv4 server detector and recogniser (PPHGNet_small behind the two v5 server kinds: a state dict that carries
`backbone.stages.0.blocks.0.att.conv.weight` loads under "ppocrv5_det_server" / "ppocrv5_rec_server" with that backbone) against the
fixtures minted from the reference's own modules (tests/golden/make_golden_v4_server.py); launch invariance; the range guard; the new
kernels alone against float64 - the direct 3x3 convolution to 128 .. 224 channels (csrc/kernels_conv3x3_wide.hip), the ESE gate and the
3x3 / stride-2 max-pool (csrc/kernels_ese.hip); and the page pipeline on both v4 states.

Bounds: `maps`, tokens, neck, logits and probabilities 1e-3 max-abs, `fuse` 1e-3 * max(1, max |ref|) (tests/test_gpu_det_server.py,
tests/test_gpu_v5_server.py); a kernel alone against float64 2e-5 * max(1, max |ref|), the project's bound for its direct convolutions;
the gate itself 2e-5.  The fixtures' top-2 probability gaps are >= 1e-2 everywhere (asserted by the generator), so the indices are compared
at EVERY position.  Figures are printed before they are asserted (run with -s to see them)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kind_helpers import check_det_fixture, engine_cache, golden_x, synth_state
from rapiddoc_amd import _lib
from rapiddoc_amd import ocr_host
from rapiddoc_amd import weights as W

pytestmark = pytest.mark.gpu
TOL = 1e-3
DET, REC = "ppocrv5_det_server", "ppocrv5_rec_server"
DET_TAGS = ["b2_h64_w96", "b1_h160_w224", "b3_h96_w352"]
REC_TAGS = ["b2_w64", "b3_w104", "b2_w100", "b3_w320"]


def _det_state(golden_dir):
    return synth_state(golden_dir, "ppocrv4_det_server", kind="ppocrv4_server")


def _rec_state(golden_dir):
    return synth_state(golden_dir, "ppocrv4_rec_server", kind="ppocrv4_server")


_det = engine_cache(DET, state=_det_state)
_rec = engine_cache(REC, guard="sync", state=_rec_state)


# ---------------------------------------------------------------------------------------------------------------- whole networks
def test_fixtures_were_minted_with_todays_generator(golden_dir):
    s = json.loads((golden_dir / "summary_v4_server.json").read_text())
    for key, st in (("det", _det_state(golden_dir)), ("rec", _rec_state(golden_dir))):
        assert abs(W.checksum(st) - s[key]["checksum"]) < 1e-6 * max(1.0, abs(s[key]["checksum"]))


@pytest.mark.parametrize("precision", ["auto", "fp32"])
@pytest.mark.parametrize("tag", DET_TAGS)
def test_detector_matches_the_reference_fixtures(golden_dir, tag, precision):
    eng = _det(golden_dir, precision)
    assert eng.kind == DET and eng.backbone == "pphgnet_small"
    check_det_fixture(eng, golden_dir, tag, precision, prefix="det4s", neck_channels=256, name="v4 det server", tol=TOL)


def test_the_v5_weights_still_pick_pphgnetv2(golden_dir):
    from rapiddoc_amd.engine import RdEngine
    assert RdEngine(DET).load_weights(synth_state(golden_dir, DET)).backbone == "pphgnetv2_b4"
    assert RdEngine(REC).load_weights(synth_state(golden_dir, REC)).backbone == "pphgnetv2_b4"
    assert RdEngine("ppocrv6_det").load_weights(synth_state(golden_dir, "ppocrv6_det")).backbone == ""


@pytest.mark.parametrize("precision", ["auto", "fp32"])
@pytest.mark.parametrize("tag", REC_TAGS)
def test_recogniser_matches_the_reference_fixtures(golden_dir, tag, precision):
    from rapiddoc_amd.engine import REC_WANT_LOGITS, REC_WANT_NECK, REC_WANT_SOFTMAX
    eng = _rec(golden_dir, precision)
    assert eng.kind == REC and eng.backbone == "pphgnet_small" and eng.num_classes == 6625
    g = np.load(golden_dir / f"rec4s_seed0_{tag}.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    cs = int(g["backbone_cs"])
    tok = eng.rec_backbone_forward(x).cpu().numpy()                                   # [B, T, 1024]
    ref_tok = g["backbone"][:, :, 0, :].transpose(0, 2, 1)
    assert tok.shape[2] == eng.rec_token_dim == 1024 and tok.shape[:2] == ref_tok.shape[:2]
    assert tok.shape[1] == ocr_host.rec_seq_len(x.shape[3])
    e_tok = float(np.abs(tok[:, :, ::cs] - ref_tok).max())
    idx, prob, neck = eng.rec_forward(x, REC_WANT_NECK)
    idx, prob = idx.cpu().numpy(), prob.cpu().numpy()
    e_neck = float(np.abs(neck.cpu().numpy() - g["neck"]).max())
    _, _, lg = eng.rec_forward(x, REC_WANT_LOGITS)
    lg = lg.cpu().numpy()
    e_lg = max(float(np.abs(lg[:, :, ::61] - g["logits_sub"]).max()), float(np.abs(lg[:, 0, :] - g["logits_t0"]).max()))
    i_sm, _, sm = eng.rec_forward(x, REC_WANT_SOFTMAX)
    sm = sm.cpu().numpy()
    ref_sm = torch.softmax(torch.from_numpy(g["logits_t0"]), dim=1).numpy()
    e_sm = max(float(np.abs(sm[:, 0, :] - ref_sm).max()), float(np.abs(sm.max(axis=2) - g["prob"]).max()))
    e_prob = float(np.abs(prob - g["prob"]).max())
    print(f"\n[v4 rec server {tag} {precision}] max-abs errors: tokens {e_tok:.3e} neck {e_neck:.3e} logits {e_lg:.3e} softmax {e_sm:.3e} "
          f"prob {e_prob:.3e}; smallest top-2 gap {float(g['top2gap'].min()):.3e}; idx mismatches {int((idx != g['idx']).sum())}")
    assert not eng.range_overflow()
    assert e_tok < TOL and e_neck < TOL and e_lg < TOL and e_sm < TOL and e_prob < TOL
    assert float(g["top2gap"].min()) >= 1e-2
    assert np.array_equal(idx, g["idx"]) and np.array_equal(i_sm.cpu().numpy(), g["idx"])


def _lines(widths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand((n, 3, 48, w), generator=g) * 2 - 1).cuda() for n, w in widths]


@pytest.mark.parametrize("precision", ["auto", "fp32"])
def test_two_stages_equal_the_whole_network(golden_dir, precision):
    """Backbone stage per launch into one token buffer + ONE ragged tail over lines of three widths == rd_rec_forward launch by launch:
    indices and probabilities bit for bit, hence the strings."""
    eng = _rec(golden_dir, precision)
    launches = _lines([(2, 100), (3, 64), (1, 320)], seed=21)
    lens, whole = [], []
    for x in launches:
        i, p, _ = eng.rec_forward(x)
        whole.append((i.clone(), p.clone()))
        lens += [ocr_host.rec_seq_len(x.shape[3])] * x.shape[0]
    tokens = torch.zeros((sum(lens), eng.rec_token_dim), device="cuda")
    pos = 0
    for x in launches:
        n = x.shape[0] * ocr_host.rec_seq_len(x.shape[3])
        eng.rec_backbone_forward(x, tokens[pos: pos + n])
        pos += n
    idx, prob = eng.rec_tail_forward(tokens, lens)
    pos = 0
    for x, (i, p) in zip(launches, whole):
        n = i.numel()
        assert torch.equal(idx[pos: pos + n], i.reshape(-1)), (precision, x.shape)
        assert torch.equal(prob[pos: pos + n], p.reshape(-1)), (precision, x.shape)
        pos += n
    assert not eng.range_overflow()


def test_per_line_widths_stay_refused_for_the_server_kind(golden_dir):
    from rapiddoc_amd.engine import EngineError, rec_line_table
    eng = _rec(golden_dir, "auto")
    x = torch.zeros((2, 3, 48, 64), device="cuda")
    tab = torch.from_numpy(rec_line_table([64, 48], [0, 8])).cuda()
    with pytest.raises(EngineError, match="out of scope for ppocrv5_rec_server"):
        eng.rec_backbone_forward_lines(x, tab, torch.zeros((14, eng.rec_token_dim), device="cuda"))


@pytest.mark.parametrize("precision", ["auto", "fp32"])
def test_an_image_does_not_depend_on_the_launch_it_rides_in(golden_dir, precision):
    eng = _det(golden_dir, precision)
    g = np.load(golden_dir / "det4s_seed0_b3_h96_w352.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    m3, f3 = eng.det_forward(x, want_neck=True)
    m3, f3 = m3.clone(), f3.clone()
    m1, f1 = eng.det_forward(x[1:2].contiguous(), want_neck=True)
    assert torch.equal(m1[0], m3[1]) and torch.equal(f1[0], f3[1])
    rec = _rec(golden_dir, precision)
    xr = torch.from_numpy(golden_x(np.load(golden_dir / "rec4s_seed0_b3_w104.npz"))).cuda()
    t3 = rec.rec_backbone_forward(xr).clone()
    t1 = rec.rec_backbone_forward(xr[1:2].contiguous())
    assert torch.equal(t1[0], t3[1])


def test_range_guard_falls_back_to_the_fp32_mode_bit_for_bit(golden_dir, monkeypatch):
    from rapiddoc_amd.engine import RdEngine
    monkeypatch.setenv("RD_PRECISION", "auto")
    big = dict(_det_state(golden_dir))
    big["backbone.stem.0.conv.weight"] = big["backbone.stem.0.conv.weight"] * 3e5
    g = np.load(golden_dir / "det4s_seed0_b2_h64_w96.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    ref = RdEngine(DET, guard="off").load_weights(big).set_precision("fp32").det_forward(x)
    raw = RdEngine(DET, guard="off").load_weights(big)
    raw.det_forward(x)
    assert raw.range_overflow() and not raw.range_overflow()          # raised once, cleared by the read
    eng = RdEngine(DET).load_weights(big)                             # default guard="sync": the forward itself falls back
    got = eng.det_forward(x)
    assert eng.precision == "fp32" and eng.range_fallbacks == 1
    assert torch.equal(got, ref)


def test_op_lists_take_the_routes_the_builder_asked_for(golden_dir):
    """auto: 64 -> 128, 128 -> 128 and 768 -> 192 run on conv3x3_wide_h1 ("c3w/h3"), the other 160- and 192-channel layers as two pieces
    on conv3x3_h1, the 224-channel layers on the generic split route, every aggregation on the one-accumulator GEMM; fp32: no split
    route anywhere; the v5 weights under the same kind: no "c3w" and no piece anywhere (the opt-in is the PPHGNet_small builder's)."""
    from rapiddoc_amd.engine import RdEngine
    x = torch.zeros((1, 3, 64, 96), device="cuda")

    def ops(eng):
        eng.set_profiling(True)
        eng.profile_log.clear()
        eng.det_forward(x)
        eng.set_profiling(False)
        return list(eng.profile_log)

    auto = ops(_det(golden_dir, "auto"))
    c3 = [o for o in auto if o["kind"] == "conv3x3" and (".layers." in o["name"] or "stem.2." in o["name"])]
    wide = [o["name"] for o in c3 if o["cfg"] == "c3w/h3"]
    assert wide == ["backbone.stem.2.conv.weight"] + [f"backbone.stages.0.blocks.0.layers.{i}.conv.weight" for i in range(6)] + \
        ["backbone.stages.2.blocks.1.layers.0.conv.weight"]
    pieces = [o for o in c3 if "@" in o["name"]]
    assert len(pieces) == 2 * (6 + 6 + 5) and all(o["cfg"] == "c3h1/h3" for o in pieces)
    assert sorted({o["name"].split("@")[1] for o in pieces}) == ["0+96", "96+64", "96+96"]
    s4 = [o for o in c3 if ".stages.3." in o["name"]]
    assert len(s4) == 6 and all(o["cfg"].endswith("/h3") and not o["cfg"].startswith("c3") for o in s4) and len(c3) == 8 + 34 + 6
    agg = [o for o in auto if "aggregation_conv" in o["name"]]
    assert len(agg) == 5 and all(o["cfg"] == "h1w256x128/h3" for o in agg), [(o["name"], o["cfg"]) for o in agg]
    assert sum(o["kind"] == "ese_gate" for o in auto) == 5 and sum(o["name"] == "maxpool3x3s2" for o in auto) == 1
    fp32 = ops(_det(golden_dir, "fp32"))
    assert not any(o["cfg"].endswith("/h3") for o in fp32 if o["kind"].startswith("conv"))
    v5 = ops(RdEngine(DET).load_weights(synth_state(golden_dir, DET)))
    assert not any(o["cfg"].startswith("c3w") or "@" in o["name"] for o in v5)


# ---------------------------------------------------------------------------------------------------------------- conv3x3_wide_h1 alone
def _debug_wide(x_view, w_oihw, bias, act, y_view, route=0):
    """One launch through rd_debug_conv3x3_wide on views of wider buffers.  Returns (ms, the route's name, the range flag)."""
    lib = _lib.load()
    N, H, W_, Cin = x_view.shape
    Cout = w_oihw.shape[0]
    wf = w_oihw.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous()               # k = (kh * 3 + kw) * Cin + ci
    name = C.create_string_buffer(32)
    rng = C.c_int(-1)
    ms = lib.rd_debug_conv3x3_wide(route, N, H, W_, Cin, Cout, act, x_view.stride(2), y_view.stride(2), 0, x_view.data_ptr(), wf.data_ptr(),
                                   bias.data_ptr() if bias is not None else None, y_view.data_ptr(), name, 32, C.byref(rng))
    torch.cuda.synchronize()
    return ms, name.value.decode(), rng.value


def _wide_case(N, H, W_, Cin, Cout, extras, seed, xs=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    xbuf = torch.full((N, H, W_, Cin + 32), float("nan"), device="cuda")
    xbuf[..., :Cin] = (torch.rand((N, H, W_, Cin), device="cuda", generator=g) * 2 - 1) * xs
    w = (torch.rand((Cout, Cin, 3, 3), device="cuda", generator=g) - 0.5) * 0.2
    b = (torch.rand((Cout,), device="cuda", generator=g) - 0.5) if extras else None
    ybuf = torch.full((N, H, W_, Cout + 64), float("nan"), device="cuda")
    return xbuf, xbuf[..., :Cin], w, b, ybuf, ybuf[..., :Cout]


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "bias_relu"])
@pytest.mark.parametrize("Cin,Cout", [(64, 128), (128, 128), (256, 160), (160, 160), (512, 192), (768, 224)])
@pytest.mark.parametrize("H,W_", [(9, 33), (8, 32)])
def test_conv3x3_wide_matches_fp64(H, W_, Cin, Cout, extras):
    """N = 2; 9 x 33 is one past each edge of the 8 x 32 tile, 8 x 32 exact; xld = Cin + 32 and yld = Cout + 64 with the gaps NaN before
    and untouched after (a NaN read from the input gap would poison the output; a write into the output gap would clear its NaN)."""
    xbuf, x, w, b, ybuf, y = _wide_case(2, H, W_, Cin, Cout, extras, 1000 * H + Cin + Cout)
    ms, name, rng = _debug_wide(x, w, b, 1 if extras else 0, y)
    assert ms >= 0 and name == "c3w", (ms, name)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double() if extras else None, padding=1)
    ref = (torch.relu(ref) if extras else ref).permute(0, 2, 3, 1)
    assert not bool(torch.isnan(y).any()), "an output element was not written (or a gap of the input was read)"
    assert bool(torch.isnan(ybuf[..., Cout:]).all()) and bool(torch.isnan(xbuf[..., Cin:]).all()), "a gap was written"
    err = float((y.double() - ref).abs().max())
    bound = 2e-5 * max(1.0, float(ref.abs().max()))
    print(f"\n[conv3x3_wide 2x{H}x{W_} {Cin}->{Cout}{' +bias+relu' if extras else ''}] max |y - fp64| = {err:.3e} (bound {bound:.3e}, "
          f"max |ref| {float(ref.abs().max()):.2f})")
    assert rng == 0
    assert err < bound


def test_conv3x3_wide_tail_pass_and_256_channels():
    """Cin = 112 = three passes of 32 + the 16-channel tail pass; Cout = 256 = eight output blocks, the widest the kernel takes."""
    _, x, w, b, ybuf, y = _wide_case(2, 9, 33, 112, 256, True, 8)
    ms, name, rng = _debug_wide(x, w, b, 1, y)
    assert ms >= 0 and name == "c3w" and rng == 0
    ref = torch.relu(F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1)).permute(0, 2, 3, 1)
    assert bool(torch.isnan(ybuf[..., 256:]).all())
    assert float((y.double() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max()))


def test_conv3x3_wide_raises_the_range_flag():
    _, x, w, b, _, y = _wide_case(2, 9, 33, 128, 128, True, 5, xs=1e5)
    ms, name, rng = _debug_wide(x, w, b, 1, y)
    assert ms >= 0 and name == "c3w" and rng == 1
    _, x, w, b, _, y = _wide_case(2, 9, 33, 128, 128, True, 5)
    assert _debug_wide(x, w, b, 1, y)[2] == 0


def test_conv3x3_wide_rows_do_not_depend_on_the_number_of_images():
    """More tiles than workgroups of the persistent grid (600 images x 2 tiles), against one image alone: bit for bit."""
    _, x, w, b, _, y = _wide_case(600, 9, 33, 64, 128, True, 6)
    _, x1, _, _, _, y1 = _wide_case(1, 9, 33, 64, 128, True, 6)
    x1.copy_(x[7:8])
    assert _debug_wide(x, w, b, 1, y)[1] == "c3w" and _debug_wide(x1, w, b, 1, y1)[1] == "c3w"
    assert torch.equal(y1[0], y[7])
    ref = torch.relu(F.conv2d(x[-1:].permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1)).permute(0, 2, 3, 1)
    assert float((y[-1:].double() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max()))


def test_the_other_two_routes_of_the_entry_compute_the_same_layer():
    """Routes 1 (generic split implicit GEMM) and 2 (conv3x3_h1 over <= 96-channel pieces), which tools/mb_v4_server.py times against the
    new kernel: the same layer within the same bound."""
    _, x, w, b, _, y = _wide_case(2, 9, 33, 256, 160, True, 7)
    ref = torch.relu(F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1)).permute(0, 2, 3, 1)
    for route, want in ((1, None), (2, "c3h1")):
        y.fill_(float("nan"))
        ms, name, _ = _debug_wide(x, w, b, 1, y, route)
        assert ms >= 0 and name != "c3w" and (want is None or name == want), (route, ms, name)
        assert float((y.double() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max()))


# ---------------------------------------------------------------------------------------------------------------- ESE gate, max-pool
def _debug_ese(x_view, w, b, idn, y_view):
    lib = _lib.load()
    N, H, W_, Cn = x_view.shape
    chunks = C.c_int(0)
    assert lib.rd_debug_ese(N, H, W_, Cn, x_view.stride(2), idn.stride(2) if idn is not None else 0, y_view.stride(2), x_view.data_ptr(), w.data_ptr(),
                            b.data_ptr(), None, None, x_view.data_ptr(), y_view.data_ptr(), C.byref(chunks)) == 0          # the size query
    partial = torch.full((N * chunks.value * Cn,), float("nan"), device="cuda")
    s = torch.full((N, Cn), float("nan"), device="cuda")
    assert lib.rd_debug_ese(N, H, W_, Cn, x_view.stride(2), idn.stride(2) if idn is not None else 0, y_view.stride(2), x_view.data_ptr(), w.data_ptr(),
                            b.data_ptr(), idn.data_ptr() if idn is not None else None, partial.data_ptr(), s.data_ptr(), y_view.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return s, chunks.value


def _ese_case(N, H, W_, Cn, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    xbuf = torch.full((N, H, W_, Cn + 8), float("nan"), device="cuda")
    xbuf[..., :Cn] = torch.rand((N, H, W_, Cn), device="cuda", generator=g)                  # post-ReLU: >= 0
    x = xbuf[..., :Cn]
    w = (torch.rand((Cn, Cn), device="cuda", generator=g) - 0.5)
    b = torch.rand((Cn,), device="cuda", generator=g) - 0.5
    mean = x.double().mean(dim=(1, 2))
    lin = mean @ w.double().t()
    scale = 9.0 / float(lin.max() - lin.min())             # the logits span 9 around their middle: at least -4 .. 4
    w = (w * scale).contiguous()
    b = (b - float(scale * (lin.max() + lin.min()) / 2)).contiguous()
    idn = torch.rand((N, H, W_, Cn), device="cuda", generator=g)
    return xbuf, x, w, b, idn


@pytest.mark.parametrize("identity", [False, True], ids=["plain", "identity"])
@pytest.mark.parametrize("H,W_", [(1, 1), (7, 5), (24, 22)])            # 24 x 22 = 528 pixels: two partial chunks of launch_gap_partial
@pytest.mark.parametrize("Cn", [256, 1024])
def test_ese_gate_matches_fp64(Cn, H, W_, identity):
    N = 3
    xbuf, x, w, b, idn = _ese_case(N, H, W_, Cn, 100 * H + Cn)
    ybuf = torch.full((N, H, W_, Cn + 12), float("nan"), device="cuda")
    y = ybuf[..., :Cn]
    s, chunks = _debug_ese(x, w, b, idn if identity else None, y)
    logit = x.double().mean(dim=(1, 2)) @ w.double().t() + b.double()
    s_ref = torch.sigmoid(logit)
    ref = x.double() * s_ref[:, None, None, :] + (idn.double() if identity else 0.0)
    e_s, e_y = float((s.double() - s_ref).abs().max()), float((y.double() - ref).abs().max())
    bound = 2e-5 * max(1.0, float(ref.abs().max()))
    print(f"\n[ese C {Cn} {H}x{W_}{' +identity' if identity else ''}] chunks {chunks}; logits {float(logit.min()):.2f} .. {float(logit.max()):.2f}; "
          f"max |s - fp64| = {e_s:.3e} (bound 2e-05), max |y - fp64| = {e_y:.3e} (bound {bound:.3e})")
    assert chunks == (2 if H * W_ >= 512 else 1)
    assert float(logit.min()) <= -4.0 and float(logit.max()) >= 4.0
    assert bool(torch.isnan(ybuf[..., Cn:]).all()) and not bool(torch.isnan(y).any())
    assert e_s < 2e-5 and e_y < bound
    # row 1 of the batch of three == that image alone, bit for bit; and in place (y = x)
    y1 = torch.full((1, H, W_, Cn), float("nan"), device="cuda")
    s1, _ = _debug_ese(x[1:2], w, b, idn[1:2] if identity else None, y1)
    assert torch.equal(s1[0], s[1]) and torch.equal(y1[0], y[1])
    _debug_ese(x, w, b, idn if identity else None, x)
    assert torch.equal(x, y)


def test_ese_gate_refuses_a_width_it_does_not_serve():
    lib = _lib.load()
    t = torch.zeros((4096,), device="cuda")
    for cn in (1028, 6):
        assert lib.rd_debug_ese(1, 1, 1, cn, cn, 0, cn, t.data_ptr(), t.data_ptr(), t.data_ptr(), None, t.data_ptr(), t.data_ptr(), t.data_ptr(), None) == -1


@pytest.mark.parametrize("N,H,W_,Cn", [(2, 7, 9, 8), (1, 8, 10, 128), (3, 1, 1, 4), (2, 5, 4, 12), (1, 32, 48, 128)])
def test_maxpool3x3s2_equals_torch(N, H, W_, Cn):
    g = torch.Generator(device="cuda").manual_seed(N + H + W_)
    xbuf = torch.full((N, H, W_, Cn + 4), float("nan"), device="cuda")
    xbuf[..., :Cn] = torch.rand((N, H, W_, Cn), device="cuda", generator=g) * 2 - 3          # all negative somewhere: a zero padding would show
    x = xbuf[..., :Cn]
    OH, OW = (H - 1) // 2 + 1, (W_ - 1) // 2 + 1
    ybuf = torch.full((N, OH, OW, Cn + 8), float("nan"), device="cuda")
    y = ybuf[..., :Cn]
    assert _lib.load().rd_debug_maxpool3x3s2(N, H, W_, Cn, x.stride(2), y.stride(2), x.data_ptr(), y.data_ptr()) == 0
    torch.cuda.synchronize()
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), 3, stride=2, padding=1).permute(0, 2, 3, 1)
    assert ref.shape == y.shape and torch.equal(y, ref) and bool(torch.isnan(ybuf[..., Cn:]).all())


# ---------------------------------------------------------------------------------------------------------------- the page pipeline
def test_page_pipeline_with_both_v4_server_states(golden_dir):
    """PagePipeline on the two v4 states under the two server kinds with a 6623-entry dictionary (+ blank and space = 6625 classes), on 2
    synthetic pages (rendered det maps, as tests/test_gpu_v5_server.py): strict-mode strings == rd_rec_forward chunk by chunk in the
    reference's loop (rapid_ocr.py:404-449) on the crops the pipeline made; the detector of the same pipeline runs the v4 backbone."""
    from rapiddoc_amd.engine import RdEngine
    from rapiddoc_amd.pages import synth_batch
    from rapiddoc_amd.pipeline import PagePipeline, render_text_maps
    chars = ["blank"] + [chr(0x4E00 + i) for i in range(6623)] + [" "]
    st_det, st_rec = _det_state(golden_dir), _rec_state(golden_dir)
    pipe = PagePipeline({DET: st_det, REC: st_rec}, characters=chars, n_rec_streams=2)
    assert pipe.det_kind == DET and pipe.rec_kind == REC and pipe.rec_mode == "strict"
    assert pipe.det.backbone == "pphgnet_small" and pipe.rec.backbone == "pphgnet_small" and pipe.rec.num_classes == 6625
    pages_np, boxes = synth_batch(11, 2)
    pages = torch.from_numpy(pages_np).cuda()
    dmaps, det_hw = pipe.det_forward(pages)
    dmaps = dmaps.clone()
    assert not pipe.det.check_range_and_fallback()
    x = pipe.det_preprocess(pages)[0]
    assert dmaps.shape == (2, 1, *det_hw) and torch.equal(dmaps, RdEngine(DET).load_weights(st_det).det_forward(x))
    maps = render_text_maps(boxes, pages_np.shape[1:3], pipe.det_preprocess(pages[:1])[1], pages.device)
    pipe.keep_rec_inputs = True
    res = pipe.run_batch(pages, None, det_maps_override=maps)
    flat = [ln for r in res for ln in r.lines]
    n = len(flat)
    assert n >= 60
    line_x = {}
    for chunk, xb, _lw, _i, _p in pipe.last_rec_batches:
        for j, i in enumerate(chunk.tolist()):
            line_x[int(i)] = xb[j]
    cw, ch, rot, _keep = pipe.last_rec_crop_sizes
    ratios = np.array([(int(cw[i]) / float(ch[i])) if not rot[i] else (int(ch[i]) / float(cw[i])) for i in range(n)])
    indices = np.argsort(ratios)
    eng = RdEngine(REC).load_weights(st_rec)
    out = [None] * n
    for beg in range(0, n, 6):
        idxs = [int(i) for i in indices[beg: beg + 6]]
        batch = torch.stack([line_x[i] for i in idxs]).contiguous()
        idx, prob, _ = eng.rec_forward(batch)
        for r, (t, sc) in enumerate(ocr_host.ctc_decode(idx.cpu().numpy(), prob.cpu().numpy(), pipe.characters)):
            out[idxs[r]] = (t, sc)
    assert any(t for t, _s in out), "every line decoded to the empty string: the comparison would say nothing"
    assert [t for t, _s in out] == [t for _q, t, _s in flat]
    assert max(abs(ocr_host.format_score(sc) - fs) for (_t, sc), (_q, _t2, fs) in zip(out, flat)) <= 1e-3 + 1e-9
