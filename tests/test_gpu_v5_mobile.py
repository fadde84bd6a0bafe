"""GPU: the PP-OCRv5 mobile recogniser (`model_kind "ppocrv5_rec_mobile"`: PPLCNetV3 scale 0.95 + SVTR neck + CTC) against the fixtures minted
from the reference's own modules (tests/golden/make_golden_v5_mobile.py), per-line widths inside one backbone launch against the same
lines launched alone, its stages against each other, the range guard, and the session / page pipeline on top of it.

Bound of the numeric comparisons against the fixtures: 1e-3 * max(1, max |reference|), the rule tests/test_gpu_det_server.py uses for the
neck output.  Everything that compares the engine with itself is bit for bit.  Figures are printed before they are asserted (-s)."""
import numpy as np
import pytest
import torch

from kind_helpers import bound, engine_cache, golden_x, hswish64, line_launch, rand_lines, synth_state, write_weights
from rapiddoc_amd import _lib
from rapiddoc_amd import ocr_host

pytestmark = pytest.mark.gpu
TOL = 1e-3
KIND = "ppocrv5_rec_mobile"
TAGS = ["b2_w320", "b1_w96", "b3_w640", "b6_w1088"]


def _state(golden_dir, kind=KIND):
    return synth_state(golden_dir, kind)


_engine = engine_cache(KIND)
_server_engine = engine_cache("ppocrv5_rec_server")


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("precision", ["auto", "fp32"])
@pytest.mark.parametrize("tag", TAGS)
def test_whole_network_matches_the_reference_fixtures(golden_dir, tag, precision):
    from rapiddoc_amd.engine import REC_WANT_NECK
    eng = _engine(golden_dir, precision)
    g = np.load(golden_dir / f"rec5m_seed0_{tag}.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    cs = int(g["backbone_cs"])
    tok = eng.rec_backbone_forward(x).cpu().numpy()                                   # [B, T, 480]
    ref_tok = g["backbone"][:, :, 0, :].transpose(0, 2, 1)                            # [B, 480 / cs, 1, T] -> [B, T, 480 / cs]
    assert tok.shape[2] == eng.rec_token_dim == 480 and tok.shape[:2] == ref_tok.shape[:2]
    e_tok = float(np.abs(tok[:, :, ::cs] - ref_tok).max())
    idx, prob, neck = eng.rec_forward(x, REC_WANT_NECK)
    idx, prob = idx.cpu().numpy(), prob.cpu().numpy()
    e_neck = float(np.abs(neck.cpu().numpy() - g["neck"]).max())
    e_prob = float(np.abs(prob - g["prob"]).max())
    safe = g["top2gap"] > 1e-2
    masked = float(1.0 - safe.mean())
    print(f"\n[v5 mobile {tag} {precision}] max-abs errors: tokens {e_tok:.3e} (bound {bound(ref_tok, TOL):.3e}) neck {e_neck:.3e} "
          f"(bound {bound(g['neck'], TOL):.3e}) prob {e_prob:.3e}; masked share {masked:.4f}; "
          f"idx mismatches at safe positions {int((idx != g['idx'])[safe].sum())}")
    assert not eng.range_overflow()
    assert e_tok < bound(ref_tok, TOL) and e_neck < bound(g["neck"], TOL) and e_prob < TOL
    assert masked <= 0.01
    assert (idx == g["idx"])[safe].all()


# ---------------------------------------------------------------------------------------------------------------- 2. per-line widths
LINE_W = [96, 322, 330, 200, 640]            # w2 / w4 odd for some (161 / 81, 165 / 83), one line far narrower than the launch


@pytest.mark.parametrize("precision", ["auto", "fp32"])
def test_lines_of_different_widths_in_one_launch_equal_each_line_alone(golden_dir, precision):
    eng = _engine(golden_dir, precision)
    g = np.load(golden_dir / "rec5m_width_pair.npz")
    lines = rand_lines(LINE_W, seed=31)
    lines[3] = torch.from_numpy(g["x200"]).cuda()                                     # the 200-px line of the width-pair fixture
    alone = [eng.rec_backbone_forward(ln)[0].clone() for ln in lines]
    x, tab, T, first = line_launch(lines, 640)
    tokens = torch.full((sum(T) + 3, eng.rec_token_dim), 7.0, device="cuda")
    eng.rec_backbone_forward_lines(x, tab, tokens)
    assert float((tokens[sum(T):] - 7.0).abs().max()) == 0.0                          # nothing past the last line's tokens
    for i, (a, t, f) in enumerate(zip(alone, T, first)):
        assert torch.equal(tokens[f: f + t], a), (precision, LINE_W[i], float((tokens[f: f + t] - a).abs().max()))
    # line 0 among other neighbours of other widths
    others = [lines[0]] + rand_lines([640, 100, 402], seed=32)
    x2, tab2, T2, _f2 = line_launch(others, 640)
    tokens2 = torch.zeros((sum(T2), eng.rec_token_dim), device="cuda")
    eng.rec_backbone_forward_lines(x2, tab2, tokens2)
    assert torch.equal(tokens2[: T2[0]], alone[0])
    # against the reference: the 200-px line at its own width and at table width 320
    ref200 = g["backbone200"][0, :, 0, :].T
    e200 = float(np.abs(tokens[first[3]: first[3] + T[3]].cpu().numpy() - ref200).max())
    x3, tab3, T3, _f3 = line_launch([torch.nn.functional.pad(lines[3], (0, 120))] + [lines[4]], 640)
    assert T3[0] == 40
    tokens3 = torch.zeros((sum(T3), eng.rec_token_dim), device="cuda")
    eng.rec_backbone_forward_lines(x3, tab3, tokens3)
    ref320 = g["backbone320"][0, :, 0, :].T
    e320 = float(np.abs(tokens3[:40].cpu().numpy() - ref320).max())
    print(f"\n[v5 mobile lines {precision}] 200-px line in a 640 launch: at width 200 {e200:.3e} (bound {bound(ref200, TOL):.3e}), at table width 320 "
          f"{e320:.3e} (bound {bound(ref320, TOL):.3e})")
    assert e200 < bound(ref200, TOL) and e320 < bound(ref320, TOL)
    assert not eng.range_overflow()


# ---------------------------------------------------------------------------------------------------------------- 3. launch invariance
@pytest.mark.parametrize("precision", ["auto", "fp32"])
def test_a_line_does_not_depend_on_the_launch_it_rides_in(golden_dir, precision):
    eng = _engine(golden_dir, precision)
    g = torch.Generator().manual_seed(22)
    x = (torch.rand((50, 3, 48, 328), generator=g) * 2 - 1).cuda()
    tok = eng.rec_backbone_forward(x).clone()
    idx, prob, _ = eng.rec_forward(x)
    idx, prob = idx.clone(), prob.clone()
    for b in (0, 17, 49):
        one = x[b: b + 1].contiguous()
        assert torch.equal(eng.rec_backbone_forward(one)[0], tok[b]), (precision, b)
        i1, p1, _ = eng.rec_forward(one)
        assert torch.equal(i1[0], idx[b]) and torch.equal(p1[0], prob[b]), (precision, b, float((p1[0] - prob[b]).abs().max()))
    assert not eng.range_overflow()


@pytest.mark.parametrize("precision", ["auto", "fp32"])
def test_two_stages_equal_the_whole_network_bit_for_bit(golden_dir, precision):
    """Backbone stage per launch into one token buffer + ONE ragged tail over lines of three widths == rd_rec_forward launch by launch."""
    eng = _engine(golden_dir, precision)
    g = torch.Generator().manual_seed(21)
    launches = [(torch.rand((n, 3, 48, w), generator=g) * 2 - 1).cuda() for n, w in [(2, 320), (3, 96), (1, 640)]]
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
        assert torch.equal(prob[pos: pos + n], p.reshape(-1)), (precision, x.shape, float((prob[pos: pos + n] - p.reshape(-1)).abs().max()))
        pos += n
    assert not eng.range_overflow()


# ---------------------------------------------------------------------------------------------------------------- 4. the depthwise kernel alone
@pytest.mark.parametrize("k,sh,sw", [(3, 1, 1), (3, 2, 1), (3, 1, 2), (5, 1, 1), (5, 2, 1)])
@pytest.mark.parametrize("pre_act", [0, 1])
@pytest.mark.parametrize("Cn", [32, 240])
def test_depthwise_layer_alone_matches_float64(k, sh, sw, pre_act, Cn):
    """`lcv3_dw_kernel` (csrc/kernels_lcv3.hip) through rd_debug_lcv3_dw against a float64 restatement: N = 3, H = 24, W = 37 (no multiple
    of the 4 columns a thread computes), C = 32 and the network's C = 240 (60 channel quads: a workgroup straddles pixels, and 17 threads share
    a quad in the row sums), line widths [37, 1, 20], inputs spanning +-4 so that all three branches of the hardswish are
    taken on load and in the epilogue.  Compared inside each line's output width; beyond it the kernel writes zeros.  Bound
    2e-5 * max(1, max |ref|): at most 25 fp32 multiply-adds of O(1) terms, two hardswishes and two affines per output - a few 2^-24
    relative roundings of values up to max |ref| - as the bound of the 9x9 and local-tail kernels' tests."""
    lib = _lib.load()
    N, H, W_ = 3, 24, 37
    g = torch.Generator(device="cuda").manual_seed(100 * k + 10 * sh + sw + pre_act + Cn)
    x = (torch.rand((N, H, W_, Cn), device="cuda", generator=g) - 0.5) * 8
    w = (torch.rand((k * k, Cn), device="cuda", generator=g) - 0.5) * (2.0 / k)
    b = torch.rand(Cn, device="cuda", generator=g) - 0.5
    aff = np.array([1.1, -0.2, 0.9, 0.15], np.float32)
    lin = [37, 1, 20]
    lout = [(v - 1) // sw + 1 for v in lin]
    OH, OW = (H - 1) // sh + 1, (W_ - 1) // sw + 1
    y = torch.full((N * OH * OW + 2, Cn), 7.0, device="cuda")
    gap = torch.zeros((N, OH, Cn), device="cuda")
    li, lo = torch.tensor(lin, dtype=torch.int32, device="cuda"), torch.tensor(lout, dtype=torch.int32, device="cuda")
    ms = lib.rd_debug_lcv3_dw(N, H, W_, Cn, k, sh, sw, pre_act, 0, aff.ctypes.data, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(),
                              li.data_ptr(), lo.data_ptr(), gap.data_ptr())
    torch.cuda.synchronize()
    assert ms >= 0
    assert float((y[N * OH * OW:] - 7.0).abs().max()) == 0.0                          # nothing past the tensor
    y = y[: N * OH * OW].reshape(N, OH, OW, Cn).double().cpu()
    worst, scale = 0.0, 1.0
    for n in range(N):
        xin = x[n, :, : lin[n]].double().cpu().permute(2, 0, 1)[None]                 # the line alone, at its own width
        if pre_act:
            xin = float(aff[0]) * hswish64(xin) + float(aff[1])
        wd = w.double().cpu().t().reshape(Cn, 1, k, k)
        ref = torch.nn.functional.conv2d(xin, wd, b.double().cpu(), stride=(sh, sw), padding=k // 2, groups=Cn)
        ref = (float(aff[2]) * hswish64(ref) + float(aff[3]))[0].permute(1, 2, 0)     # [OH][lout][C]
        assert ref.shape[1] == lout[n]
        worst = max(worst, float((y[n, :, : lout[n]] - ref).abs().max()))
        scale = max(scale, float(ref.abs().max()))
        assert lout[n] == OW or float(y[n, :, lout[n]:].abs().max()) == 0.0
        # the SE row sums over the line's width: every term within the element bound, so the sum within lout x that bound
        e_gap = float((gap[n].double().cpu() - ref.sum(dim=1)).abs().max())
        assert e_gap < lout[n] * 2e-5 * max(1.0, float(ref.abs().max())), (n, e_gap)
    print(f"\n[lcv3 dw {k}x{k} s{sh}{sw} C {Cn} pre_act {pre_act}] max-abs error {worst:.3e}, bound {2e-5 * scale:.3e} (max |ref| {scale:.2f})")
    assert worst < 2e-5 * scale


# ---------------------------------------------------------------------------------------------------------------- 4b. the fused block kernel alone
@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("pre_act", [0, 1])
@pytest.mark.parametrize("cin,cout", [(16, 32), (32, 64), (64, 64)])
def test_fused_block_alone_matches_float64_and_the_separate_operators(cin, cout, pre_act, split):
    """`lcv3_block_kernel` (csrc/kernels_lcv3_block.hip) through rd_debug_lcv3_block: N = 3, H = 24, W = 37 (two column tiles, the second
    5 wide), line widths [37, 1, 20], inputs spanning +-4 so that the hardswish takes its three branches on load, between the layers and in
    the epilogue.  split = 1: the split-fp16 product, 0: the fp32 one.  Compared inside each line's width
      - with the epilogue's hardswish + affine, against a float64 restatement of the line alone at its own width;
      - without it (the form the engine runs), against the separate operators on the same operands: rd_debug_lcv3_dw, then the 1x1
        convolution of rd_debug_conv on the fp32 matrix kernel.
    Bound 2e-5 * max(1, max |ref|), as the 9x9 and local-tail kernels' tests: 9 + cin <= 73 fp32 multiply-adds of O(1) terms and three
    hardswishes per output; the split product drops the lo x lo term, 2^-22 of a product.  The range flag stays down in both routes; one
    input element of 1e5 raises it on the split route only."""
    lib = _lib.load()
    N, H, W_ = 3, 24, 37
    g = torch.Generator(device="cuda").manual_seed(1000 + cin + cout + 2 * pre_act + split)
    x = (torch.rand((N, H, W_, cin), device="cuda", generator=g) - 0.5) * 8
    dw = (torch.rand((9, cin), device="cuda", generator=g) - 0.5) * (2.0 / 3)
    db = torch.rand(cin, device="cuda", generator=g) - 0.5
    pw = (torch.rand((cout, cin), device="cuda", generator=g) - 0.5) * (4.0 / cin ** 0.5)
    pb = torch.rand(cout, device="cuda", generator=g) - 0.5
    aff = np.array([1.1, -0.2, 0.9, 0.15, 1.05, -0.1], np.float32)
    lin = [37, 1, 20]
    li = torch.tensor(lin, dtype=torch.int32, device="cuda")
    flag = torch.zeros(4, dtype=torch.int32, device="cuda")

    def run(out_act, xin):
        y = torch.full((N * H * W_ + 2, cout), 7.0, device="cuda")
        ms = lib.rd_debug_lcv3_block(N, H, W_, cin, cout, pre_act, out_act, split, 0, aff.ctypes.data, xin.data_ptr(), dw.data_ptr(),
                                     db.data_ptr(), pw.data_ptr(), pb.data_ptr(), y.data_ptr(), li.data_ptr(), flag.data_ptr())
        torch.cuda.synchronize()
        assert ms >= 0
        assert float((y[N * H * W_:] - 7.0).abs().max()) == 0.0                        # nothing past the tensor
        return y[: N * H * W_].reshape(N, H, W_, cout)

    y_act, y_lin = run(1, x).double().cpu(), run(0, x)
    assert int(flag[0]) == 0

    # the separate operators on the same operands
    mid = torch.empty((N, H, W_, cin), device="cuda")
    assert lib.rd_debug_lcv3_dw(N, H, W_, cin, 3, 1, 1, pre_act, 0, aff.ctypes.data, x.data_ptr(), dw.data_ptr(), db.data_ptr(), mid.data_ptr(),
                                li.data_ptr(), li.data_ptr(), None) >= 0
    sep = torch.empty((N, H, W_, cout), device="cuda")
    assert lib.rd_debug_conv(N, H, W_, cin, cout, 1, 1, 1, 0, 0, 0, 0, 0, 0, mid.data_ptr(), pw.data_ptr(), None, None, pb.data_ptr(), None,
                             sep.data_ptr(), None) >= 0
    torch.cuda.synchronize()

    worst, worst_sep, scale, scale_sep = 0.0, 0.0, 1.0, 1.0
    for n in range(N):
        xin = x[n, :, : lin[n]].double().cpu().permute(2, 0, 1)[None]                 # the line alone, at its own width
        if pre_act:
            xin = float(aff[0]) * hswish64(xin) + float(aff[1])
        a = torch.nn.functional.conv2d(xin, dw.double().cpu().t().reshape(cin, 1, 3, 3), db.double().cpu(), padding=1, groups=cin)
        a = float(aff[2]) * hswish64(a) + float(aff[3])
        ref = torch.nn.functional.conv2d(a, pw.double().cpu().reshape(cout, cin, 1, 1), pb.double().cpu())
        ref = (float(aff[4]) * hswish64(ref) + float(aff[5]))[0].permute(1, 2, 0)     # [H][lw][cout]
        worst = max(worst, float((y_act[n, :, : lin[n]] - ref).abs().max()))
        scale = max(scale, float(ref.abs().max()))
        s_n = sep[n, :, : lin[n]].double().cpu()
        worst_sep = max(worst_sep, float((y_lin[n, :, : lin[n]].double().cpu() - s_n).abs().max()))
        scale_sep = max(scale_sep, float(s_n.abs().max()))
    print(f"\n[lcv3 block {cin}->{cout} pre_act {pre_act} {'split' if split else 'fp32'}] max-abs error against float64 {worst:.3e} (bound "
          f"{2e-5 * scale:.3e}, max |ref| {scale:.2f}); against the separate operators {worst_sep:.3e} (bound {2e-5 * scale_sep:.3e})")
    assert worst < 2e-5 * scale
    assert worst_sep < 2e-5 * scale_sep

    xb = x.clone()
    xb[0, 5, 3, 2] = 1e5
    run(1, xb)
    assert int(flag[0]) == (1 if split else 0)


# ---------------------------------------------------------------------------------------------------------------- 5. range guard
def test_range_guard_falls_back_to_the_fp32_mode_bit_for_bit(golden_dir, monkeypatch):
    from rapiddoc_amd.engine import RdEngine
    monkeypatch.setenv("RD_PRECISION", "auto")
    big = dict(_state(golden_dir))
    big["backbone.conv1.conv.weight"] = big["backbone.conv1.conv.weight"] * 3e5
    x = torch.from_numpy(golden_x(np.load(golden_dir / "rec5m_seed0_b2_w320.npz"))).cuda()
    ref = RdEngine(KIND, guard="off").load_weights(big).set_precision("fp32").rec_forward(x)
    raw = RdEngine(KIND, guard="off").load_weights(big)
    raw.rec_forward(x)
    assert raw.range_overflow() and not raw.range_overflow()          # raised once, cleared by the read
    eng = RdEngine(KIND).load_weights(big)                            # default guard="sync": the forward itself falls back
    got = eng.rec_forward(x)
    assert eng.precision == "fp32" and eng.range_fallbacks == 1
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


# ---------------------------------------------------------------------------------------------------------------- 6. session
def test_session_from_cfg_chunk_of_six_eager_and_lazy(tmp_path, golden_dir):
    from rapiddoc_amd.session import LazySoftmax, Mi355RecSession
    st = _state(golden_dir)
    sess = Mi355RecSession.from_cfg({"model_path": str(write_weights(tmp_path, "ch_PP-OCRv5_rec_mobile", st))})
    assert sess.kind == KIND and sess.engine.num_classes == 18385
    g = np.load(golden_dir / "rec5m_seed0_b6_w1088.npz")
    x = golden_x(g)                                                   # a chunk of six at full width
    sess.lazy_softmax = False
    eager = sess(x)
    assert type(eager) is np.ndarray and eager.shape == (6, 136, 18385) and float(np.abs(eager.sum(axis=2) - 1.0).max()) < 1e-4
    e = float(np.abs(eager.max(axis=2) - g["prob"]).max())
    print(f"\n[v5 mobile session] max |max prob - reference| = {e:.3e}")
    assert e < TOL and (eager.argmax(axis=2) == g["idx"])[g["top2gap"] > 1e-2].all()
    sess.lazy_softmax = True
    lazy = sess(x)
    assert isinstance(lazy, LazySoftmax) and lazy.shape == eager.shape
    assert np.array_equal(lazy.argmax(axis=2), eager.argmax(axis=2)) and np.array_equal(lazy.max(axis=2), eager.max(axis=2))
    assert not lazy.materialized and sess.softmax_materialized == 0
    assert np.array_equal(np.asarray(lazy), eager)


# ---------------------------------------------------------------------------------------------------------------- 7. pipeline, strict mode
def test_page_pipeline_strict_equals_the_reference_chunk_loop_through_the_session(tmp_path, golden_dir):
    """PagePipeline with the mobile recogniser on 2 synthetic pages (rendered det maps, v6 detector): strict-mode strings == calling the
    session chunk by chunk in the reference's loop (rapid_ocr.py:404-449) on the crops the pipeline made; launches carry lines of
    several widths, each at its reference chunk's width."""
    from rapiddoc_amd.pages import synth_batch
    from rapiddoc_amd.pipeline import PagePipeline, render_text_maps
    from rapiddoc_amd.session import Mi355RecSession
    states = {"ppocrv6_det": _state(golden_dir, "ppocrv6_det"), KIND: _state(golden_dir)}
    pipe = PagePipeline(states, n_rec_streams=2)
    assert pipe.rec_kind == KIND and pipe.rec_mode == "strict" and pipe.rec_lines_in_launch
    pipe.keep_rec_inputs = True
    pages_np, boxes = synth_batch(11, 2)
    pages = torch.from_numpy(pages_np).cuda()
    maps = render_text_maps(boxes, pages_np.shape[1:3], pipe.det_preprocess(pages[:1])[1], pages.device)
    res = pipe.run_batch(pages, None, det_maps_override=maps)
    flat = [ln for r in res for ln in r.lines]
    n = len(flat)
    assert n >= 60
    line_x, line_w = {}, {}
    mixed = 0
    for chunk, x, lw, _i, _p in pipe.last_rec_batches:
        mixed += len(set(int(v) for v in lw)) > 1
        for j, i in enumerate(chunk.tolist()):
            w = int(lw[j])
            assert w == x.shape[3] or float(x[j, :, :, w:].abs().max()) == 0.0             # zeros beyond the line's own width
            line_x[int(i)], line_w[int(i)] = x[j, :, :, :w].cpu().numpy(), w
    assert mixed >= 1                                                   # at least one launch carried lines of more than one width
    assert len(pipe.last_rec_batches) < len(set(line_w.values()))       # fewer launches than distinct widths
    cw, ch, rot, _keep = pipe.last_rec_crop_sizes
    crop_hw = [(int(cw[i]), int(ch[i])) if rot[i] else (int(ch[i]), int(cw[i])) for i in range(n)]
    sess = Mi355RecSession.from_cfg({"model_path": str(write_weights(tmp_path, "ch_PP-OCRv5_rec_mobile", states[KIND]))})
    ratios = np.array([w / float(h) for h, w in crop_hw])
    indices = np.argsort(ratios)
    out = [None] * n
    for beg in range(0, n, 6):
        idxs = [int(i) for i in indices[beg: beg + 6]]
        img_w = int(48 * max(320 / 48, max(ratios[i] for i in idxs)))
        assert all(line_w[i] == img_w for i in idxs)                   # every line got its reference chunk's width
        batch = np.stack([line_x[i] for i in idxs])
        preds = sess(batch)
        for r, (t, s) in enumerate(ocr_host.ctc_decode(preds.argmax(axis=2), preds.max(axis=2), pipe.characters)):
            out[idxs[r]] = (t, s)
    assert [t for t, _s in out] == [t for _q, t, _s in flat]
    assert max(abs(ocr_host.format_score(s) - fs) for (_t, s), (_q, _t2, fs) in zip(out, flat)) <= 1e-3 + 1e-9


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_the_server_kind_still_refuses_per_line_widths(golden_dir):
    from rapiddoc_amd.engine import EngineError, rec_line_table
    eng = _server_engine(golden_dir, "auto")
    x = torch.zeros((2, 3, 48, 320), device="cuda")
    tab = torch.from_numpy(rec_line_table([320, 200], [0, 40])).cuda()
    tokens = torch.zeros((65, eng.rec_token_dim), device="cuda")
    with pytest.raises(EngineError, match="out of scope for ppocrv5_rec_server"):
        eng.rec_backbone_forward_lines(x, tab, tokens)


def test_page_pipeline_refuses_two_recognisers(golden_dir):
    from rapiddoc_amd.pipeline import PagePipeline
    states = {"ppocrv6_det": _state(golden_dir, "ppocrv6_det"), KIND: {}, "ppocrv5_rec_server": {}}
    with pytest.raises(ValueError, match="exactly one recogniser"):
        PagePipeline(states)
