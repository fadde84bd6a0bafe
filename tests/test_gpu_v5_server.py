"""GPU: the PP-OCRv5 server recogniser (`model_kind "ppocrv5_rec_server"`: PPHGNetV2-B4 text_rec + SVTR neck + CTC) against the fixtures
minted from the reference's own modules (tests/golden/make_golden_v5_server.py), its stages and flags against each other, the ragged
sequence convolution (csrc/kernels_seqconv.hip) alone against fp64, and the session / page pipeline on top of it.

Bound of the numeric comparisons: 1e-3 max-abs, the project's stated bound (BASELINE.json north star, tests/test_gpu_parity.py).  With the
synthetic weights the argmax takes only 2-5 classes (the neck's output varies little along T), so index equality says little here; the
numeric comparisons are the yardstick.  Figures are printed before they are asserted (run with -s to see them)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from kind_helpers import engine_cache, golden_x, synth_state, write_weights
from rapiddoc_amd import _lib
from rapiddoc_amd import ocr_host
from rapiddoc_amd import weights as W

pytestmark = pytest.mark.gpu
TOL = 1e-3
KIND = "ppocrv5_rec_server"
TAGS = ["b2_w320", "b1_w96", "b3_w640", "b6_w1088"]


def _state(golden_dir, kind=KIND):
    return synth_state(golden_dir, kind)


_engine = engine_cache(KIND, guard="sync")


@pytest.mark.parametrize("precision", ["auto", "fp32"])
@pytest.mark.parametrize("tag", TAGS)
def test_whole_network_matches_the_reference_fixtures(golden_dir, tag, precision):
    from rapiddoc_amd.engine import REC_WANT_LOGITS, REC_WANT_NECK, REC_WANT_SOFTMAX
    eng = _engine(golden_dir, precision)
    g = np.load(golden_dir / f"rec5s_seed0_{tag}.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    cs = int(g["backbone_cs"])
    tok = eng.rec_backbone_forward(x).cpu().numpy()                                   # [B, T, 2048]
    ref_tok = g["backbone"][:, :, 0, :].transpose(0, 2, 1)                            # [B, 2048 / cs, 1, T] -> [B, T, 2048 / cs]
    assert tok.shape[2] == eng.rec_token_dim == 2048 and tok.shape[:2] == ref_tok.shape[:2]
    e_tok = float(np.abs(tok[:, :, ::cs] - ref_tok).max())
    idx, prob, neck = eng.rec_forward(x, REC_WANT_NECK)
    idx, prob = idx.cpu().numpy(), prob.cpu().numpy()
    e_neck = float(np.abs(neck.cpu().numpy() - g["neck"]).max())
    _, _, lg = eng.rec_forward(x, REC_WANT_LOGITS)
    lg = lg.cpu().numpy()
    sub = g["logits_sub"] if "logits_sub" in g.files else np.load(golden_dir / f"rec5s_seed0_{tag}_logits.npz")["logits_sub"]
    e_lg = max(float(np.abs(lg[:, :, ::61] - sub).max()), float(np.abs(lg[:, 0, :] - g["logits_t0"]).max()))
    _, _, sm = eng.rec_forward(x, REC_WANT_SOFTMAX)
    sm = sm.cpu().numpy()
    ref_sm = torch.softmax(torch.from_numpy(g["logits_t0"]), dim=1).numpy()           # the reference's probabilities of time step 0
    e_sm = max(float(np.abs(sm[:, 0, :] - ref_sm).max()), float(np.abs(sm.max(axis=2) - g["prob"]).max()))
    e_prob = float(np.abs(prob - g["prob"]).max())
    safe = g["top2gap"] > 1e-2
    masked = float(1.0 - safe.mean())
    print(f"\n[v5 server {tag} {precision}] max-abs errors: tokens {e_tok:.3e} neck {e_neck:.3e} logits {e_lg:.3e} softmax {e_sm:.3e} "
          f"prob {e_prob:.3e}; masked share {masked:.4f}; idx mismatches at safe positions {int((idx != g['idx'])[safe].sum())}")
    assert not eng.range_overflow()
    assert e_tok < TOL and e_neck < TOL and e_lg < TOL and e_sm < TOL and e_prob < TOL
    assert masked <= 0.01
    assert (idx == g["idx"])[safe].all()
    assert all(i in t for i, t in zip(idx[~safe].tolist(), g["top2idx"][~safe].tolist()))       # a masked position: one of the reference's top two


def test_fixtures_were_minted_with_todays_generator(golden_dir):
    s = json.loads((golden_dir / "summary_v5_server.json").read_text())
    assert abs(W.checksum(_state(golden_dir)) - s["checksum"]) < 1e-6 * max(1.0, abs(s["checksum"]))


@pytest.mark.parametrize("precision", ["auto", "fp32"])
def test_ctc_flags_agree_with_the_fused_head(golden_dir, precision):
    from rapiddoc_amd.engine import REC_UNFUSED_CTC, REC_WANT_LOGITS, REC_WANT_SOFTMAX
    eng = _engine(golden_dir, precision)
    g = np.load(golden_dir / "rec5s_seed0_b3_w640.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    safe = g["top2gap"] > 1e-2
    i0, p0, _ = eng.rec_forward(x)
    i0, p0 = i0.cpu().numpy(), p0.cpu().numpy()
    for flags in (REC_UNFUSED_CTC, REC_WANT_SOFTMAX, REC_WANT_LOGITS):
        i1, p1, full = eng.rec_forward(x, flags)
        i1, p1 = i1.cpu().numpy(), p1.cpu().numpy()
        d = float(np.abs(p1 - p0).max())
        print(f"\n[v5 server flags {flags} {precision}] max |prob - fused prob| = {d:.3e}")
        assert (i1 == i0)[safe].all() and d < TOL
        if flags == REC_WANT_SOFTMAX:
            sm = full.cpu().numpy()
            assert full.shape == (3, 80, eng.num_classes) and float(np.abs(sm.sum(axis=2) - 1.0).max()) < 1e-4
            assert np.array_equal(sm.argmax(axis=2), i1) and np.array_equal(sm.max(axis=2), p1)   # numpy's view of the tensor written
        if flags == REC_WANT_LOGITS:
            assert np.array_equal(full.cpu().numpy().argmax(axis=2)[safe], i1[safe])
    assert eng.num_classes == 18385


@pytest.mark.parametrize("precision", ["auto", "fp32"])
def test_a_line_is_computed_at_its_padded_width(golden_dir, precision):
    """The same 200-px line alone and zero-padded to 320: the reference's two neck outputs lie >= 1.4e-2 apart at every step of the
    line (d in the fixture), the engine matches EACH within 1e-3 - an engine that ignored the padded width, or padded the attention, the
    1x3 borders or the pooling differently, fails one of the two."""
    from rapiddoc_amd.engine import REC_WANT_NECK
    eng = _engine(golden_dir, precision)
    g = np.load(golden_dir / "rec5s_width_pair.npz")
    assert g["d"].shape == (25,) and float(g["d"].min()) >= 10 * TOL
    x200 = g["x200"]
    x320 = np.zeros((1, 3, 48, 320), np.float32)
    x320[..., :200] = x200
    for x, w in ((x200, 200), (x320, 320)):
        xt = torch.from_numpy(x).cuda()
        tok = eng.rec_backbone_forward(xt).cpu().numpy()
        _, _, neck = eng.rec_forward(xt, REC_WANT_NECK)
        e_tok = float(np.abs(tok - g[f"backbone{w}"][:, :, 0, :].transpose(0, 2, 1)).max())
        e_neck = float(np.abs(neck.cpu().numpy() - g[f"neck{w}"]).max())
        print(f"\n[v5 server width pair {w} {precision}] tokens {e_tok:.3e} neck {e_neck:.3e} (the two references: d = {g['d'].min():.3e} .. {g['d'].max():.3e})")
        assert e_tok < TOL and e_neck < TOL


def _lines(widths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand((n, 3, 48, w), generator=g) * 2 - 1).cuda() for n, w in widths]


@pytest.mark.parametrize("precision", ["auto", "fp32"])
def test_two_stages_equal_the_whole_network_bit_for_bit(golden_dir, precision):
    """Backbone stage per launch into one token buffer + ONE ragged tail over lines of three widths == rd_rec_forward launch by launch."""
    eng = _engine(golden_dir, precision)
    launches = _lines([(2, 320), (3, 96), (1, 640)], seed=21)
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


@pytest.mark.parametrize("precision", ["auto", "fp32"])
def test_a_line_does_not_depend_on_the_launch_it_rides_in(golden_dir, precision):
    """A line alone at [1,3,48,W] == the same line inside a 50-line launch of width W (tokens and the head's result), and a line's tail
    result with and without other lines in the token buffer - bit for bit."""
    eng = _engine(golden_dir, precision)
    (x,) = _lines([(50, 328)], seed=22)
    T = ocr_host.rec_seq_len(328)
    tok = eng.rec_backbone_forward(x).clone()
    idx, prob, _ = eng.rec_forward(x)
    idx, prob = idx.clone(), prob.clone()
    for b in (0, 17, 49):
        one = x[b: b + 1].contiguous()
        assert torch.equal(eng.rec_backbone_forward(one)[0], tok[b]), (precision, b)
        i1, p1, _ = eng.rec_forward(one)
        assert torch.equal(i1[0], idx[b]) and torch.equal(p1[0], prob[b]), (precision, b, float((p1[0] - prob[b]).abs().max()))
    (y,) = _lines([(2, 96)], seed=23)
    tok_y = eng.rec_backbone_forward(y)
    Ty = ocr_host.rec_seq_len(96)
    mixed = torch.cat([tok_y[0], tok[3], tok_y[1], tok[4]], dim=0).contiguous()
    im, pm = eng.rec_tail_forward(mixed, [Ty, T, Ty, T])
    ia, pa = eng.rec_tail_forward(tok[3].contiguous(), [T])
    assert torch.equal(im[Ty: Ty + T], ia) and torch.equal(pm[Ty: Ty + T], pa)
    assert torch.equal(ia, idx[3]) and torch.equal(pa, prob[3])
    assert not eng.range_overflow()


def _seqconv(x0, x1, w, b, lens, split, act=3, T=0):
    lib = _lib.load()
    M, C0 = x0.shape
    C1 = x1.shape[1] if x1 is not None else 0
    N = w.shape[0]
    tokinfo = None
    if lens is not None:
        from rapiddoc_amd.engine import ragged_tables
        tokinfo = torch.from_numpy(ragged_tables(np.asarray(lens))[1]).cuda()
    y = torch.full((M + 2, N), 7.0, device="cuda")
    flag = C.c_int(0)
    ms = lib.rd_debug_seqconv(M, C0, C1, N, T, act, int(split), 0, x0.data_ptr(), x0.stride(0), x1.data_ptr() if C1 else None,
                              x1.stride(0) if C1 else 0, w.data_ptr(), b.data_ptr(), tokinfo.data_ptr() if tokinfo is not None else None,
                              y.data_ptr(), N, C.byref(flag))
    torch.cuda.synchronize()
    assert ms >= 0, "the kernel did not take the shape"
    assert float((y[M:] - 7.0).abs().max()) == 0.0                   # nothing past M
    return y[:M], flag.value


def _seqconv_fp64(x0, x1, w, b, lens):
    """fp64 restatement: y[m] = silu(sum_tap x[m + tap - 1] . w[:, tap] + b), rows outside m's line are zero."""
    x = (x0 if x1 is None else torch.cat([x0, x1], dim=1)).double().cpu()
    M, Cin = x.shape
    wd = w.double().cpu().reshape(w.shape[0], 3, Cin)
    out = torch.zeros((M, w.shape[0]), dtype=torch.float64)
    pos = 0
    for n in lens:
        seg = torch.zeros((n + 2, Cin), dtype=torch.float64)
        seg[1: n + 1] = x[pos: pos + n]
        for tap in range(3):
            out[pos: pos + n] += seg[tap: tap + n] @ wd[:, tap, :].t()
        pos += n
    out = out + b.double().cpu()
    return out * torch.sigmoid(out)


@pytest.mark.parametrize("segs", [(2048, 0), (2048, 2048)], ids=["conv1_K6144", "conv4_K12288"])
@pytest.mark.parametrize("split", [True, False], ids=["split_fp16", "fp32"])
def test_sequence_conv_alone_matches_fp64_on_ragged_lines(segs, split):
    """Ragged lines of 1, 2, 3, 40, 136 and 137 tokens mixed in one buffer, both K-segment forms, unit-scale operands.  Error measured as
    tests/test_gpu_gemm_h1.py measures the pointwise split-fp16 kernel (max-abs error over the largest reference value) against that
    test's bound, 2e-6: the arithmetic per product is the same (22-bit operands, fp32 accumulate).  That bound is the split route's.
    The native fp32 route (RD_PRECISION=fp32) is another arithmetic - v_mfma_f32_32x32x2: ONE fp32 rounding of the accumulator per 2
    products where the fp16 instruction rounds once per 16 - so its bound is derived, not measured: 8 x as many roundings of 2^-24 each
    grow a random-walk error by sqrt(8), and K beyond the gemm_h1 test's largest K (2176) by sqrt(K / 2176):
    2e-6 * sqrt(8 * K / 2176) = 9.5e-6 at K = 6144, 1.3e-5 at K = 12288."""
    C0, C1 = segs
    lens = [1, 137, 2, 40, 3, 136, 1, 40, 2, 137, 3]
    M, Cin, N = sum(lens), C0 + C1, 256
    g = torch.Generator(device="cuda").manual_seed(C0 + C1)
    x0 = (torch.rand((M, C0 + 16), device="cuda", generator=g) - 0.5) * 2          # row stride wider than the segment
    x1 = (torch.rand((M, C1), device="cuda", generator=g) - 0.5) * 2 if C1 else None
    w = (torch.rand((N, 3 * Cin), device="cuda", generator=g) - 0.5) * 2 * (3.0 / (3 * Cin)) ** 0.5    # outputs of unit scale
    b = torch.rand(N, device="cuda", generator=g) - 0.5
    y, flag = _seqconv(x0[:, :C0], x1, w, b, lens, split)
    ref = _seqconv_fp64(x0[:, :C0], x1, w, b, lens)
    err = float((y.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"\n[seqconv K={3 * Cin} {'split' if split else 'fp32'}] max-abs error / max |ref| = {err:.3e} (|ref| max {float(ref.abs().max()):.3f}), flag {flag}")
    assert flag == 0
    assert err < (2e-6 if split else 2e-6 * (8 * 3 * Cin / 2176.0) ** 0.5)
    # the uniform form is the same code path: lines of equal length without a table
    T = 8
    Mu = M // T * T
    yu, _ = _seqconv(x0[:Mu, :C0], x1[:Mu] if C1 else None, w, b, None, split, T=T)
    yr, _ = _seqconv(x0[:Mu, :C0], x1[:Mu] if C1 else None, w, b, [T] * (Mu // T), split)
    assert torch.equal(yu, yr)


def test_sequence_conv_raises_the_range_flag():
    M, C0, N = 70, 64, 64
    x0 = torch.rand((M, C0), device="cuda") - 0.5
    x0[33, 5] = 1e5
    w = (torch.rand((N, 3 * C0), device="cuda") - 0.5) * 0.1
    b = torch.zeros(N, device="cuda")
    _y, flag = _seqconv(x0, None, w, b, [30, 40], True)
    assert flag == 1
    _y, flag = _seqconv(x0, None, w, b, [30, 40], False)
    assert flag == 0                                                  # the fp32 route has no range to leave


def test_per_line_widths_inside_a_launch_are_refused(golden_dir):
    from rapiddoc_amd.engine import EngineError, rec_line_table
    eng = _engine(golden_dir)
    x = torch.zeros((2, 3, 48, 320), device="cuda")
    tab = torch.from_numpy(rec_line_table([320, 200], [0, 40])).cuda()
    tokens = torch.zeros((65, eng.rec_token_dim), device="cuda")
    with pytest.raises(EngineError, match="out of scope for ppocrv5_rec_server"):
        eng.rec_backbone_forward_lines(x, tab, tokens)


def test_session_from_cfg_chunk_of_six_eager_and_lazy(tmp_path, golden_dir):
    from rapiddoc_amd.session import LazySoftmax, Mi355RecSession
    st = _state(golden_dir)
    sess = Mi355RecSession.from_cfg({"model_path": str(write_weights(tmp_path, "ch_PP-OCRv5_rec_server", st))})
    assert sess.kind == KIND and sess.engine.num_classes == 18385
    g = np.load(golden_dir / "rec5s_seed0_b6_w1088.npz")
    x = golden_x(g)                                                   # a chunk of six at full width
    sess.lazy_softmax = False
    eager = sess(x)
    assert type(eager) is np.ndarray and eager.shape == (6, 136, 18385) and float(np.abs(eager.sum(axis=2) - 1.0).max()) < 1e-4
    e = float(np.abs(eager.max(axis=2) - g["prob"]).max())
    print(f"\n[v5 server session] max |max prob - reference| = {e:.3e}")
    assert e < TOL and (eager.argmax(axis=2) == g["idx"])[g["top2gap"] > 1e-2].all()
    sess.lazy_softmax = True
    lazy = sess(x)
    assert isinstance(lazy, LazySoftmax) and lazy.shape == eager.shape
    assert np.array_equal(lazy.argmax(axis=2), eager.argmax(axis=2)) and np.array_equal(lazy.max(axis=2), eager.max(axis=2))
    assert not lazy.materialized and sess.softmax_materialized == 0
    assert np.array_equal(np.asarray(lazy), eager)


def _pages(pipe, seed, n_pages):
    from rapiddoc_amd.pages import synth_batch
    from rapiddoc_amd.pipeline import render_text_maps
    pages_np, boxes = synth_batch(seed, n_pages)
    pages = torch.from_numpy(pages_np).cuda()
    maps = render_text_maps(boxes, pages_np.shape[1:3], pipe.det_preprocess(pages[:1])[1], pages.device)
    return pages, maps


def test_page_pipeline_strict_equals_the_reference_chunk_loop_through_the_session(tmp_path, golden_dir):
    """PagePipeline with the server recogniser on 2 synthetic pages (rendered det maps): strict-mode strings == calling the session chunk
    by chunk in the reference's loop (rapid_ocr.py:404-449) on the crops the pipeline made."""
    from rapiddoc_amd.pipeline import PagePipeline
    from rapiddoc_amd.session import Mi355RecSession
    states = {"ppocrv6_det": _state(golden_dir, "ppocrv6_det"), KIND: _state(golden_dir)}
    pipe = PagePipeline(states, n_rec_streams=2)
    assert pipe.rec_kind == KIND and pipe.rec_mode == "strict"
    pipe.keep_rec_inputs = True
    pages, maps = _pages(pipe, 11, 2)
    res = pipe.run_batch(pages, None, det_maps_override=maps)
    flat = [ln for r in res for ln in r.lines]
    n = len(flat)
    assert n >= 60
    line_x, line_w = {}, {}
    for chunk, x, lw, _i, _p in pipe.last_rec_batches:
        assert len(set(int(v) for v in lw)) == 1 and int(lw[0]) == x.shape[3]       # one padded width per launch, the launch's own
        for j, i in enumerate(chunk.tolist()):
            line_x[int(i)], line_w[int(i)] = x[j].cpu().numpy(), int(lw[j])
    cw, ch, rot, _keep = pipe.last_rec_crop_sizes
    crop_hw = [(int(cw[i]), int(ch[i])) if rot[i] else (int(ch[i]), int(cw[i])) for i in range(n)]
    sess = Mi355RecSession.from_cfg({"model_path": str(write_weights(tmp_path, "ch_PP-OCRv5_rec_server", states[KIND]))})
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
    # lines come back page by page in reading order; pooled index i = the i-th line of that order
    assert [t for t, _s in out] == [t for _q, t, _s in flat]
    assert max(abs(ocr_host.format_score(s) - fs) for (_t, s), (_q, _t2, fs) in zip(out, flat)) <= 1e-3 + 1e-9


def test_v6_pipeline_results_do_not_change_next_to_the_server_kind(golden_dir):
    """The v6 recogniser still takes the per-line-width launches in strict mode and gives the strings of the whole network batch by batch."""
    from rapiddoc_amd.pipeline import PagePipeline
    states = {k: _state(golden_dir, k) for k in ("ppocrv6_det", "ppocrv6_rec")}
    pipe = PagePipeline(states, n_rec_streams=2)
    assert pipe.rec_kind == "ppocrv6_rec" and pipe.rec_lines_in_launch
    pages, maps = _pages(pipe, 11, 2)
    a = [[(t, s) for _q, t, s in r.lines] for r in pipe.run_batch(pages, None, det_maps_override=maps)]
    pipe.rec_two_stage = False
    b = [[(t, s) for _q, t, s in r.lines] for r in pipe.run_batch(pages, None, det_maps_override=maps)]
    assert [len(p) for p in a] == [45, 45]
    assert [[t for t, _s in p] for p in a] == [[t for t, _s in p] for p in b]
    assert max(abs(sa - sb) for pa, pb in zip(a, b) for (_t, sa), (_t2, sb) in zip(pa, pb)) <= 1e-3 + 1e-9


def test_op_lists_of_the_other_kinds_are_what_they_were(golden_dir):
    """The backbone builder gained per-stage strides and a stem3 stride for the text_rec geometry; with their defaults the plans of
    the existing kinds must not move: (name, kind, cfg) of every op of one fixed shape per kind, recorded from the tree before the
    server recogniser was added (tests/golden/op_lists_default_kinds.json)."""
    from rapiddoc_amd.engine import RdEngine
    want = json.loads((golden_dir / "op_lists_default_kinds.json").read_text())
    assert sorted(want) == ["pphgnetv2_b4", "pphgnetv2_b6_formula", "ppocrv6_det", "ppocrv6_rec"]
    old = os.environ.pop("RD_PRECISION", None)                         # the lists were recorded in the default precision
    try:
        for kind, rec in want.items():
            eng = RdEngine(kind).load_weights(_state(golden_dir, kind))
            x = torch.zeros(tuple(rec["shape"]), device="cuda")
            eng.set_profiling(True)
            eng.profile_log.clear()
            {"pphgnetv2_b4": eng.backbone_forward, "pphgnetv2_b6_formula": eng.formula_encoder_forward, "ppocrv6_rec": eng.rec_forward,
             "ppocrv6_det": eng.det_forward}[kind](x)
            got = [[r["name"], r["kind"], r["cfg"]] for r in eng.profile_log]
            eng.set_profiling(False)
            assert got == rec["ops"], kind
    finally:
        if old is not None:
            os.environ["RD_PRECISION"] = old
