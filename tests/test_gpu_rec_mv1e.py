"""GPU: the multilingual PP-OCRv3 / v4 mobile recognisers (`model_kind "ppocr_rec_mv1e"`: MobileNetV1Enhance scale 0.5 + SVTR neck dims 64 +
CTCHead) against the fixtures minted from the reference's own modules (tests/golden/make_golden_rec_mv1e.py), per-line widths inside one
backbone launch against the same lines launched alone, its stages and its two depthwise routes against each other, the session, the two
new kernels alone (`dw5_strip_kernel`, `mv1e_pool_kernel`, csrc/kernels_mv1e.hip) against float64, and the CTC head at small, odd class
counts.

Bound of the numeric comparisons against the fixtures: 1e-3 * max(1, max |reference|), the project's rule for whole networks.  The strip
kernel alone: 2e-5 * max(1, max |ref|), the bound tests/test_gpu_v5_mobile.py uses for the same 25-term arithmetic.  Everything that
compares the engine with itself on one route is bit for bit.  Figures are printed before they are asserted (-s)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from kind_helpers import bound, engine_cache, golden_x, hswish64, line_launch, rand_lines, synth_state, write_weights
from rapiddoc_amd import _lib
from rapiddoc_amd import ocr_host
from rapiddoc_amd import weights as W

pytestmark = pytest.mark.gpu
TOL = 1e-3
KIND = "ppocr_rec_mv1e"
FIXTURES = [("korean", "b2_w320"), ("korean", "b1_w96"), ("korean", "b3_w640"), ("korean", "b6_w1088"), ("latin", "b6_w1088"), ("latin", "b1_w96")]
STEP = {"korean": 61, "latin": 7}
ROOT = Path(__file__).resolve().parents[1]


def _state(golden_dir, lang="korean"):
    return synth_state(golden_dir, f"{KIND}_{lang}", kind=KIND)


_engines = engine_cache(KIND, state=_state)


def _engine(golden_dir, precision="auto", lang="korean"):
    """One engine per (precision, file) for the module"""
    return _engines(golden_dir, precision, lang)


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("precision", ["auto", "fp32"])
@pytest.mark.parametrize("lang,tag", FIXTURES)
def test_whole_network_matches_the_reference_fixtures(golden_dir, lang, tag, precision):
    from rapiddoc_amd.engine import REC_WANT_LOGITS, REC_WANT_NECK
    eng = _engine(golden_dir, precision, lang)
    g = np.load(golden_dir / f"recmv1e_{lang}_seed0_{tag}.npz")
    x = torch.from_numpy(golden_x(g)).cuda()
    cs = int(g["backbone_cs"])
    tok = eng.rec_backbone_forward(x).cpu().numpy()                                   # [B, T, 512]
    ref_tok = g["backbone"][:, :, 0, :].transpose(0, 2, 1)                            # [B, 512 / cs, 1, T] -> [B, T, 512 / cs]
    assert tok.shape[2] == eng.rec_token_dim == 512 and tok.shape[:2] == ref_tok.shape[:2]
    assert tok.shape[1] == ocr_host.rec_seq_len(x.shape[3])
    e_tok = float(np.abs(tok[:, :, ::cs] - ref_tok).max())
    idx, prob, neck = eng.rec_forward(x, REC_WANT_NECK)
    idx, prob = idx.cpu().numpy(), prob.cpu().numpy()
    assert neck.shape == g["neck"].shape and neck.shape[2] == 64
    e_neck = float(np.abs(neck.cpu().numpy() - g["neck"]).max())
    e_prob = float(np.abs(prob - g["prob"]).max())
    _i, _p, logits = eng.rec_forward(x, REC_WANT_LOGITS)
    sub = logits.cpu().numpy()[:, :, ::STEP[lang]]
    e_log = float(np.abs(sub - g["logits_sub"]).max())
    e_t0 = float(np.abs(logits.cpu().numpy()[:, 0, :] - g["logits_t0"]).max())
    safe = g["top2gap"] > 1e-2
    masked = float(1.0 - safe.mean())
    print(f"\n[mv1e {lang} {tag} {precision}] max-abs errors: tokens {e_tok:.3e} (bound {bound(ref_tok, TOL):.3e}) neck {e_neck:.3e} "
          f"(bound {bound(g['neck'], TOL):.3e}) prob {e_prob:.3e} logits {e_log:.3e} / t0 {e_t0:.3e} (bound {bound(g['logits_sub'], TOL):.3e}); "
          f"masked share {masked:.4f}; idx mismatches at safe positions {int((idx != g['idx'])[safe].sum())}")
    assert not eng.range_overflow()
    assert e_tok < bound(ref_tok, TOL) and e_neck < bound(g["neck"], TOL) and e_prob < TOL
    assert e_log < bound(g["logits_sub"], TOL) and e_t0 < bound(g["logits_t0"], TOL)
    assert masked <= 0.01
    assert (idx == g["idx"])[safe].all()
    assert (_i.cpu().numpy() == g["idx"])[safe].all()


# ---------------------------------------------------------------------------------------------------------------- 2. per-line widths
LINE_W = [96, 322, 330, 200, 640]            # w2 / w4 odd for some (161 / 81, 165 / 83), one line far narrower than the launch


@pytest.mark.parametrize("precision", ["auto", "fp32"])
def test_lines_of_different_widths_in_one_launch_equal_each_line_alone(golden_dir, precision):
    from rapiddoc_amd.engine import REC_WANT_NECK
    eng = _engine(golden_dir, precision)
    g = np.load(golden_dir / "recmv1e_width_pair.npz")
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
    # against the reference: the 200-px line at its own width and at table width 320, backbone and (through the ragged tail's input) neck
    ref200 = g["backbone200"][0, :, 0, :].T
    e200 = float(np.abs(tokens[first[3]: first[3] + T[3]].cpu().numpy() - ref200).max())
    x3, tab3, T3, _f3 = line_launch([torch.nn.functional.pad(lines[3], (0, 120))] + [lines[4]], 640)
    assert T3[0] == 40
    tokens3 = torch.zeros((sum(T3), eng.rec_token_dim), device="cuda")
    eng.rec_backbone_forward_lines(x3, tab3, tokens3)
    ref320 = g["backbone320"][0, :, 0, :].T
    e320 = float(np.abs(tokens3[:40].cpu().numpy() - ref320).max())
    n200 = eng.rec_forward(lines[3], REC_WANT_NECK)[2].cpu().numpy()
    n320 = eng.rec_forward(torch.nn.functional.pad(lines[3], (0, 120)), REC_WANT_NECK)[2].cpu().numpy()
    en200, en320 = float(np.abs(n200 - g["neck200"]).max()), float(np.abs(n320 - g["neck320"]).max())
    print(f"\n[mv1e lines {precision}] 200-px line in a 640 launch: at width 200 {e200:.3e} (bound {bound(ref200, TOL):.3e}), at table width 320 "
          f"{e320:.3e} (bound {bound(ref320, TOL):.3e}); neck alone {en200:.3e} / {en320:.3e} (bound {bound(g['neck200'], TOL):.3e}), the two widths "
          f"are {float(g['d'].min()):.3e} apart")
    assert e200 < bound(ref200, TOL) and e320 < bound(ref320, TOL)
    assert en200 < bound(g["neck200"], TOL) and en320 < bound(g["neck320"], TOL)
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


_ROUTE_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from rapiddoc_amd import ocr_host, weights as W
from rapiddoc_amd.engine import RdEngine, rec_line_table
golden, out = sys.argv[2], sys.argv[3]
st = W.synth_state_dict(W.load_manifest(golden + "/manifest_ppocr_rec_mv1e_korean.json"), 0, kind="ppocr_rec_mv1e")
eng = RdEngine("ppocr_rec_mv1e", guard="off").load_weights(st)
widths = [96, 322, 330, 200, 640]
g = torch.Generator().manual_seed(31)
lines = [(torch.rand((1, 3, 48, w), generator=g) * 2 - 1).cuda() for w in widths]
alone = [eng.rec_backbone_forward(ln)[0].clone() for ln in lines]
x = torch.zeros((len(lines), 3, 48, 640), device="cuda")
for i, ln in enumerate(lines):
    x[i, :, :, : ln.shape[3]] = ln[0]
T = [ocr_host.rec_seq_len(w) for w in widths]
first = np.concatenate([[0], np.cumsum(T)[:-1]])
tab = torch.from_numpy(rec_line_table(widths, first)).cuda()
tokens = torch.zeros((sum(T), eng.rec_token_dim), device="cuda")
eng.rec_backbone_forward_lines(x, tab, tokens)
same = all(torch.equal(tokens[f: f + t], a) for a, t, f in zip(alone, T, first))
big = torch.cat([lines[1]] * 50)
same50 = bool(torch.equal(eng.rec_backbone_forward(big)[37], alone[1]))
np.savez(out, tokens=tokens.cpu().numpy(), same=np.array(same), same50=np.array(same50), overflow=np.array(eng.range_overflow()))
"""


def test_both_depthwise_routes_are_invariant_and_agree_within_the_bound(golden_dir, tmp_path):
    """RD_MV1E_DW_STRIP=0 (lcv3_dw_kernel on every 5x5 layer) and =1 (dw5_strip_kernel), one fresh child process each: on either route
    the lines of five widths in one launch equal each line alone and a line alone equals the line in a 50-line launch, bit for bit;
    between the routes the tokens agree within the bound (the two kernels add the 25 terms in different orders)."""
    script = tmp_path / "route_child.py"
    script.write_text(_ROUTE_CHILD)
    got = {}
    for route in ("0", "1"):
        out = tmp_path / f"route{route}.npz"
        env = dict(os.environ, RD_MV1E_DW_STRIP=route)
        r = subprocess.run([sys.executable, str(script), str(ROOT), str(golden_dir), str(out)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got[route] = np.load(out)
        assert bool(got[route]["same"]) and bool(got[route]["same50"]) and not bool(got[route]["overflow"]), route
    a, b = got["0"]["tokens"], got["1"]["tokens"]
    e = float(np.abs(a - b).max())
    print(f"\n[mv1e routes] direct against strip: max-abs difference of the tokens {e:.3e} (bound {bound(a, TOL):.3e}, max |tokens| {float(np.abs(a).max()):.2f})")
    assert e < bound(a, TOL)


# ---------------------------------------------------------------------------------------------------------------- 4. session
def test_session_from_cfg_chunk_of_six_eager_and_lazy(tmp_path, golden_dir):
    from rapiddoc_amd.session import LazySoftmax, Mi355RecSession
    st = _state(golden_dir)
    p = write_weights(tmp_path, "korean_PP-OCRv4_rec_mobile", st)
    sess = Mi355RecSession.from_cfg({"model_path": str(p)})
    assert sess.kind == KIND and sess.engine.num_classes == 3690
    g = np.load(golden_dir / "recmv1e_korean_seed0_b6_w1088.npz")
    x = golden_x(g)                                                   # a chunk of six at full width
    sess.lazy_softmax = False
    eager = sess(x)
    assert type(eager) is np.ndarray and eager.shape == (6, 136, 3690) and float(np.abs(eager.sum(axis=2) - 1.0).max()) < 1e-4
    e = float(np.abs(eager.max(axis=2) - g["prob"]).max())
    print(f"\n[mv1e session] max |max prob - reference| = {e:.3e}")
    assert e < TOL and (eager.argmax(axis=2) == g["idx"])[g["top2gap"] > 1e-2].all()
    sess.lazy_softmax = True
    lazy = sess(x)
    assert isinstance(lazy, LazySoftmax) and lazy.shape == eager.shape
    assert np.array_equal(lazy.argmax(axis=2), eager.argmax(axis=2)) and np.array_equal(lazy.max(axis=2), eager.max(axis=2))
    assert not lazy.materialized and sess.softmax_materialized == 0
    assert np.array_equal(np.asarray(lazy), eager)


def test_page_pipeline_strict_equals_the_reference_chunk_loop_through_the_session(tmp_path, golden_dir):
    """PagePipeline with this kind (the latin file, 187 classes) on 2 synthetic pages (rendered det maps, v6 detector): strict-mode strings
    == calling the session chunk by chunk in the reference's loop on the crops the pipeline made; launches carry lines of several widths,
    each at its reference chunk's width."""
    from rapiddoc_amd.pages import synth_batch
    from rapiddoc_amd.pipeline import PagePipeline, render_text_maps
    from rapiddoc_amd.session import Mi355RecSession
    states = {"ppocrv6_det": W.synth_state_dict(W.load_manifest(golden_dir / "manifest_ppocrv6_det.json"), 0), KIND: _state(golden_dir, "latin")}
    pipe = PagePipeline(states, n_rec_streams=2)
    assert pipe.rec_kind == KIND and pipe.rec_mode == "strict" and pipe.rec_lines_in_launch and len(pipe.characters) == 187
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
    p = tmp_path / "latin_PP-OCRv3_rec_mobile.safetensors"
    p.write_bytes(W.to_safetensors_bytes(states[KIND]))
    sess = Mi355RecSession.from_cfg({"model_path": str(p)})
    assert sess.kind == KIND
    ratios = np.array([w / float(h) for h, w in crop_hw])
    indices = np.argsort(ratios)
    out = [None] * n
    for beg in range(0, n, 6):
        idxs = [int(i) for i in indices[beg: beg + 6]]
        img_w = int(48 * max(320 / 48, max(ratios[i] for i in idxs)))
        assert all(line_w[i] == img_w for i in idxs)                   # every line got its reference chunk's width
        batch = np.stack([line_x[i] for i in idxs])
        preds = sess(batch)
        for r, (t, sc) in enumerate(ocr_host.ctc_decode(preds.argmax(axis=2), preds.max(axis=2), pipe.characters)):
            out[idxs[r]] = (t, sc)
    assert [t for t, _s in out] == [t for _q, t, _s in flat]
    assert max(abs(ocr_host.format_score(sc) - fs) for (_t, sc), (_q, _t2, fs) in zip(out, flat)) <= 1e-3 + 1e-9


# ---------------------------------------------------------------------------------------------------------------- 5. the strip kernel alone
@pytest.mark.parametrize("sh,sw", [(1, 1), (2, 1), (1, 2)])
@pytest.mark.parametrize("pre_act,post_act", [(1, 1), (0, 1), (1, 0), (0, 0)])
@pytest.mark.parametrize("H,W_,Cn", [(6, 37, 48), (3, 70, 16), (2, 37, 16), (1, 1, 48), (6, 70, 16)])
def test_strip_kernel_alone_matches_float64(sh, sw, pre_act, post_act, H, W_, Cn):
    """`dw5_strip_kernel` through rd_debug_dw5_strip against float64 conv2d: N = 3; H = 6 (the network's), 3, 2, 1 (rows of the halo
    outside the map on both sides); W = 37 (inside one strip), 70 (two strips of 64 at SW = 1, three of 32 output columns at SW = 2), 1;
    C = 16 (one channel slice) and 48 (three); row strides of x / y larger than C; non-identity affines; line widths [W, 1, 20] (for
    W = 70 at SW = 1 line 1 and 2 leave the second strip wholly beyond the line: it must write zeros); inputs spanning +-4 so that
    all three branches of the hardswish are taken.  Compared inside each line's output width; beyond it zeros; a NaN guard band around
    and between the pixels (the padding channels of y) stays NaN.  Bound 2e-5 * max(1, max |ref|) (25 fp32 multiply-adds of O(1) terms, two
    hardswishes, two affines).  Where post_act = 1 also against `lcv3_dw_kernel` on the same operands, within twice the bound."""
    lib = _lib.load()
    N, xld, yld = 3, Cn + 8, Cn + 4
    g = torch.Generator(device="cuda").manual_seed(1000 * H + 10 * W_ + 100 * sh + sw + pre_act + 2 * post_act + Cn)
    xbuf = torch.full((N, H, W_, xld), float("nan"), device="cuda")
    xbuf[..., :Cn] = (torch.rand((N, H, W_, Cn), device="cuda", generator=g) - 0.5) * 8
    x = xbuf[..., :Cn]
    w = (torch.rand((25, Cn), device="cuda", generator=g) - 0.5) * 0.4
    b = torch.rand(Cn, device="cuda", generator=g) - 0.5
    aff = np.array([1.1, -0.2, 0.9, 0.15], np.float32)
    lin = [W_, 1, min(20, W_)]
    lout = [(v - 1) // sw + 1 for v in lin]
    OH, OW = (H - 1) // sh + 1, (W_ - 1) // sw + 1
    guard = 5
    ybuf = torch.full((guard + N * OH * OW + guard, yld), float("nan"), device="cuda")
    li, lo = torch.tensor(lin, dtype=torch.int32, device="cuda"), torch.tensor(lout, dtype=torch.int32, device="cuda")
    ms = lib.rd_debug_dw5_strip(N, H, W_, Cn, sh, sw, pre_act, post_act, xld, yld, 0, aff.ctypes.data, xbuf.data_ptr(), w.data_ptr(), b.data_ptr(),
                                ybuf[guard:].data_ptr(), li.data_ptr(), lo.data_ptr())
    torch.cuda.synchronize()
    assert ms >= 0
    assert bool(torch.isnan(ybuf[:guard]).all()) and bool(torch.isnan(ybuf[guard + N * OH * OW:]).all())      # the guard band is untouched
    assert bool(torch.isnan(ybuf[:, Cn:]).all())                                                              # ... and y's padding channels
    y = ybuf[guard: guard + N * OH * OW, :Cn].reshape(N, OH, OW, Cn)
    assert not bool(torch.isnan(y).any())
    yd = y.double().cpu()
    worst, scale = 0.0, 1.0
    for n in range(N):
        xin = x[n, :, : lin[n]].double().cpu().permute(2, 0, 1)[None]                 # the line alone, at its own width
        if pre_act:
            xin = float(aff[0]) * hswish64(xin) + float(aff[1])
        wd = w.double().cpu().t().reshape(Cn, 1, 5, 5)
        ref = torch.nn.functional.conv2d(xin, wd, b.double().cpu(), stride=(sh, sw), padding=2, groups=Cn)
        if post_act:
            ref = float(aff[2]) * hswish64(ref) + float(aff[3])
        ref = ref[0].permute(1, 2, 0)                                                 # [OH][lout][C]
        assert ref.shape[:2] == (OH, lout[n])
        worst = max(worst, float((yd[n, :, : lout[n]] - ref).abs().max()))
        scale = max(scale, float(ref.abs().max()))
        assert lout[n] == OW or float(yd[n, :, lout[n]:].abs().max()) == 0.0          # zeros beyond the line's output width
    print(f"\n[dw5 strip s{sh}{sw} H {H} W {W_} C {Cn} pre {pre_act} post {post_act}] max-abs error {worst:.3e}, bound {2e-5 * scale:.3e} (max |ref| {scale:.2f})")
    assert worst < 2e-5 * scale
    if post_act:
        xc = x.contiguous()
        y2 = torch.zeros((N, OH, OW, Cn), device="cuda")
        assert lib.rd_debug_lcv3_dw(N, H, W_, Cn, 5, sh, sw, pre_act, 0, aff.ctypes.data, xc.data_ptr(), w.data_ptr(), b.data_ptr(), y2.data_ptr(),
                                    li.data_ptr(), lo.data_ptr(), None) >= 0
        torch.cuda.synchronize()
        e2 = float((y2 - y).abs().max())
        print(f"    against lcv3_dw_kernel: {e2:.3e} (bound {4e-5 * scale:.3e})")
        assert e2 < 4e-5 * scale


def test_strip_kernel_declines_what_it_does_not_cover():
    lib = _lib.load()
    aff = np.array([1, 0, 1, 0], np.float32)
    z = torch.zeros(8 * 7 * 40 * 32, device="cuda")
    args = (aff.ctypes.data, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None, None)
    assert lib.rd_debug_dw5_strip(1, 6, 40, 16, 1, 1, 0, 1, 16, 16, 0, *args) >= 0
    assert lib.rd_debug_dw5_strip(1, 7, 40, 16, 1, 1, 0, 1, 16, 16, 0, *args) < 0          # more than 6 rows
    assert lib.rd_debug_dw5_strip(1, 6, 40, 24, 1, 1, 0, 1, 24, 24, 0, *args) < 0          # channels % 16
    assert lib.rd_debug_dw5_strip(1, 6, 40, 16, 2, 2, 0, 1, 16, 16, 0, *args) < 0          # stride (2,2)
    assert lib.rd_debug_dw5_strip(1, 6, 40, 16, 1, 1, 0, 1, 12, 16, 0, *args) < 0          # row stride below C
    assert lib.rd_debug_dw5_strip(1, 6, 40, 16, 1, 1, 0, 1, 18, 16, 0, *args) < 0          # pixels not 16-byte aligned
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 6. the pool kernel alone
def test_pool_kernel_alone_ignores_row_2_and_follows_the_line_table():
    from rapiddoc_amd.engine import rec_line_table
    lib = _lib.load()
    N, H, W4, Cn = 3, 3, 21, 32
    g = torch.Generator(device="cuda").manual_seed(5)
    x = (torch.rand((N, H, W4, Cn), device="cuda", generator=g) - 0.5) * 8
    ref = hswish64(x[:, :2, :20].double()).reshape(N, 2, 10, 2, Cn).mean(dim=(1, 3))            # [N][10][C]
    y = torch.full((N, W4 // 2, Cn), 7.0, device="cuda")
    assert lib.rd_debug_mv1e_pool(N, H, W4, Cn, x.data_ptr(), y.data_ptr(), None) == 0
    e = float((y.double() - ref).abs().max())
    bound = 2e-5 * max(1.0, float(ref.abs().max()))           # 4 hardswishes (3 roundings each) and 4 adds of values up to max |ref| * 4
    print(f"\n[mv1e pool] max-abs error {e:.3e} (bound {bound:.3e})")
    assert e < bound
    xp = x.clone()
    xp[:, 2] = float("nan")                                                            # a poisoned row 2 changes nothing
    y2 = torch.zeros_like(y)
    assert lib.rd_debug_mv1e_pool(N, H, W4, Cn, xp.data_ptr(), y2.data_ptr(), None) == 0
    assert torch.equal(y2, y)
    # line table: widths whose w4 are 21, 6 and 13 -> 10, 3 and 6 tokens, rows in a permuted order of a compact buffer
    widths = [81, 21, 49]
    assert [((w - 1) // 2) // 2 + 1 for w in widths] == [21, 6, 13]
    T = [ocr_host.rec_seq_len(w) for w in widths]
    assert T == [10, 3, 6]
    first = [9, 0, 3]
    tab = torch.from_numpy(rec_line_table(widths, first)).cuda()
    buf = torch.full((sum(T) + 2, Cn), 7.0, device="cuda")
    assert lib.rd_debug_mv1e_pool(N, H, W4, Cn, xp.data_ptr(), buf.data_ptr(), tab.data_ptr()) == 0
    for n in range(N):
        assert torch.equal(buf[first[n]: first[n] + T[n]], y[n, : T[n]]), n
    assert float((buf[sum(T):] - 7.0).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- 7. small, odd class counts
@pytest.mark.parametrize("ncls", [130, 187])
def test_ctc_head_at_small_odd_class_counts(golden_dir, ncls):
    """`ctc_head` (flags 0), `ctc_stats` (REC_UNFUSED_CTC / REC_WANT_LOGITS) and `softmax_rows` (REC_WANT_SOFTMAX) at 130 and 187 classes,
    T = 12 (width 96), through a synthetic state of this kind whose classifier has that many rows, against float64 on the engine's own
    neck output (K = 64, padded to 128 by the fused head).  Bound of a logit: 65 sequentially rounded fp32 terms, each |x_k w_k| <= S_row
    in sum, twice for the split-fp16 operands' own 2^-22 representation: 2 * 65 * 2^-24 * max_row(sum_k |x_k w_k| + |bias|).  A
    probability moves by at most twice the logit error (softmax is 1-Lipschitz per logit in the sup norm up to the factor 2) plus 1e-6 for the exponentials."""
    from rapiddoc_amd.engine import REC_UNFUSED_CTC, REC_WANT_LOGITS, REC_WANT_NECK, REC_WANT_SOFTMAX, RdEngine
    man = [(n, ((ncls,) + tuple(s[1:]) if n.startswith("head.fc.") else s), d) for n, s, d in W.load_manifest(golden_dir / f"manifest_{KIND}_latin.json")]
    st = W.synth_state_dict(man, 0, kind=KIND)
    assert st["head.fc.weight"].shape == (ncls, 64) and st["head.fc.bias"].shape == (ncls,)
    eng = RdEngine(KIND, guard="off").load_weights(st)
    assert eng.num_classes == ncls
    x = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, (3, 3, 48, 96)).astype(np.float32)).cuda()
    i0, p0, neck = (t.clone() for t in eng.rec_forward(x, REC_WANT_NECK))
    assert neck.shape == (3, 12, 64)
    nk = neck.double().cpu().numpy()
    w64, b64 = st["head.fc.weight"].astype(np.float64), st["head.fc.bias"].astype(np.float64)
    ref = nk @ w64.T + b64
    s_row = float((np.abs(nk) @ np.abs(w64).T + np.abs(b64)).max())
    lb = 2 * 65 * 2.0 ** -24 * s_row
    sm = np.exp(ref - ref.max(axis=2, keepdims=True))
    sm /= sm.sum(axis=2, keepdims=True)
    top2 = np.sort(ref, axis=2)[..., -2:]
    safe = (top2[..., 1] - top2[..., 0]) > 2 * lb
    assert safe.mean() > 0.9
    i1, p1, _ = (t.clone() if t is not None else None for t in eng.rec_forward(x, REC_UNFUSED_CTC))
    i2, p2, logits = (t.clone() for t in eng.rec_forward(x, REC_WANT_LOGITS))
    i3, p3, soft = (t.clone() for t in eng.rec_forward(x, REC_WANT_SOFTMAX))
    e_log = float(np.abs(logits.cpu().numpy() - ref).max())
    e_soft = float(np.abs(soft.cpu().numpy() - sm).max())
    print(f"\n[mv1e {ncls} classes] logits {e_log:.3e} (bound {lb:.3e}, max |ref| {np.abs(ref).max():.1f}); softmax {e_soft:.3e}; "
          f"prob: fused {float(np.abs(p0.cpu().numpy() - sm.max(axis=2)).max()):.3e} unfused {float(np.abs(p1.cpu().numpy() - sm.max(axis=2)).max()):.3e}")
    assert logits.shape == (3, 12, ncls) and soft.shape == (3, 12, ncls)
    assert e_log < lb and e_soft < 2 * lb + 1e-6
    assert float(np.abs(soft.cpu().numpy().sum(axis=2) - 1.0).max()) < 1e-5
    for name, i, p in (("fused", i0, p0), ("unfused", i1, p1), ("logits", i2, p2), ("softmax", i3, p3)):
        assert (i.cpu().numpy() == ref.argmax(axis=2))[safe].all(), name
        assert 0 <= int(i.min()) and int(i.max()) < ncls, name
        assert float(np.abs(p.cpu().numpy() - sm.max(axis=2)).max()) < 2 * lb + 1e-6, name
    assert not eng.range_overflow()
