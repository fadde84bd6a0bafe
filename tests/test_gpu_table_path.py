"""GPU: the table path around the UniTable networks.

Resample (`rd_preproc_resize_aa_norm`, csrc/kernels_resize_aa.hip): for every Pillow-minted fixture the resampled bytes equal Pillow's
exactly and the normalised floats lie within 2^-21 of the torch CPU expression ((u8.float() / 255) - mean) / std - one fp32 ulp at the
largest magnitude the normalisation can produce (about 4.86); bit-equality is what is expected and printed, the ulp allows for the
division.  A target that is no multiple of four pixels and misaligned buffers (the byte-moving forms of both kernels) against the numpy
restatement, which tests/test_table_path_host.py pins to Pillow.  Input forms, NaN guard rows, the size guards.  `preprocess`: a batch
against each crop alone, device tensors against numpy, "linear" unchanged.  End to end: the ids, structure and boxes the mint recorded
from the reference networks on the PIL-preprocessed crop; `predict`; the matcher behind the engine; seam S3 of the page driver."""
import copy
import ctypes as C
import json

import numpy as np
import pytest
import torch

import table_path_reference as TP
import unitable_reference as R
from rapiddoc_amd import table_unitable as TU
from rapiddoc_amd import weights as W

pytestmark = pytest.mark.gpu
IDS = TU.STAND_IN_IDS
MEAN, STD = TU.NORM_MEAN, TU.NORM_STD
ULP = 2.0 ** -21
NAMES = ["down_down", "up_up", "v_skipped", "h_skipped", "identity", "up_down10", "one_pixel", "600x1000", "120x300"]
_CACHE = {}


def _cases(golden_dir):
    if "cases" not in _CACHE:
        cases = {c[0]: c for c in TP.resample_cases(golden_dir)}
        for name in NAMES[-2:]:
            z = np.load(golden_dir / f"table_path_resample_448_{name}.npz")
            seed, h, w = (int(v) for v in z[name + "_recipe"])
            cases[name] = (name, W.synth_table_crop(seed, h, w), 448, 448, z[name + "_exp"])
        _CACHE["cases"] = cases
    return _CACHE["cases"]


def _normalised(u8_hwc: np.ndarray) -> torch.Tensor:
    """torchvision's ToTensor + Normalize as one torch CPU expression -> [3, OH, OW]"""
    t = torch.from_numpy(np.ascontiguousarray(u8_hwc))
    return ((t.float() / 255 - torch.tensor(MEAN)) / torch.tensor(STD)).permute(2, 0, 1).contiguous()


@pytest.mark.parametrize("name", NAMES)
def test_resample_equals_pillow_byte_for_byte(golden_dir, name):
    from rapiddoc_amd.engine import preproc_resize_aa_norm
    _, src, oh, ow, exp = _cases(golden_dir)[name]
    out, u8 = preproc_resize_aa_norm(torch.from_numpy(src).cuda(), (oh, ow), MEAN, STD, return_u8=True)
    assert np.array_equal(u8.cpu().numpy(), exp)
    ref = _normalised(exp)
    err = float((out.cpu() - ref).abs().max())
    print(f"\n[resize_aa {name}] {src.shape[0]} x {src.shape[1]} -> {oh} x {ow}: bytes equal, float max-abs diff {err:.3e} (bit-equal: {torch.equal(out.cpu(), ref)}), "
          f"largest |value| {float(ref.abs().max()):.3f}")
    assert out.shape == (3, oh, ow) and err <= ULP
    alone = preproc_resize_aa_norm(torch.from_numpy(src).cuda(), (oh, ow), MEAN, STD)          # without the byte output: the same floats
    assert torch.equal(alone, out)


def test_swap_rb_reads_the_source_as_bgr(golden_dir):
    from rapiddoc_amd.engine import preproc_resize_aa_norm
    for name in ("down_down", "h_skipped", "identity"):
        _, src, oh, ow, _ = _cases(golden_dir)[name]
        a, a8 = preproc_resize_aa_norm(torch.from_numpy(src).cuda(), (oh, ow), MEAN, STD, swap_rb=True, return_u8=True)
        b, b8 = preproc_resize_aa_norm(torch.from_numpy(np.ascontiguousarray(src[:, :, ::-1])).cuda(), (oh, ow), MEAN, STD, swap_rb=False, return_u8=True)
        assert torch.equal(a, b) and torch.equal(a8, b8), name


def _raw(src_dev, oh, ow, out_ptr, u8_ptr, swap=0):
    from rapiddoc_amd import _lib
    lib = _lib.load()
    m, s = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    h, w = int(src_dev.shape[0]), int(src_dev.shape[1])
    return lib.rd_preproc_resize_aa_norm(0, src_dev.data_ptr(), h, w, oh, ow, m, s, swap, out_ptr, u8_ptr, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("oh,ow,shift", [(24, 40, 0), (24, 40, 3), (23, 37, 0), (23, 37, 1), (7, 2, 0)])
def test_nan_guard_rows_stay_nan_and_the_byte_moving_kernels_agree(golden_dir, oh, ow, shift):
    """Output buffers with guard rows on both sides, NaN / 0xA5 filled.  shift: the float output starts `shift` floats, the byte output
    `shift` bytes and the source `shift` bytes off their aligned bases - misaligned bases and targets that are no multiple of four pixels
    take the byte-moving form of both kernels.  The expectation is the numpy restatement."""
    _, src, _, _, _ = _cases(golden_dir)["down_down"]
    exp = TP.resize_aa_u8(src, oh, ow)
    guard = 256
    src_buf = torch.zeros(src.size + 8, dtype=torch.uint8, device="cuda")
    src_dev = src_buf[shift:shift + src.size].view(src.shape)
    src_dev.copy_(torch.from_numpy(src))
    n = 3 * oh * ow
    fbuf = torch.full((n + 2 * guard + 4,), float("nan"), device="cuda")
    bbuf = torch.full((n + 2 * guard + 4,), 0xA5, dtype=torch.uint8, device="cuda")
    f0, b0 = guard + shift, guard + shift
    assert _raw(src_dev, oh, ow, fbuf.data_ptr() + 4 * f0, bbuf.data_ptr() + b0) == 0
    torch.cuda.synchronize()
    f, b = fbuf.cpu(), bbuf.cpu()
    assert bool(torch.isnan(f[:f0]).all()) and bool(torch.isnan(f[f0 + n:]).all()) and bool(torch.isfinite(f[f0:f0 + n]).all())
    assert bool((b[:b0] == 0xA5).all()) and bool((b[b0 + n:] == 0xA5).all())
    assert np.array_equal(b[b0:b0 + n].numpy().reshape(oh, ow, 3), exp)
    assert float((f[f0:f0 + n].view(3, oh, ow) - _normalised(exp)).abs().max()) <= ULP


def test_size_guards_return_an_error_and_launch_nothing(golden_dir):
    from rapiddoc_amd import _lib
    from rapiddoc_amd.engine import EngineError, preproc_resize_aa_norm
    lib = _lib.load()
    src = torch.zeros((4, 5, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((3, 8, 8), float("nan"), device="cuda")
    m, s = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    stream = torch.cuda.current_stream().cuda_stream
    for h, w, oh, ow in ((0, 5, 8, 8), (4, 0, 8, 8), (4, 5, 0, 8), (4, 5, 8, -1), (16385, 5, 8, 8), (4, 16385, 8, 8), (4, 5, 16385, 8), (4, 5, 8, 16385)):
        assert lib.rd_preproc_resize_aa_norm(0, src.data_ptr(), h, w, oh, ow, m, s, 0, out.data_ptr(), None, stream) != 0, (h, w, oh, ow)
        assert "1 .. 16384" in lib.rd_create_error().decode()
    assert lib.rd_preproc_resize_aa_norm(0, None, 4, 5, 8, 8, m, s, 0, out.data_ptr(), None, stream) != 0
    assert lib.rd_preproc_resize_aa_norm(0, src.data_ptr(), 4, 5, 8, 8, m, s, 0, None, None, stream) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                     # nothing was launched
    with pytest.raises(EngineError, match="1 .. 16384"):
        preproc_resize_aa_norm(src, (16385, 8), MEAN, STD)
    with pytest.raises(EngineError, match="1 .. 16384"):
        preproc_resize_aa_norm(src, (8, 0), MEAN, STD, return_u8=True)
    with pytest.raises(EngineError):
        preproc_resize_aa_norm(src.float(), (8, 8), MEAN, STD)
    ok = preproc_resize_aa_norm(src, (8, 8), MEAN, STD)         # the largest legal tap count on a tiny image still runs: 16384 -> 1
    tall = preproc_resize_aa_norm(torch.full((16384, 1, 3), 77, dtype=torch.uint8, device="cuda"), (1, 1), (0, 0, 0), (1, 1, 1), return_u8=True)
    assert bool(torch.isfinite(ok).all()) and np.array_equal(tall[1].cpu().numpy(), TP.resize_aa_u8(np.full((16384, 1, 3), 77, np.uint8), 1, 1))


def test_table_cache_survives_its_own_eviction(golden_dir):
    """The per-(in, out) coefficient tables live in a cache of 512 entries that is emptied when full: 300 calls with two new tables each
    cross that point twice; the answers before, across and after it are the restatement's / Pillow's."""
    from rapiddoc_amd.engine import preproc_resize_aa_norm
    _, src, oh, ow, exp = _cases(golden_dir)["down_down"]
    big = torch.from_numpy(W.synth_table_crop(9, 720, 330)).cuda()
    kept = {}
    for i in range(300):
        h, w = 420 + i, 30 + i                              # (h, 5) and (w, 7): 600 distinct tables
        _, u8 = preproc_resize_aa_norm(big[:h, :w].contiguous(), (5, 7), MEAN, STD, return_u8=True)
        if i in (0, 254, 255, 256, 299):
            kept[i] = u8.cpu().numpy()
    for i, got in kept.items():
        assert np.array_equal(got, TP.resize_aa_u8(big[:420 + i, :30 + i].cpu().numpy(), 5, 7)), i
    _, u8 = preproc_resize_aa_norm(torch.from_numpy(src).cuda(), (oh, ow), MEAN, STD, return_u8=True)
    assert np.array_equal(u8.cpu().numpy(), exp)


# ------------------------------------------------------------------------------------------------------------------ the classes
def _class_pil(golden_dir):
    """(the structure class with resize="pil" on the EOS variant the mint tuned for the crop, the BGR crop, the recorded expectation)"""
    exp = TP.load_summary(golden_dir)["class_pil"]
    if "cls" not in _CACHE:
        st = dict(R.dec_state(golden_dir))
        b = st["generator.bias"].copy()
        b[IDS.eos] += np.float32(exp["bias_add"])
        st["generator.bias"] = b
        _CACHE["cls"] = TU.Mi355UniTableStructure(R.state(golden_dir), st, IDS, TU.stand_in_tokens(), max_new_tokens=64, resize="pil")
        _CACHE["crop"] = W.synth_table_crop(int(exp["crop_seed"]), *exp["crop_hw"])
    return _CACHE["cls"], _CACHE["crop"], exp


def test_preprocess_pil_batch_equals_each_crop_alone_and_the_reference_pixels(golden_dir):
    cls, crop, exp = _class_pil(golden_dir)
    crops = [crop, W.synth_table_crop(5, 120, 300), W.synth_table_crop(6, 448, 97)]
    x, shapes = cls.preprocess(crops)
    assert x.shape == (3, 3, 448, 448) and shapes == [(600, 1000), (120, 300), (448, 97)]
    for i, c in enumerate(crops):
        assert torch.equal(cls.preprocess([c])[0][0], x[i]), i
        ref = _normalised(TP.resize_aa_u8(np.ascontiguousarray(c[:, :, ::-1]), 448, 448))      # BGR in, RGB planes out
        assert float((x[i].cpu() - ref).abs().max()) <= ULP
    assert float(x[0].abs().max()) == pytest.approx(exp["x_absmax"], abs=ULP) and float(x[0].mean()) == pytest.approx(exp["x_mean"], abs=1e-5)
    xd, _ = cls.preprocess([torch.from_numpy(c).cuda() for c in crops] + [None])           # device tensors, a None entry dropped
    assert torch.equal(xd, x)
    view = torch.from_numpy(np.pad(crops[1], ((3, 3), (5, 5), (0, 0)))).cuda()[3:-3, 5:-5]    # a non-contiguous device view of a page
    assert torch.equal(cls.preprocess([view])[0][0], x[1])


def test_preprocess_linear_is_unchanged(golden_dir):
    from rapiddoc_amd.engine import preproc_resize_norm
    cls, crop, _ = _class_pil(golden_dir)
    small = W.synth_table_crop(5, 120, 300)
    try:
        cls.resize = "linear"
        x, shapes = cls.preprocess([crop, small])
    finally:
        cls.resize = "pil"
    for i, c in enumerate((crop, small)):
        ref = preproc_resize_norm(torch.from_numpy(c).cuda(), (448, 448), mean=MEAN, std=STD, swap_rb=True)
        assert torch.equal(x[i], ref)
    assert shapes == [(600, 1000), (120, 300)]
    pil = cls.preprocess([crop])[0][0]
    print(f"\n[table preprocess 600 x 1000] linear against PIL-exact: max-abs {float((x[0] - pil).abs().max()):.3f}, mean-abs {float((x[0] - pil).abs().mean()):.4f}")
    assert not torch.equal(x[0], pil)


def test_structure_class_gives_the_reference_ids_structure_and_boxes(golden_dir):
    """The expectation is the mint's (`class_pil`): the reference encoder on the PIL-preprocessed crop, the loop around the reference
    decoder, then the reference's decode_tokens, rescale_bboxes and wrap_with_html_struct.  Ids first, then what the class returns."""
    cls, crop, exp = _class_pil(golden_dir)
    x, shapes = cls.preprocess([crop])
    assert cls.decode_ids(x) == [exp["ids"]]
    struct, boxes = cls([crop])
    assert struct == [(exp["wrapped"], 1.0)]
    assert len(boxes) == 1 and boxes[0].dtype == np.float32 and boxes[0].tolist() == exp["boxes"]


def test_predict_returns_what_the_reference_path_returns(golden_dir):
    cls, crop, exp = _class_pil(golden_dir)
    model = TU.Mi355RapidTable(cls)
    rgb = np.ascontiguousarray(crop[:, :, ::-1])
    got = model.predict(rgb, copy.deepcopy(exp["ocr_result"]))
    assert got == exp["predict"]                            # None: the recorded structure holds no cell and the reference's matcher raises
    assert exp["predict"] is None and exp["html"] == []
    assert model.predict(rgb, []) is None and model.batch_predict([rgb], None) == [None]


class _InjectedIds:
    """The hook of the two tests below: `Mi355UniTableStructure.decode_ids` of ONE instance is wrapped - the engine's encoder and decoder
    run on the preprocessed crops as always, then the ids they return are replaced by recorded ids whose structure holds cells (synthetic
    weights never decode a `<tr> ... </tr>` pair).  Everything behind the ids - decode_tokens, rescale_bboxes, the matcher - is the path
    under test."""

    def __init__(self, cls, ids):
        self.cls, self.ids, self.engine_ids = cls, ids, []

    def __enter__(self):
        real = self.cls.decode_ids

        def decode_ids(x):
            self.engine_ids.append(real(x))
            return [list(self.ids) for _ in range(x.shape[0])]
        self.cls.decode_ids = decode_ids
        return self

    def __exit__(self, *a):
        del self.cls.decode_ids


def test_matcher_runs_behind_the_engine(golden_dir):
    cls, crop, exp = _class_pil(golden_dir)
    inj = json.loads((golden_dir / "table_path_match.json").read_text())["engine_inject"]
    model = TU.Mi355RapidTable(cls)
    rgb = np.ascontiguousarray(crop[:, :, ::-1])
    with _InjectedIds(cls, inj["ids"]) as hook:
        out = model([crop], [copy.deepcopy(inj["ocr_result"])])
        html = model.predict(rgb, copy.deepcopy(inj["ocr_result"]))
    assert hook.engine_ids == [[exp["ids"]], [exp["ids"]]]              # the engine did run, on the reference's pixels
    assert out.pred_htmls == [inj["html"]] and html == inj["html"]
    assert out.cell_bboxes[0].tolist() == inj["cell_bboxes"] and out.logic_points[0].tolist() == inj["logic_points"]


def test_class_runs_through_seam_s3_of_the_page_driver(golden_dir):
    """analyze.PageAnalyzer with the stub layout of test_class_runs_inside_the_table_seam_of_the_page_driver and the class as `table_model`:
    it has `predict`, so the driver takes seam S3 - `TableOcr` (here with a prepared detector and recogniser answer) hands `predict` the
    RGB crop and the OCR list, and the `<table>` part of the answer lands on the table detection."""
    from rapiddoc_amd.analyze import PageAnalyzer
    from rapiddoc_amd.layout_model import LayoutModel
    from rapiddoc_amd.pages import synth_batch
    from rapiddoc_amd.pipeline import PagePipeline
    cls, _, _ = _class_pil(golden_dir)
    inj = json.loads((golden_dir / "table_path_match.json").read_text())["engine_inject"]
    maps = json.loads((golden_dir / "layout_category_maps.json").read_text())
    labels = list(maps["label_to_category"]["pp_doclayoutv2"])
    TAB = (80, 500, 1150, 1000)

    class Session:
        characters = labels

        def __call__(self, x, sf):
            rows = [[labels.index("table"), 0.9, *TAB, 0]] * x.shape[0]
            return [np.asarray(rows, np.float32), np.full(x.shape[0], 1, np.int32)]

    quads = np.array([[[40, 40], [400, 40], [400, 100], [40, 100]], [[600, 40], [1000, 40], [1000, 100], [600, 100]], [[100, 200], [700, 200], [700, 260], [100, 260]]], np.float32)
    texts = [("Item", 0.9), ("5 &lt; 7", 0.8), ("wide", 0.7)]
    model = TU.Mi355RapidTable(cls)
    seen = []
    real_predict = model.predict

    def predict(image, ocr_result, *args, **kwargs):
        seen.append((image.copy(), copy.deepcopy(ocr_result), args, dict(kwargs)))
        return real_predict(image, ocr_result, *args, **kwargs)
    model.predict = predict
    assert hasattr(model, "batch_predict")                              # as the reference's RapidTableModel: both, and `predict` decides
    states = {k: W.synth_state_dict(W.load_manifest(golden_dir / f"manifest_{k}.json"), 0) for k in ("ppocrv6_det", "ppocrv6_rec")}
    an = PageAnalyzer(LayoutModel(Session(), "pp_doclayoutv3"), PagePipeline(states, n_rec_streams=2), table_model=model, table_use_word_box=False,
                      table_det_raw_fn=lambda canvas, n: [quads.copy()], table_rec_fn=lambda canvas, q: list(texts))
    pages_np, _ = synth_batch(0, 1)
    with _InjectedIds(cls, inj["ids"]):
        out = an(torch.from_numpy(pages_np).cuda(), page_scales=[2.0])[0]
        assert len(seen) == 1
        image, ocr_result, args, kwargs = seen[0]
        direct = real_predict(image, copy.deepcopy(ocr_result), *args, **kwargs)
    assert image.dtype == np.uint8 and image.shape == (TAB[3] - TAB[1], TAB[2] - TAB[0], 3)
    assert np.array_equal(image, pages_np[0, TAB[1]:TAB[3], TAB[0]:TAB[2]])
    assert len(ocr_result) == 3 and ocr_result[1] == ["Item", "5 &amp;lt; 7", "wide"] and [float(s) for s in ocr_result[2]] == [0.9, 0.8, 0.7]
    assert np.array_equal(np.asarray(ocr_result[0], np.float32), quads)
    assert args == ([], [], True, False) and kwargs == {"skip_table_orientation": True}
    table = [d for d in out if d["category_id"] == 5][0]
    assert direct == '<html><body><table><tr><td>Item</td><td>5 &amp;lt; 7</td></tr><tr><td colspan="2">wide</td></tr></table></body></html>'
    assert table["html"] == direct[len("<html><body>"):-len("</body></html>")]
