"""CPU: the OCR-model seam without RapidDoc and without a GPU.  `plugin.install_ocr_model` against stand-in `rapid_doc` modules in
`sys.modules`; `ocr_model.Mi355RapidOcrModel`'s constructor, argument checks and the return nesting of its `ocr` forms over stubbed
device stages; `LazyLineCrop` against the project's restatement of the reference's crop (oracle/cv2_ops.py) injected as the "original"
function; the packing of `rd_line_source_desc` against a numpy restatement."""
import sys
import types

import numpy as np
import pytest

from oracle import cv2_ops


# ---------------------------------------------------------------------------------------------------------------- stand-ins
def _stand_in_modules():
    """the three modules install_ocr_model touches, with recording originals"""
    names = ("rapid_doc", "rapid_doc.backend", "rapid_doc.backend.pipeline", "rapid_doc.backend.pipeline.model_init", "rapid_doc.utils",
             "rapid_doc.utils.ocr_utils", "rapid_doc.backend.pipeline.analyze_utils")
    mods = {name: types.ModuleType(name) for name in names}
    calls = []

    def ocr_model_init(det_db_box_thresh=0.5, lang=None, ocr_config=None, det_db_unclip_ratio=1.8, enable_merge_det_boxes=True, is_seal=False):
        calls.append((det_db_box_thresh, lang, ocr_config, det_db_unclip_ratio, enable_merge_det_boxes, is_seal))
        return ("reference model", is_seal)

    def get_rotate_crop_image(img, points):
        calls.append("crop")
        return cv2_ops.get_rotate_crop_image(img, points)

    mods["rapid_doc.backend.pipeline.model_init"].ocr_model_init = ocr_model_init
    mods["rapid_doc.utils.ocr_utils"].get_rotate_crop_image = get_rotate_crop_image
    mods["rapid_doc.backend.pipeline.analyze_utils"].get_rotate_crop_image = get_rotate_crop_image       # `from ...ocr_utils import ...`
    return mods, calls


@pytest.fixture()
def rapid_doc(monkeypatch):
    mods, calls = _stand_in_modules()
    for name, mod in mods.items():
        monkeypatch.setitem(sys.modules, name, mod)
    return mods, calls


class _StubPipe:
    use_cls = False
    rec_mode = "strict"


# ---------------------------------------------------------------------------------------------------------------- install / uninstall
def test_install_replaces_the_factory_and_uninstall_restores_identity(rapid_doc):
    from rapiddoc_amd import ocr_model, plugin
    mods, calls = rapid_doc
    init, utils, users = (mods["rapid_doc.backend.pipeline.model_init"], mods["rapid_doc.utils.ocr_utils"],
                          mods["rapid_doc.backend.pipeline.analyze_utils"])
    original, crop = init.ocr_model_init, utils.get_rotate_crop_image
    pipe = _StubPipe()
    uninstall = plugin.install_ocr_model({"ch": pipe})                       # the default: module found by import, crops stay on the host
    assert init.ocr_model_init is not original and utils.get_rotate_crop_image is crop and users.get_rotate_crop_image is crop
    # the six positional arguments of atom_model_init (model_init.py:105-112)
    model = init.ocr_model_init(0.3, "ch", {"use_det_mode": "auto", "Det.unclip_ratio": 1.6}, 1.8, False, False)
    assert isinstance(model, ocr_model.Mi355RapidOcrModel) and model.pipe is pipe and model.lang == "ch"
    assert model.box_thresh == 0.3 and model.unclip_ratio == 1.6 and model.enable_merge_det_boxes is False and model.is_seal is False
    assert (model.drop_score, model.rec_batch_num) == (0.5, 6) and calls == []
    # a seal request reaches the original, with all six arguments
    assert init.ocr_model_init(0.6, "ch", None, 0.5, False, True) == ("reference model", True)
    assert calls == [(0.6, "ch", None, 0.5, False, True)]
    with pytest.raises(KeyError, match="'en'"):
        init.ocr_model_init(0.3, "en", None, 1.8, True, False)
    # a second install is a no-op
    installed = init.ocr_model_init
    assert plugin.install_ocr_model({"ch": pipe}) is uninstall and init.ocr_model_init is installed
    uninstall()
    assert init.ocr_model_init is original and utils.get_rotate_crop_image is crop and users.get_rotate_crop_image is crop
    uninstall()                                                                # harmless
    assert init.ocr_model_init is original


def test_device_crops_replaces_both_names_of_the_crop_function(rapid_doc):
    from rapiddoc_amd import ocr_model, plugin
    mods, calls = rapid_doc
    init, utils, users = (mods["rapid_doc.backend.pipeline.model_init"], mods["rapid_doc.utils.ocr_utils"],
                          mods["rapid_doc.backend.pipeline.analyze_utils"])
    original, crop = init.ocr_model_init, utils.get_rotate_crop_image
    uninstall = plugin.install_ocr_model(_StubPipe(), device_crops=True, module=init)
    assert utils.get_rotate_crop_image is users.get_rotate_crop_image and utils.get_rotate_crop_image is not crop
    img = np.arange(40 * 60 * 3, dtype=np.uint8).reshape(40, 60, 3)
    lazy = utils.get_rotate_crop_image(img, np.float32([[5, 5], [45, 5], [45, 25], [5, 25]]))
    assert isinstance(lazy, ocr_model.LazyLineCrop) and lazy.source is img and lazy.shape == (20, 40, 3) and calls == []
    assert np.array_equal(np.asarray(lazy), cv2_ops.get_rotate_crop_image(img, lazy.points)) and calls == ["crop"]
    uninstall()
    assert utils.get_rotate_crop_image is crop and users.get_rotate_crop_image is crop and init.ocr_model_init is original
    # a user module that holds another function under that name is left alone
    users.get_rotate_crop_image = other = lambda img, points: None
    uninstall = plugin.install_ocr_model(_StubPipe(), device_crops=True, module=init)
    assert users.get_rotate_crop_image is other and utils.get_rotate_crop_image is not crop
    uninstall()
    assert users.get_rotate_crop_image is other and utils.get_rotate_crop_image is crop


def test_install_without_rapid_doc_says_so():
    from rapiddoc_amd import plugin
    assert "rapid_doc" not in sys.modules
    with pytest.raises(ImportError, match="model_init"):
        plugin.install_ocr_model(_StubPipe())


# ---------------------------------------------------------------------------------------------------------------- constructor, arguments
def test_constructor_follows_the_reference_and_names_what_it_does_not_serve():
    from rapiddoc_amd.ocr_model import Mi355RapidOcrModel
    pipe = _StubPipe()
    m = Mi355RapidOcrModel(pipe)
    assert (m.drop_score, m.rec_batch_num, m.enable_merge_det_boxes, m.is_seal) == (0.5, 6, True, False)
    assert (m.box_thresh, m.unclip_ratio) == (0.5, 1.8) and m.params["Det.limit_side_len"] == 960 and m.params["Det.limit_type"] == "max"
    # driver keys are ignored, as the reference pops them; model-choice keys cannot change a result here
    m = Mi355RapidOcrModel(pipe, 0.3, "ch", {"engine_type": "torch", "use_det_mode": "auto", "custom_model": object(), "seal_enable": True,
                                              "Det.model_path": "x.onnx", "Rec.ocr_version": "PP-OCRv5", "EngineConfig.torch.use_cuda": True,
                                              "Det.limit_side_len": 960, "Det.mean": [0.485, 0.456, 0.406], "Global.use_cls": False,
                                              "Det.box_thresh": 0.4})
    assert m.box_thresh == 0.4 and m.unclip_ratio == 1.8
    for key, value in (("Det.limit_side_len", 736), ("Det.limit_type", "min"), ("Det.thresh", 0.2), ("Det.box_type", "poly"),
                       ("Global.use_cls", True), ("Rec.rec_batch_num", 8), ("Det.use_dilation", False), ("Cls.cls_thresh", 0.8),
                       ("Global.text_score", 0.3), ("Det.max_side_limit", 4000)):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            Mi355RapidOcrModel(pipe, ocr_config={key: value})
    with pytest.raises(ValueError, match="is_seal"):
        Mi355RapidOcrModel(pipe, is_seal=True)
    with pytest.raises(ValueError, match="use_dilation"):
        Mi355RapidOcrModel(pipe, use_dilation=False)
    cls_pipe = _StubPipe()
    cls_pipe.use_cls = True
    with pytest.raises(ValueError, match="use_cls"):
        Mi355RapidOcrModel(cls_pipe)
    with pytest.raises(KeyError, match="'ja'"):
        Mi355RapidOcrModel({"ch": pipe}, lang="ja")


def test_return_nesting_of_the_ocr_forms_over_stubbed_stages():
    """what RapidDoc indexes: `ocr(...)[0]` of every form (rapid_ocr.py:244-299)"""
    from rapiddoc_amd.ocr_model import Mi355RapidOcrModel
    m = Mi355RapidOcrModel(_StubPipe())
    img = np.full((32, 64, 3), 255, np.uint8)
    box = np.float32([[1, 2], [30, 2], [30, 12], [1, 12]])
    with pytest.raises(ValueError, match="det must be false"):
        m.ocr([img], det=True)
    seen = []

    def det_rec(image, mfd_res, rec):
        seen.append((image.shape, mfd_res, rec))
        return ([box, box + 20], [("ab", 0.9), ("cd", 0.7)] if rec else None)
    m._det_rec = det_rec
    mfd = [{"bbox": [0, 0, 4, 4]}]
    assert m.ocr(img, mfd_res=mfd, rec=False) == [[box.tolist(), (box + 20).tolist()]]
    assert m.ocr(img, mfd_res=mfd) == [[[box.tolist(), ("ab", 0.9)], [(box + 20).tolist(), ("cd", 0.7)]]]
    assert m.ocr(img[:, :, 0]) is not None and seen[-1][0] == (32, 64, 3)              # a grey image arrives as three channels
    assert seen[0] == ((32, 64, 3), mfd, False) and seen[1] == ((32, 64, 3), mfd, True)
    got_boxes, got_lines = m(img)
    assert np.array_equal(got_boxes, [box, box + 20]) and got_lines == [("ab", 0.9), ("cd", 0.7)] and m(None) == (None, None)
    m._det_rec = lambda image, mfd_res, rec: (None, None)                              # the detector found nothing
    assert m.ocr(img, rec=False) == [None] and m.ocr(img) == [None] and m(img) == (None, None)
    m._det_rec = lambda image, mfd_res, rec: ([], [])                                  # every line fell below drop_score
    assert m.ocr(img) == [None]
    # det=False: one pooled call, (text, score) per crop in the caller's order
    pooled = []

    def recognise(crops, want_words):
        pooled.append((len(crops), want_words))
        if want_words:
            return [("ab", 0.9, None), ("", 0.0, None)]
        return [("t%d" % i, 0.5 + i / 10) for i in range(len(crops))]
    m._recognise = recognise
    assert m.ocr([img, img, img], det=False, tqdm_enable=True) == [[("t0", 0.5), ("t1", 0.6), ("t2", 0.7)]]
    assert m.ocr(img, det=False) == [[("t0", 0.5)]] and pooled == [(3, False), (1, False)]
    # the word-box form: words come from the lines that have them; lines without words drop out of the zip (rapid_ocr.py:295,325-326)
    assert m.ocr([img, img], det=False, return_word_box=True, ori_img=img, dt_boxes=[box, box + 20]) == [[]] and pooled[-1] == (2, True)
    assert m.ocr([img, img], det=False, return_word_box=True) == [[("t0", 0.5), ("t1", 0.6)]] and pooled[-1] == (2, False)
    assert m.ocr(img, det=False, rec=False) is None


def test_normalize_image_follows_check_img_and_preprocess_image():
    from rapiddoc_amd.ocr_model import normalize_image
    rng = np.random.default_rng(0)
    grey = rng.integers(0, 256, (5, 7), dtype=np.uint8)
    assert np.array_equal(normalize_image(grey), np.repeat(grey[:, :, None], 3, axis=2))
    bgra = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    alpha = bgra[:, :, 3] / 255                                                         # alpha_to_color, utils/ocr_utils.py:81-91
    want = np.stack([(255 * (1 - alpha) + bgra[:, :, c] * alpha).astype(np.uint8) for c in range(3)], axis=2)
    assert np.array_equal(normalize_image(bgra), want)
    big = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    flipped = big[::-1, ::2]                                                            # negative row stride, pixel stride 6
    got = normalize_image(flipped)
    assert np.array_equal(got, flipped) and got.flags["C_CONTIGUOUS"]
    window = big[2:6, 3:8]
    assert normalize_image(window).base is not None and np.shares_memory(normalize_image(window), big)     # a window stays a view
    with pytest.raises(ValueError, match="shape"):
        normalize_image(np.zeros((3, 3, 2), np.uint8))


# ---------------------------------------------------------------------------------------------------------------- LazyLineCrop
QUADS = {"axis": [[10, 8], [70, 8], [70, 28], [10, 28]],
         "tilted": [[12.3, 9.1], [68.9, 14.2], [66.7, 33.8], [10.2, 28.6]],
         "tall": [[20, 5], [31, 5], [31, 52], [20, 52]],                                 # h / w >= 2: np.rot90
         "just_not_tall": [[20, 5], [40, 5], [40, 44.5], [20, 44.5]],                    # 39 / 20: stays
         "overhang": [[-6, -4], [50, -4], [50, 14], [-6, 14]]}


@pytest.mark.parametrize("name", sorted(QUADS))
def test_lazy_crop_has_the_eager_shape_and_materialises_once(name):
    from rapiddoc_amd.ocr_model import LazyLineCrop, crop_shape, lazy_crop_function
    img = np.random.default_rng(1).integers(0, 256, (60, 80, 3), dtype=np.uint8)
    pts = np.float32(QUADS[name])
    calls = []

    def original(image, points):
        calls.append(1)
        return cv2_ops.get_rotate_crop_image(image, points)
    eager = cv2_ops.get_rotate_crop_image(img, pts)
    lazy = lazy_crop_function(original)(img, pts.copy())
    assert isinstance(lazy, LazyLineCrop) and not isinstance(lazy, np.ndarray) and not lazy.materialized
    assert lazy.shape == eager.shape and len(lazy) == eager.shape[0] and lazy.dtype == np.uint8 and lazy.ndim == 3
    assert lazy.size == eager.size and lazy.nbytes == eager.nbytes and lazy.source is img and np.array_equal(lazy.points, pts)
    w, h, rot = crop_shape(pts)
    assert ((w, h, 3) if rot else (h, w, 3)) == eager.shape and rot == (name == "tall")
    assert calls == []                                                                   # nothing so far has cut the crop
    assert np.array_equal(np.asarray(lazy), eager) and calls == [1] and lazy.materialized
    assert np.array_equal(lazy[2:5, 3], eager[2:5, 3]) and np.array_equal(lazy + 1, eager + 1) and np.array_equal(np.flip(lazy, 0), eager[::-1])
    assert lazy.mean() == eager.mean() and [r.shape for r in lazy] == [r.shape for r in eager]
    assert np.asarray(lazy) is np.asarray(lazy) and calls == [1]                         # cached: the original ran exactly once
    assert np.asarray(lazy, dtype=np.float32).dtype == np.float32


def test_what_has_no_lazy_form_goes_to_the_original():
    from rapiddoc_amd.ocr_model import LazyLineCrop, lazy_crop_function
    seen = []
    fn = lazy_crop_function(lambda image, points: seen.append(np.asarray(points).shape) or "eager")
    img = np.zeros((20, 20, 3), np.uint8)
    assert fn(img, np.float32([[0, 0], [0.5, 0], [0.5, 9], [0, 9]])) == "eager"         # a crop width of 0: cv2 raises there
    assert fn(img.astype(np.float32), np.float32(QUADS["axis"])) == "eager"
    assert fn(img[:, :, 0], np.float32(QUADS["axis"])) == "eager"
    assert fn(img, np.float32(QUADS["axis"])[:3]) == "eager" and len(seen) == 4
    assert isinstance(fn(img, QUADS["axis"]), LazyLineCrop) and len(seen) == 4          # a list of points is taken


# ---------------------------------------------------------------------------------------------------------------- descriptor packing
def test_line_source_descriptors_against_a_numpy_restatement():
    from rapiddoc_amd.ocr_model import pack_line_sources
    from rapiddoc_amd.rec_plan import LINE_SOURCE_DTYPE
    assert LINE_SOURCE_DTYPE.itemsize == 112 and LINE_SOURCE_DTYPE.fields["m"][1] == 40 and LINE_SOURCE_DTYPE.fields["scratch_off"][1] == 32
    base, offsets, shapes = 0x7F0000001000, [0, 4800, 4816], [(40, 40), (1, 5), (7, 33)]
    source_of = [0, 2, 2, 1, 0]
    cw, ch = [30, 5, 0, 4, 17], [9, 11, 6, 1, 3]                                        # one crop without pixels
    mats = np.arange(45, dtype=np.float64).reshape(5, 9) / 7
    descs, offs, end = pack_line_sources(base, offsets, shapes, source_of, mats, cw, ch, 5520)
    want_off, at = [], 5520
    for w, h in zip(cw, ch):
        want_off.append(at)
        at += (3 * w * h + 15) // 16 * 16
    assert offs.tolist() == want_off == [5520, 6336, 6512, 6512, 6528] and end == at == 6688
    assert all(o % 16 == 0 for o in want_off) and want_off[2] == want_off[3]            # the empty crop takes no bytes
    assert descs.dtype == LINE_SOURCE_DTYPE and descs["scratch_off"].tolist() == want_off
    assert descs["src"].tolist() == [base + offsets[s] for s in source_of]
    assert descs["pitch"].tolist() == [3 * shapes[s][1] for s in source_of]
    assert descs["W"].tolist() == [shapes[s][1] for s in source_of] and descs["H"].tolist() == [shapes[s][0] for s in source_of]
    assert descs["crop_w"].tolist() == cw and descs["crop_h"].tolist() == ch and not descs["reserved"].any()
    assert np.array_equal(descs["m"], mats)
    raw = descs.tobytes()
    assert np.frombuffer(raw[112 + 40: 112 + 112], "<f8").tolist() == mats[1].tolist() and int.from_bytes(raw[:8], "little") == base


def test_plan_lines_is_what_plan_rec_ends_in():
    """the split of rec_plan.plan_rec: the same quads planned through `plan_lines` directly give the same descriptors"""
    from rapiddoc_amd import rec_plan as RP
    rng = np.random.default_rng(3)
    quads = []
    for _ in range(17):
        x0, y0, w, h = rng.uniform(0, 50), rng.uniform(0, 50), rng.uniform(8, 300), rng.uniform(8, 40)
        quads.append([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]])
    quads = np.asarray(quads)
    modes = dict(strict=True, two_stage=True, lines_in_launch=True, chunking="adaptive", rec_batch_num=6, rec_width_multiple=1, n_cu=256,
                 n_streams=2, host_native=False)
    a = RP.plan_rec([(1, [quads])], None, **modes)
    mats, cw, ch, ok = RP.quads_to_crop_matrices(quads)
    pooling = dict(n_img=[1], src_of=np.zeros(17, np.int32), page_of=np.zeros(17, np.int32), perm=None, n_all=17)
    b = RP.plan_lines(pooling, mats, cw, ch, (ch / cw >= 2.0).astype(np.int32), ok, None, 0, **modes)
    assert np.array_equal(a.descs, b.descs) and np.array_equal(a.order_all, b.order_all) and np.array_equal(a.line_w, b.line_w)
    assert [len(j) for j in a.warp_jobs] == [1] * len(a.batches) and b.warp_jobs == [[]] * len(b.batches) and b.swap_rb == a.swap_rb == 1
