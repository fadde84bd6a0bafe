"""GPU: the OCR-model seam (rapiddoc_amd/ocr_model.py) and its kernel.  `Mi355RapidOcrModel` with synthetic `ppocrv6_det` /
`ppocrv6_rec` weights against the project's existing routes for the same pixels - `RegionOcr`'s raw group detection, the reference's
chunk-of-6 recogniser loop through `Mi355RecSession`, `TableOcr` - and `rd_line_warp_sources` (csrc/kernels_image.hip) byte for byte
against `rd_line_warp_batch` run once per source.  Equalities, except the one score bound that is named where it is used."""
import sys
import types

import numpy as np
import pytest
import torch

from kind_helpers import synth_state
from rapiddoc_amd import _lib, ocr_host
from rapiddoc_amd.pages import synth_page
from rapiddoc_amd.rec_plan import LINE_DTYPE, LINE_SOURCE_DTYPE, quads_to_crop_matrices

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5


@pytest.fixture(scope="module")
def pipe(golden_dir):
    from rapiddoc_amd.pipeline import PagePipeline
    return PagePipeline({k: synth_state(golden_dir, k) for k in ("ppocrv6_det", "ppocrv6_rec")}, n_rec_streams=2)


@pytest.fixture(scope="module")
def ink():
    """the textured text lines of one synthetic page (pages.synth_batch's recipe), to be pasted where a test wants text"""
    page, boxes = synth_page(5)
    return [page[int(y0): int(y1), int(x0): int(x1)] for x0, y0, x1, y1 in boxes]


def _canvas(ink, h, w, boxes, first=0):
    """a white BGR canvas with a text line in every (x0, y0, x1, y1) box"""
    img = np.full((h, w, 3), 255, np.uint8)
    for k, (x0, y0, x1, y1) in enumerate(boxes):
        line = ink[(first + k) % len(ink)]
        reps = (-(-(y1 - y0) // line.shape[0]), -(-(x1 - x0) // line.shape[1]), 1)
        img[y0:y1, x0:x1] = np.tile(line, reps)[: y1 - y0, : x1 - x0]
    return img


def _maps_fn(boxes_by_size, device):
    """det_maps_fn of a model: rendered maps of the known boxes of every image of a size group"""
    from rapiddoc_amd.pipeline import render_text_maps
    return lambda hw, dhw, first, n: render_text_maps([np.float32(b) for b in boxes_by_size[hw][first: first + n]], hw, dhw, device)


def _device_crops(img_bgr, boxes):
    """the eager crops of `boxes` from a BGR image: the project's existing device warp (rd_line_warp_batch), downloaded, tall crops
    turned by np.rot90 - the arrays an unmodified RapidDoc would hold, made without cv2"""
    lib = _lib.load()
    mats, cw, ch, ok = quads_to_crop_matrices(np.float32(boxes))
    assert ok.all()
    descs = np.zeros(len(boxes), LINE_DTYPE)
    descs["crop_w"], descs["crop_h"], descs["m"] = cw, ch, mats
    size = (3 * descs["crop_w"].astype(np.int64) * descs["crop_h"] + 15) // 16 * 16
    descs["scratch_off"] = np.cumsum(size) - size
    src = torch.from_numpy(np.ascontiguousarray(img_bgr)).cuda()[None]
    scratch = torch.zeros(int(size.sum()), dtype=torch.uint8, device="cuda")
    descs_dev = torch.from_numpy(descs.view(np.uint8)).cuda()
    px = int((descs["crop_w"].astype(np.int64) * descs["crop_h"]).max())
    assert lib.rd_line_warp_batch(0, src.data_ptr(), 1, src.shape[1], src.shape[2], descs_dev.data_ptr(), len(descs), px, scratch.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream) == 0
    host = scratch.cpu().numpy()
    out = []
    for d in descs:
        crop = host[d["scratch_off"]: d["scratch_off"] + 3 * d["crop_w"] * d["crop_h"]].reshape(d["crop_h"], d["crop_w"], 3)
        out.append(np.ascontiguousarray(np.rot90(crop)) if d["crop_h"] / d["crop_w"] >= 2 else crop.copy())
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. det_batch_predict
def test_det_batch_predict_is_region_ocrs_group_detection(pipe, ink, monkeypatch):
    from rapiddoc_amd import ocr_model
    from rapiddoc_amd.analyze import RegionOcr
    from rapiddoc_amd.pipeline import render_text_maps
    small = [[(8, 6, 118, 30)], [(4, 4, 90, 28), (10, 34, 120, 60)], []]                       # 64 x 128: the third canvas is blank
    large = [[(10, 10, 180, 40), (12, 50, 150, 78), (20, 90, 170, 120)], [(6, 20, 186, 50)]]   # 128 x 192
    sizes = {(64, 128): small, (128, 192): large}
    imgs = [_canvas(ink, 64, 128, small[0]), _canvas(ink, 128, 192, large[0], 3), _canvas(ink, 64, 128, small[1], 1),
            _canvas(ink, 128, 192, large[1], 6), _canvas(ink, 64, 128, small[2])]              # the two size groups interleaved
    where = [((64, 128), 0), ((128, 192), 0), ((64, 128), 1), ((128, 192), 1), ((64, 128), 2)]
    model = ocr_model.Mi355RapidOcrModel(pipe)
    model.det_maps_fn = _maps_fn(sizes, pipe.tdev)
    assert model.det_batch_predict([]) == []
    uploads = model._stage.uploads if model._stage else 0
    got = model.det_batch_predict(imgs, 8)
    assert model._stage.uploads == uploads + 1                                                  # one pack, one copy for the whole list
    region = RegionOcr(pipe, box_thresh=0.5, unclip_ratio=1.8)
    n_found = 0
    for hw, boxes in sizes.items():
        members = [i for i, (s, _k) in enumerate(where) if s == hw]
        canv = torch.from_numpy(np.stack([imgs[i][:, :, ::-1] for i in members]).copy()).cuda()       # RGB, as RegionOcr takes them
        maps = render_text_maps([np.float32(b) for b in boxes], hw, ocr_host.det_resize_shape(*hw, 960, "max"), pipe.tdev)
        for i, want in zip(members, region._detect_group(canv, maps, pipe)):
            boxes_i, elapse = got[i]
            assert elapse >= 0
            if len(want) == 0:
                assert boxes_i is None                                                          # rapidocr's value for "nothing found"
            else:
                assert boxes_i.dtype == np.float32 and boxes_i.shape == (len(want), 4, 2) and np.array_equal(boxes_i, want)
                n_found += len(want)
    assert got[4][0] is None and n_found == 7                                                   # every drawn line was found
    # the result of an image does not depend on max_batch_size - nor on where the engine cuts its launches
    for bs, launch in ((1, ocr_model.DET_LAUNCH), (8, 2), (3, 1)):
        monkeypatch.setattr(ocr_model, "DET_LAUNCH", launch)
        again = model.det_batch_predict(imgs, bs)
        assert all((a[0] is None and b[0] is None) or np.array_equal(a[0], b[0]) for a, b in zip(got, again))


# ---------------------------------------------------------------------------------------------------------------- 2. pooled rec
@pytest.fixture(scope="module")
def crops13():
    """13 BGR crops - three chunks of six with a ragged tail: heights 20 .. 60, w / h from far below to well above 320 / 48, one crop a
    single pixel wide, the caller's order unrelated to the aspect order"""
    rng = np.random.default_rng(7)
    hw = [(48, 320), (20, 1), (60, 90), (32, 600), (24, 31), (40, 267), (57, 1100), (33, 220), (48, 321), (21, 500), (60, 401), (30, 75), (26, 890)]
    out = []
    for h, w in hw:
        c = rng.integers(0, 61, (h, w, 1), dtype=np.uint8).repeat(3, axis=2) + rng.integers(0, 3, (h, w, 3), dtype=np.uint8)     # (channels differ)
        for x in range(0, w, 9):
            c[:, x: x + 4] = 255 - c[:, x: x + 4] // 4
        out.append(c)
    return out


def test_pooled_rec_is_the_reference_chunk_loop_through_the_session(pipe, crops13, golden_dir):
    """`ocr(crops, det=False)` against rapid_ocr.py:404-472 restated over Mi355RecSession: argsort by w / h, chunks of six, every chunk
    resized and padded to int(48 * max ratio) on the HOST (oracle/cv2_ops.resize_norm_img), one session call per chunk, CTC decode on the
    host.  Strings are equal; scores are compared exactly first, and where they are not bit-equal they meet the bound of
    tests/test_gpu_s2_dropin.py::test_the_reference_chunk_loop_through_the_session_gives_the_fast_path_strings (the project's strict-
    versus-chunk comparison): printed to three places (analyze_utils.py:280), at most one unit of the third place apart."""
    from oracle import cv2_ops
    from rapiddoc_amd.ocr_model import Mi355RapidOcrModel
    from rapiddoc_amd.session import Mi355RecSession
    model = Mi355RapidOcrModel(pipe)
    got = model.ocr(crops13, det=False, tqdm_enable=True)
    assert isinstance(got, list) and len(got) == 1 and len(got[0]) == 13 and all(isinstance(r, tuple) and len(r) == 2 for r in got[0])
    assert model.stats["warp_source_launches"] == 0                        # eager crops are read where they were uploaded: nothing is warped
    sess = Mi355RecSession(synth_state(golden_dir, "ppocrv6_rec"))
    ratios = np.array([c.shape[1] / float(c.shape[0]) for c in crops13])
    indices = np.argsort(ratios)
    want = [None] * 13
    for beg in range(0, 13, 6):
        idxs = [int(i) for i in indices[beg: beg + 6]]
        max_wh_ratio = max(320 / 48, max(ratios[i] for i in idxs))
        batch = np.stack([cv2_ops.resize_norm_img(crops13[i], max_wh_ratio) for i in idxs]).astype(np.float32)
        preds = sess(batch)
        for r, ts in enumerate(ocr_host.ctc_decode(preds.argmax(axis=2), preds.max(axis=2), pipe.characters)):
            want[idxs[r]] = ts
    assert [t for t, _s in got[0]] == [t for t, _s in want]                 # the caller's order, the reference's strings
    assert any(t for t, _s in want)
    diff = max(abs(a[1] - b[1]) for a, b in zip(got[0], want))
    print("pooled rec: largest score difference to the chunk loop %.3g (%s)" % (diff, "bit-equal" if diff == 0 else "not bit-equal"))
    if diff != 0:
        assert max(abs(ocr_host.format_score(a[1]) - ocr_host.format_score(b[1])) for a, b in zip(got[0], want)) <= 1e-3 + 1e-9
    # a call of one crop is that crop's entry of the pooled call wherever the crop defines its chunk's width (a line's result depends on
    # its padded width): the widest line of every chunk - alone it is padded to the same width
    for widest in (int(indices[5]), int(indices[11]), int(indices[12])):
        assert model.ocr([crops13[widest]], det=False) == [[got[0][widest]]]
    assert model.ocr(crops13[widest], det=False) == [[got[0][widest]]]     # a bare array is a list of one
    # inputs the host normalises: a non-contiguous view and a grey image give what their contiguous three-channel forms give
    wide = np.ascontiguousarray(np.concatenate([crops13[3], crops13[3]], axis=1))
    assert model.ocr([wide[:, :600]], det=False) == model.ocr([crops13[3]], det=False)
    grey = crops13[5][:, :, 0]
    assert model.ocr([grey], det=False) == model.ocr([np.repeat(grey[:, :, None], 3, axis=2)], det=False)
    assert model.ocr([], det=False) == [[]]


# ---------------------------------------------------------------------------------------------------------------- 3. table forms
def test_table_forms_are_table_ocrs(pipe, ink):
    from rapiddoc_amd import table_host
    from rapiddoc_amd.analyze import TableOcr
    from rapiddoc_amd.ocr_model import Mi355RapidOcrModel, lazy_crop_function
    boxes = [(12, 10, 300, 38), (12, 50, 140, 76), (190, 50, 310, 76), (20, 92, 280, 122), (14, 134, 200, 160)]
    img = _canvas(ink, 176, 320, boxes)
    mfd = [{"bbox": [150, 8, 200, 40], "latex": "x^2"}]                      # a formula inside the first line's box: the box is cut in two
    img[8:40, 150:200] = 255                                                 # (white already, so the detector's masked copy is this image)
    model = Mi355RapidOcrModel(pipe, det_db_box_thresh=0.5, det_db_unclip_ratio=1.6, enable_merge_det_boxes=False)      # the table stage's model
    model.det_maps_fn = _maps_fn({(176, 320): [boxes], (64, 128): [[]]}, pipe.tdev)
    table = torch.from_numpy(img[:, :, ::-1].copy()).cuda()
    maps = model.det_maps_fn((176, 320), ocr_host.det_resize_shape(176, 320, 960, "max"), 0, 1)
    line_level = TableOcr(pipe, use_word_box=False, compose="host").ocr_result(table, mfd, maps)
    quads, texts, scores = line_level
    assert len(quads) == 6                                                   # five lines, the first cut around the formula
    # ocr(img, mfd_res, rec=False)[0]: the boxes
    det_only = model.ocr(img, mfd_res=mfd, rec=False)[0]
    assert isinstance(det_only, list) and np.array_equal(np.float32(det_only), np.stack(quads))
    # ocr(img, mfd_res)[0]: [[box, (text, score)]] of the lines at or above drop_score
    model.drop_score = 0.0
    everything = model.ocr(img, mfd_res=mfd)[0]
    assert [table_host.normalize_table_ocr_text(t) for _b, (t, _s) in everything] == texts
    assert [ocr_host.format_score(s) for _b, (_t, s) in everything] == scores and np.array_equal(np.float32([b for b, _r in everything]), np.stack(quads))
    # the lines of this form are cut from the uploaded image into a scratch of the model's own: nothing behind the upload is written
    model._stage.upload([np.zeros((200, 400, 3), np.uint8)])                  # (a larger upload first: the stage's buffer now has room behind this image)
    model._stage.release()
    stage_dev, used = model._stage._dev, 16 * ((3 * 176 * 320 + 15) // 16)
    assert stage_dev.numel() >= used + 4096
    torch.cuda.synchronize()
    stage_dev[used:] = FILL
    assert model.ocr(img, mfd_res=mfd)[0] == everything and stage_dev is model._stage._dev
    assert bool((stage_dev[used:] == FILL).all())
    model.drop_score = 0.5
    kept = [e for e in everything if e[1][1] >= 0.5]
    print("table forms: %d of %d lines at or above drop_score" % (len(kept), len(everything)))
    assert model.ocr(img, mfd_res=mfd)[0] == (kept or None)
    raw_scores = sorted(s for _b, (_t, s) in everything)
    model.drop_score = raw_scores[len(raw_scores) // 2]                      # a threshold that certainly splits the list
    assert model.ocr(img, mfd_res=mfd)[0] == [e for e in everything if e[1][1] >= model.drop_score]
    model.drop_score = 0.5
    blank = np.full((64, 128, 3), 255, np.uint8)                             # nothing detected: the reference's None, in both forms
    assert model.ocr(blank, rec=False) == [None] and model.ocr(blank, mfd_res=mfd) == [None] and model(blank) == (None, None)
    # the word-box form, driven as _run_table_ocr drives it (analyze_utils.py:476-539), with lazy crops
    crop = lazy_crop_function(lambda image, points: pytest.fail("a lazy crop was cut on the host"))
    crops = [crop(img, np.asarray(b, dtype=np.float32)) for b in det_only]
    res = model.ocr(crops, det=False, tqdm_enable=False, return_word_box=True, ori_img=img, dt_boxes=det_only)[0]
    flat = [[w[2], table_host.normalize_table_ocr_text(w[0]), w[1]] for _c, r in zip(crops, res) for w in r[2]]
    mine = [list(x) for x in zip(*flat)] if flat else []
    theirs = TableOcr(pipe, use_word_box=True, compose="host").ocr_result(table, mfd, maps)
    print("table forms: %d word entries" % len(flat))
    assert mine == theirs
    assert model.stats["warp_source_launches"] == model.stats["rec_batches"] >= 1


# ---------------------------------------------------------------------------------------------------------------- 4. the kernel alone
def _warp_case():
    """9 lines from 3 sources: A 37 x 53, B one pixel high, C a 23 x 29 window with a padded pitch at an odd byte address of a larger
    buffer.  -> (source arrays as the kernel sees them, [(source, crop_w, crop_h, m)])"""
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (1, 40, 3), dtype=np.uint8)
    c = rng.integers(0, 256, (23, 29, 3), dtype=np.uint8)

    def quad(q):
        m, cw, ch, ok = quads_to_crop_matrices(np.float32([q]))
        assert ok[0]
        return int(cw[0]), int(ch[0]), m[0]
    lines = [(0, *quad([[-7, 5], [30, 5], [30, 20], [-7, 20]])),                   # overhangs the left border
             (0, *quad([[30, 3], [61, 6], [60, 18], [29, 15]])),                   # the right one, tilted
             (0, *quad([[5, -9], [45, -9], [45, 8], [5, 8]])),                     # the top
             (0, *quad([[8, 25], [44, 27], [43, 44], [7, 42]])),                   # the bottom
             (1, *quad([[2, -3], [38, -3], [38, 4], [2, 4]])),                     # the one-pixel-high source: every row is row 0
             (1, *quad([[-4, 0], [44, 0], [44, 1], [-4, 1]])),
             (2, *quad([[3, 2], [27.5, 4.25], [26, 20], [1.5, 17.75]])),
             (2, 11, 7, np.array([0.5, 0.1, 3.0, 0.0, 1.0, 2.0, 0.0, 0.0, 0.0])),  # a degenerate homography: w = 0 everywhere
             (0, 300, 230, np.array([53 / 300, 0, -0.5, 0, 37 / 230, -0.5, 0, 0, 1.0]))]      # 69000 pixels: more than one grid pass (65536)
    return [a, b, c], lines


def test_rd_line_warp_sources_is_rd_line_warp_batch_byte_for_byte():
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    (a, b, c), lines = _warp_case()
    pitch_c, lead = 3 * 29 + 5, 7
    big = torch.full((lead + 23 * pitch_c + 64,), 0x3C, dtype=torch.uint8, device="cuda")
    big[lead: lead + 23 * pitch_c].view(23, pitch_c)[:, : 3 * 29] = torch.from_numpy(c.reshape(23, -1)).cuda()
    dev = [torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(c).cuda()]         # C's packed copy: the comparison's source
    srcs = [(dev[0].data_ptr(), 3 * 53, 53, 37), (dev[1].data_ptr(), 3 * 40, 40, 1), (big.data_ptr() + lead, pitch_c, 29, 23)]
    assert srcs[2][0] % 2 == 1
    offs, at = [], GUARD                                                          # 64 guard bytes in front of, between and behind the crops
    for _s, cw, ch, _m in lines:
        offs.append(at)
        at += (3 * cw * ch + 15) // 16 * 16 + GUARD
    total = at
    sd = np.zeros(len(lines), LINE_SOURCE_DTYPE)
    ld = np.zeros(len(lines), LINE_DTYPE)
    for k, (s, cw, ch, m) in enumerate(lines):
        sd[k] = (srcs[s][0], srcs[s][1], srcs[s][2], srcs[s][3], cw, ch, offs[k], 0, m)
        ld[k] = (0, 0, cw, ch, 0, offs[k], m)
    got = torch.full((total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    want = torch.full((total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    sd_dev = torch.from_numpy(sd.view(np.uint8)).cuda()
    assert lib.rd_line_warp_sources(0, sd.ctypes.data, sd_dev.data_ptr(), len(sd), got.data_ptr(), total, stream) == 0, lib.rd_create_error()
    ld_dev = torch.from_numpy(ld.view(np.uint8)).cuda()
    for s in range(3):                                                            # the existing route: one launch per source
        ks = [k for k, ln in enumerate(lines) if ln[0] == s]
        part = torch.from_numpy(np.ascontiguousarray(ld[ks]).view(np.uint8)).cuda()
        px = max(lines[k][1] * lines[k][2] for k in ks)
        assert lib.rd_line_warp_batch(0, dev[s].data_ptr(), 1, dev[s].shape[0], dev[s].shape[1], part.data_ptr(), len(ks), px, want.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    g, w = got.cpu().numpy(), want.cpu().numpy()
    written = np.zeros(total + GUARD, bool)
    for k, (_s, cw, ch, _m) in enumerate(lines):
        n = 3 * cw * ch
        assert np.array_equal(g[offs[k]: offs[k] + n], w[offs[k]: offs[k] + n]), f"line {k}"
        assert (g[offs[k]: offs[k] + n] != FILL).any()
        written[offs[k]: offs[k] + n] = True
    assert (g[~written] == FILL).all() and (w[~written] == FILL).all() and (~written).sum() >= GUARD * (len(lines) + 1)
    assert (big.cpu().numpy()[:lead] == 0x3C).all()                               # (the sources are read only)
    # refused descriptors: a non-zero return, the message, nothing launched - the guard pattern of a fresh buffer stays whole
    fresh = torch.full((total + GUARD,), FILL, dtype=torch.uint8, device="cuda")

    def refused(descs, n=None, host=True, dev_ptr=True, scratch=True, scratch_bytes=total, match="rd_line_warp_sources"):
        d_dev = torch.from_numpy(np.ascontiguousarray(descs).view(np.uint8)).cuda()
        rc = lib.rd_line_warp_sources(0, descs.ctypes.data if host else None, d_dev.data_ptr() if dev_ptr else None, len(descs) if n is None else n,
                                      fresh.data_ptr() if scratch else None, scratch_bytes, stream)
        assert rc != 0 and match.encode() in lib.rd_create_error(), (rc, lib.rd_create_error())

    def changed(**kw):
        d = sd.copy()
        for name, v in kw.items():
            d[name][3] = v
        return d
    refused(sd, host=False, match="NULL")
    refused(sd, dev_ptr=False, match="NULL")
    refused(sd, scratch=False, match="scratch")
    refused(sd, n=0, match="n outside")
    refused(sd, n=65536, match="n outside")
    refused(changed(src=0), match="line 3: src is NULL")
    refused(changed(pitch=3 * 53 - 1), match="line 3: pitch")
    refused(changed(W=0), match="line 3: source size")
    refused(changed(H=-2), match="line 3: source size")
    refused(changed(crop_w=0), match="line 3: crop size")
    refused(changed(crop_h=-1), match="line 3: crop size")
    refused(changed(scratch_off=-16), match="line 3: crop of")
    refused(sd, scratch_bytes=offs[-1] + 3 * 300 * 230 - 1, match="line 8: crop of")       # the last crop overruns by one byte
    torch.cuda.synchronize()
    assert (fresh.cpu().numpy() == FILL).all()


# ---------------------------------------------------------------------------------------------------------------- 5. lazy route end to end
def test_lazy_crops_give_what_the_eager_arrays_give(pipe, ink):
    """The shape of get_ocr_result_list (utils/ocr_utils.py:361-432) over 5 region images of 3 sizes: one copy of the region per region,
    one crop per box.  The eager arrays are the project's existing device warp of the same boxes, downloaded - the same bytes on both
    sides, so no dependence on cv2."""
    from rapiddoc_amd.ocr_model import LazyLineCrop, Mi355RapidOcrModel, lazy_crop_function
    regions = [(64, 192, [(6, 4, 180, 30), (8, 34, 120, 60)]),
               (128, 256, [(10, 8, 240, 40), (12, 48, 200, 76), (-3, 84, 128, 110), (200, 20, 212, 120)]),      # one overhangs, one is tall
               (64, 192, [(4, 6, 60, 28), (70, 6, 188, 28), (10, 36, 150, 62)]),
               (96, 320, [(8, 8, 310, 44), (20, 52, 180, 84)]),
               (128, 256, [(16, 16, 250, 46), (16, 60.5, 120.25, 90), (130, 58, 255, 92)])]
    lazy_fn = lazy_crop_function(lambda image, points: pytest.fail("a lazy crop was cut on the host"))
    lazy, eager = [], []
    for k, (h, w, boxes) in enumerate(regions):
        ori_im = _canvas(ink, h, w, [tuple(int(max(v, 0)) for v in b) for b in boxes], k).copy()      # `ori_im = bgr_image.copy()`, once per region
        quads = [np.float32([[x0, y0], [x1, y0], [x1, y1], [x0, y1]]) for x0, y0, x1, y1 in boxes]
        lazy += [lazy_fn(ori_im, q) for q in quads]
        eager += _device_crops(ori_im, quads)
    assert len(lazy) == 14 and all(isinstance(c, LazyLineCrop) for c in lazy) and [c.shape for c in lazy] == [c.shape for c in eager]
    assert lazy[5].shape == (12, 100, 3)                                        # the tall box: np.rot90's shape
    model = Mi355RapidOcrModel(pipe)
    want = model.ocr(eager, det=False)[0]
    assert any(t for t, _s in want) and model.stats["warp_source_launches"] == 0
    uploads = model._stage.uploads
    got = model.ocr(lazy, det=False)[0]
    assert got == want                                                           # strings and scores, exactly
    staged, what = model.last_staged
    assert model._stage.uploads == uploads + 1 and len(staged.shapes) == 5 == len(what["sources"]) and what["eager"] == []      # every source once
    assert model.stats["warp_source_launches"] == model.stats["rec_batches"] < 5       # one warp launch per rec launch, not one per source
    assert not any(c.materialized for c in lazy)
    # a mixed list, in another order
    order = [9, 0, 13, 4, 5, 2, 11, 7, 1, 12, 3, 10, 6, 8]
    mixed = [lazy[i] if j % 2 else eager[i] for j, i in enumerate(order)]
    assert model.ocr(mixed, det=False)[0] == [want[i] for i in order]
    staged, what = model.last_staged
    assert len(what["eager"]) == 7 and len(staged.shapes) == 7 + len(what["sources"]) and len(what["sources"]) <= 5
    # a lazy crop somebody looked at is an eager array from then on
    looked = lazy_crop_function(lambda image, points: eager[0])(lazy[0].source, lazy[0].points)
    assert np.asarray(looked) is eager[0] and model.ocr([looked], det=False) == model.ocr([eager[0]], det=False)


# ---------------------------------------------------------------------------------------------------------------- 6. through the plugin
def test_the_installed_factory_answers_the_five_call_forms(pipe, ink, monkeypatch):
    from rapiddoc_amd import plugin
    from rapiddoc_amd.ocr_model import LazyLineCrop, Mi355RapidOcrModel
    names = ("rapid_doc", "rapid_doc.backend", "rapid_doc.backend.pipeline", "rapid_doc.backend.pipeline.model_init", "rapid_doc.utils",
             "rapid_doc.utils.ocr_utils", "rapid_doc.backend.pipeline.analyze_utils")
    mods = {name: types.ModuleType(name) for name in names}
    init, utils = mods["rapid_doc.backend.pipeline.model_init"], mods["rapid_doc.utils.ocr_utils"]
    init.ocr_model_init = lambda *a, **k: "reference model"
    utils.get_rotate_crop_image = mods["rapid_doc.backend.pipeline.analyze_utils"].get_rotate_crop_image = lambda img, points: pytest.fail("host crop")
    for name, mod in mods.items():
        monkeypatch.setitem(sys.modules, name, mod)
    uninstall = plugin.install_ocr_model({"ch": pipe}, device_crops=True, module=init)
    try:
        model = init.ocr_model_init(0.3, "ch", {"use_det_mode": "auto"}, 1.8, True, False)
        assert isinstance(model, Mi355RapidOcrModel) and init.ocr_model_init(0.6, "ch", None, 0.5, False, True) == "reference model"
        boxes = [(8, 6, 118, 30), (10, 34, 120, 60)]
        img = _canvas(ink, 64, 128, boxes)
        model.det_maps_fn = _maps_fn({(64, 128): [boxes, boxes]}, pipe.tdev)
        (det_boxes, _e), (det_boxes2, _e2) = model.det_batch_predict([img, img], 2)                       # form 1
        assert det_boxes.shape == (2, 4, 2) and np.array_equal(det_boxes, det_boxes2)
        only = model.ocr(img, mfd_res=None, rec=False)[0]                                                   # form 3
        assert len(only) >= 1 and all(np.float32(b).shape == (4, 2) for b in only)
        model.drop_score = 0.0
        both = model.ocr(img, mfd_res=[])[0]                                                                # form 4
        assert [b for b, _r in both] == only and all(isinstance(t, str) and isinstance(s, float) for _b, (t, s) in both)
        crops = [utils.get_rotate_crop_image(img, np.float32(b)) for b in only]
        assert all(isinstance(c, LazyLineCrop) for c in crops)
        lines = model.ocr(crops, det=False, tqdm_enable=True)[0]                                            # form 2
        assert lines == [r for _b, r in both]                                                               # the same lines, cut from the same image
        words = model.ocr(crops, det=False, return_word_box=True, ori_img=img, dt_boxes=only)[0]           # form 5
        assert len(words) <= len(lines) and all(len(w) == 3 and isinstance(w[2], tuple) for w in words)
    finally:
        uninstall()
    assert init.ocr_model_init("x") == "reference model"
