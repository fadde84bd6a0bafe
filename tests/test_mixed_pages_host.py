"""CPU: the host side of page batches of mixed sizes - the `rd_preproc_resize_norm_sources` rows in the header, the library and
`_lib`, the 48-byte descriptor and its packer, every refusal of the entry (the checks read the HOST copy of the descriptors and
nothing is launched, so no GPU is needed), the grouping of pages by det shape, the page-list input rules and the uploader's
offset plan."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NAME = "rd_preproc_resize_norm_sources"


@pytest.fixture(scope="module")
def lib():
    from rapiddoc_amd import build as rd_build
    rd_build.build(verbose=False)
    from rapiddoc_amd import _lib
    return _lib.load()


def test_header_export_and_table_rows_exist(lib):
    from rapiddoc_amd import _lib
    header = (ROOT / "include" / "rapiddoc_mi355.h").read_text()
    assert re.search(r"^int " + NAME + r"\(int device_id, const rd_resize_source_desc\* descs_host, const rd_resize_source_desc\* descs_dev,", header, re.M)
    assert "typedef struct rd_resize_source_desc {" in header
    assert hasattr(lib, NAME) and NAME in _lib.SYMBOLS
    res, args = _lib.SYMBOLS[NAME]
    assert res is C.c_int and len(args) == 12 and args[10] is C.c_int64
    assert NAME in (ROOT / "tools" / "README.md").read_text()
    assert "kernels_resize_sources.hip" in __import__("rapiddoc_amd.build", fromlist=["SOURCES"]).SOURCES


def test_descriptor_layout_is_48_bytes_with_the_headers_field_order():
    from rapiddoc_amd.engine import RESIZE_SOURCE_DTYPE as D
    want = np.dtype({"names": ["src", "pitch", "out_off", "W", "H", "OW", "OH", "reserved"],
                     "formats": ["<u8", "<i8", "<i8", "<i4", "<i4", "<i4", "<i4", ("<i4", (2,))],
                     "offsets": [0, 8, 16, 24, 28, 32, 36, 40], "itemsize": 48})
    assert D.itemsize == 48 and D.names == want.names
    assert [D.fields[n][1] for n in D.names] == [0, 8, 16, 24, 28, 32, 36, 40]
    assert [D.fields[n][0] for n in D.names] == [want.fields[n][0] for n in want.names]
    # the struct as the header spells it, field by field
    body = re.search(r"typedef struct rd_resize_source_desc \{(.*?)\} rd_resize_source_desc;", (ROOT / "include" / "rapiddoc_mi355.h").read_text(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields == ["const uint8_t* src", "int64_t pitch", "int64_t out_off", "int32_t W, H, OW, OH", "int32_t reserved[2]"]
    assert 'static_assert(sizeof(rd_resize_source_desc) == 48' in (ROOT / "rapiddoc_amd" / "csrc" / "kernels_resize_sources.hip").read_text()


def test_packer_matches_a_numpy_restatement():
    from rapiddoc_amd.engine import RESIZE_SOURCE_DTYPE, pack_resize_sources
    ptrs, pitches = [0x7F0000001003, 4096, 2 ** 40 + 1], [3 * 53 + 11, 900, 3]
    hws, out_hws, offs = [(37, 53), (200, 300), (1, 1)], [(64, 96), (96, 64), (32, 32)], [3, 3 + 3 * 64 * 96 + 5, 10 ** 10]
    got = pack_resize_sources(ptrs, pitches, hws, out_hws, offs)
    assert got.dtype == RESIZE_SOURCE_DTYPE and got.shape == (3,)
    raw = np.frombuffer(got.tobytes(), dtype=np.uint8).reshape(3, 48)
    for k in range(3):
        want = (np.array([ptrs[k]], "<u8").tobytes() + np.array([pitches[k], offs[k]], "<i8").tobytes() +
                np.array([hws[k][1], hws[k][0], out_hws[k][1], out_hws[k][0], 0, 0], "<i4").tobytes())
        assert raw[k].tobytes() == want
    with pytest.raises(ValueError):
        pack_resize_sources(ptrs, pitches[:2], hws, out_hws, offs)


def test_every_refusal_returns_non_zero_with_a_message_and_nothing_is_launched(lib):
    """Fake non-NULL addresses throughout: a launch would fault (or, without a GPU, fail in the runtime with another message) - every
    case below must be turned away by the host checks before that."""
    from rapiddoc_amd.engine import pack_resize_sources
    good = dict(ptrs=[4096, 8192], pitches=[24, 24], hws=[(8, 8), (8, 8)], out_hws=[(4, 4), (4, 4)], out_offs=[0, 48])
    m, s = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)

    def refused(match, host=True, dev=True, out=True, n=None, interp=1, out_floats=96, **change):
        descs = pack_resize_sources(**{**good, **change})
        rc = lib.rd_preproc_resize_norm_sources(0, descs.ctypes.data if host else None, 0x10000 if dev else None, len(descs) if n is None else n,
                                                m, s, 1.0, interp, 0, 0x20000 if out else None, C.c_int64(out_floats), None)
        msg = lib.rd_create_error().decode()
        assert rc != 0 and msg.startswith(NAME + ": ") and match in msg, (match, rc, msg)

    refused("descriptors are NULL", host=False)
    refused("descriptors are NULL", dev=False)
    refused("out_dev is NULL", out=False)
    refused("n outside 1 .. 65535", n=0)
    refused("n outside 1 .. 65535", n=-3)
    refused("n outside 1 .. 65535", n=65536)
    refused("source 1: src is NULL", ptrs=[4096, 0])
    refused("source 1: pitch 23 is below 3 * W", pitches=[24, 23])
    refused("source 0: source size 8 x 0", hws=[(8, 0), (8, 8)])
    refused("source 1: source size 32769 x 8", hws=[(8, 8), (32769, 8)], pitches=[24, 24])
    refused("source 0: output size 0 x 4", out_hws=[(0, 4), (4, 4)])
    refused("source 1: output size 4 x 32769", out_hws=[(4, 4), (4, 32769)])
    refused("interp 0", interp=0)
    refused("interp 3", interp=3)
    refused("out_off -1 is negative", out_offs=[-1, 48])
    refused("overruns out_floats = 95", out_floats=95)                       # one float too far
    refused("overruns", out_offs=[0, 2 ** 63 - 1])                           # INT64_MAX: no sum that overflows
    refused("out_floats negative", out_floats=-1)
    refused("offsets 0 and 47 overlap", out_offs=[0, 47])
    refused("offsets 48 and 95 overlap", out_offs=[95, 48], out_floats=200)  # in either order
    refused("offsets 7 and 7 overlap", out_offs=[7, 7])


def test_pages_are_grouped_by_det_shape_in_order_of_first_appearance():
    from rapiddoc_amd import ocr_host
    from rapiddoc_amd.pipeline import DET_LIMIT, group_pages_by_det_shape, page_det_shape
    hws = [(200, 140), (140, 200), (200, 140), (120, 260), (140, 200)]
    shapes, groups, inverse = group_pages_by_det_shape(hws)
    assert shapes == [(320, 256), (256, 320), (320, 256), (256, 384), (256, 320)]
    assert groups == [((320, 256), [0, 2]), ((256, 320), [1, 4]), ((256, 384), [3])]
    grouped = [i for _s, members in groups for i in members]
    assert grouped == [0, 2, 1, 4, 3] and [grouped[k] for k in inverse.tolist()] == list(range(5))
    # the rule is det_preprocess's: 64-px bucket of the page with its margins, then the limit of 960 on the longer side
    for h, w in hws + [(1684, 1191), (1191, 1684), (3000, 400), (1, 1)]:
        bh, bw = -(-(h + 100) // 64) * 64, -(-(w + 100) // 64) * 64
        assert page_det_shape(h, w) == ocr_host.det_resize_shape(bh, bw, DET_LIMIT, "max")
    assert page_det_shape(1684, 1191) == (960, 704) and max(page_det_shape(3000, 400)) == 960
    one, groups1, inv1 = group_pages_by_det_shape([(1684, 1191)] * 4)
    assert groups1 == [((960, 704), [0, 1, 2, 3])] and inv1.tolist() == [0, 1, 2, 3]
    # pages of different sizes may share a det shape: they ride in one group
    assert group_pages_by_det_shape([(200, 140), (210, 150)])[1] == [((320, 256), [0, 1])]


def test_page_list_rules():
    from rapiddoc_amd.pipeline import split_page_list
    a, b = np.zeros((20, 30, 3), np.uint8), np.zeros((31, 17, 3), np.uint8)
    kind, arrs = split_page_list([a, torch.from_numpy(b), b[:, 2:9]])
    assert kind == "host" and [x.shape for x in arrs] == [(20, 30, 3), (31, 17, 3), (31, 7, 3)] and all(isinstance(x, np.ndarray) for x in arrs)
    assert arrs[2].base is not None and arrs[2].strides[0] == 51             # a window stays a view: the pack gathers its rows
    meta = torch.empty((20, 30, 3), dtype=torch.uint8, device="meta")

    class OnDevice(torch.Tensor):                                            # a stand-in that says it lies on the GPU
        is_cuda = True
    dev = torch.Tensor._make_subclass(OnDevice, torch.zeros((4, 5, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="mix"):
        split_page_list([dev, a])
    with pytest.raises(ValueError, match="mix"):
        split_page_list([a, dev, a])
    for bad, match in (([], "at least one"), ([np.zeros((4, 5), np.uint8)], r"\[H, W, 3\]"), ([np.zeros((4, 5, 4), np.uint8)], r"\[H, W, 3\]"),
                       ([np.zeros((4, 5, 3), np.float32)], "uint8"), ([torch.zeros((4, 5, 3))], "uint8"), ([np.zeros((0, 5, 3), np.uint8)], r"\[H, W, 3\]")):
        with pytest.raises(ValueError, match=match):
            split_page_list(bad)
    del meta


def test_page_uploader_plans_a_list_with_aligned_page_starts():
    from rapiddoc_amd.host_stage import plan_offsets
    from rapiddoc_amd.pipeline import PageUploader
    shapes = [(200, 140), (140, 200), (1, 1), (120, 260), (7, 5)]
    offs, total = PageUploader.plan_list(shapes)
    assert (offs, total) == plan_offsets(shapes)
    assert offs[0] == 0 and all(o % 16 == 0 for o in offs) and total % 16 == 0
    for (h, w), o, nxt in zip(shapes, offs, offs[1:] + [total]):
        assert 0 <= nxt - (o + 3 * h * w) < 16                               # no overlap, less than one alignment unit of padding


def test_lines_name_their_sources_keeps_every_crop_in_place():
    """the recogniser plan of a list call: one source per page, then every line names its page (host arithmetic only)"""
    from rapiddoc_amd.pipeline import boxes_to_quads, lines_name_their_sources
    from rapiddoc_amd.rec_plan import LINE_SOURCE_DTYPE, plan_rec
    quads = [boxes_to_quads(np.float32([[8, 16, 70, 28], [8, 60, 130, 72]])), np.zeros((0, 4, 2), np.float32),
             boxes_to_quads(np.float32([[8, 14, 190, 26], [8, 44, 90, 56], [8, 74, 150, 86]]))]
    hws, views = [(200, 140), (140, 200), (120, 260)], [(0x1000, 3 * 140), (0x2000, 3 * 200 + 5), (0x3001, 3 * 260)]
    modes = dict(strict=True, two_stage=True, lines_in_launch=True, chunking="adaptive", rec_batch_num=6, rec_width_multiple=1, n_cu=256, n_streams=2,
                 host_native=False)
    plan = plan_rec([(1, [q]) for q in quads], [[k] for k in range(3)], **modes)
    before = plan.descs.copy()
    base = np.repeat(np.asarray(plan.batch_base[:-1]), np.diff(plan.starts))
    total = plan.scratch_bytes
    lines_name_their_sources(plan, views, hws)
    sd = plan.src_descs
    assert sd.dtype == LINE_SOURCE_DTYPE and len(sd) == 5 and plan.src_scratch_bytes == total and plan.scratch_bytes == 0
    src = plan.src_of[plan.line_ids]
    assert sorted(src.tolist()) == [0, 0, 2, 2, 2]
    assert sd["src"].tolist() == [views[s][0] for s in src] and sd["pitch"].tolist() == [views[s][1] for s in src]
    assert sd["H"].tolist() == [hws[s][0] for s in src] and sd["W"].tolist() == [hws[s][1] for s in src]
    assert (plan.descs["scratch_off"] == before["scratch_off"] + base).all() and (sd["scratch_off"] == plan.descs["scratch_off"]).all()
    assert (sd["m"] == before["m"]).all() and (sd["crop_w"] == before["crop_w"]).all() and (sd["crop_h"] == before["crop_h"]).all()
    assert plan.warp_jobs == [[] for _ in plan.batches] and sum(c for _f, c in plan.src_jobs) == 5
    assert [f for f, _c in plan.src_jobs] == plan.starts[:-1].tolist()
    ends = sd["scratch_off"].astype(np.int64) + 3 * sd["crop_w"].astype(np.int64) * sd["crop_h"]
    assert ends.max() <= total and len(set(sd["scratch_off"].tolist())) == 5
