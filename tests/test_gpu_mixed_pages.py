"""GPU: page batches of mixed page sizes.  `rd_preproc_resize_norm_sources` (csrc/kernels_resize_sources.hip) bit for bit against
`rd_preproc_resize_norm` on a contiguous copy of every source, with guard floats around every destination slot; `PagePipeline.run_batch`
on a LIST of pages (det groups, one pooled strict recogniser plan, one warp launch per rec launch, host lists, `PageUploader` lists,
prefetch); the one-launch routes of `LayoutModel.preprocess` and `Mi355UniTableStructure(resize="linear")` against their loops."""
import ctypes as C

import numpy as np
import pytest
import torch

import unitable_reference as R
from rapiddoc_amd import ocr_host, weights as W

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GUARD = 5
DET_NORM = dict(mean=ocr_host.DET_MEAN, std=ocr_host.DET_STD, scale=1.0 / 255.0)
RAW_NORM = dict(mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), scale=1.0)


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _window(rng, H, W, pitch, odd_offset):
    """a [H, W, 3] view with rows `pitch` bytes apart that starts `odd_offset` bytes into its buffer"""
    buf = torch.from_numpy(rng.integers(0, 256, odd_offset + H * pitch + 7, dtype=np.uint8)).cuda()
    return torch.as_strided(buf, (H, W, 3), (pitch, 3, 1), storage_offset=odd_offset)


@pytest.fixture(scope="module")
def kernel_sources():
    """[(source tensor, (OH, OW))]: the seven sources of the n = 7 launch; the fifth is the pitch-padded window at an odd address"""
    rng = np.random.default_rng(11)
    img = lambda h, w: torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
    win = _window(rng, 45, 61, 3 * 61 + 11, 3)
    assert win.data_ptr() % 2 == 1
    return [(img(1, 1), (32, 32)), (img(37, 53), (64, 96)), (img(200, 300), (96, 64)), (img(3, 500), (48, 16)), (win, (40, 56)),
            (img(37, 53), (20, 30)), (img(64, 48), (2100, 2048))]


def _run_sources(pairs, norm, interp, swap_rb):
    """one launch into a sentinel-filled buffer whose slots are GUARD floats apart -> (buffer, offsets)"""
    from rapiddoc_amd.engine import launch_resize_sources, pack_resize_sources, resize_source_view
    offs, n = [], 3
    for _t, (oh, ow) in pairs:
        offs.append(n)
        n += 3 * oh * ow + GUARD
    out = torch.full((n + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    views = [resize_source_view(t) for t, _hw in pairs]
    descs = pack_resize_sources([v[0] for v in views], [v[1] for v in views], [tuple(t.shape[:2]) for t, _hw in pairs], [hw for _t, hw in pairs], offs)
    launch_resize_sources(descs, out.device, out.data_ptr(), out.numel(), interp=interp, swap_rb=swap_rb, **norm)
    return out, offs


@pytest.mark.parametrize("norm", [DET_NORM, RAW_NORM], ids=["det", "raw"])
@pytest.mark.parametrize("swap_rb", [False, True])
@pytest.mark.parametrize("interp", [1, 2])
def test_sources_kernel_is_the_single_image_kernel_bit_for_bit(kernel_sources, interp, swap_rb, norm):
    from rapiddoc_amd.engine import preproc_resize_norm
    before = [t.clone() for t, _hw in kernel_sources]
    refs = [preproc_resize_norm(t.contiguous(), hw, interp=interp, swap_rb=swap_rb, **norm) for t, hw in kernel_sources]
    for pairs, want in ((kernel_sources, refs), (kernel_sources[4:5], refs[4:5]), (kernel_sources[6:], refs[6:])):      # n = 7, n = 1, n = 1
        out, offs = _run_sources(pairs, norm, interp, swap_rb)
        expect = torch.full_like(out, SENTINEL)
        for o, r in zip(offs, want):
            expect[o: o + r.numel()] = r.reshape(-1)
        torch.cuda.synchronize()
        for k, (o, r) in enumerate(zip(offs, want)):
            assert same_bits(out[o: o + r.numel()], r.reshape(-1)), (len(pairs), k)
        assert same_bits(out, expect)                          # guards, the floats in front of the first and behind the last slot
    for t, (b, _hw) in zip(before, kernel_sources):
        assert torch.equal(t, b)                               # inputs unchanged


def test_python_face_writes_rows_of_batch_tensors_and_its_own_buffer(kernel_sources):
    from rapiddoc_amd.engine import preproc_resize_norm, preproc_resize_norm_sources
    srcs = [t for t, _hw in kernel_sources[:5]]
    x = torch.full((6, 3, 24, 40), SENTINEL, device="cuda")
    got = preproc_resize_norm_sources(srcs, [(24, 40)] * 5, interp=2, out=[x[4], x[0], x[2], x[1], x[3]])
    for t, g, row in zip(srcs, got, (4, 0, 2, 1, 3)):
        assert same_bits(x[row], preproc_resize_norm(t.contiguous(), (24, 40), interp=2)) and g.data_ptr() == x[row].data_ptr()
    assert float((x[5] - SENTINEL).abs().max()) == 0.0
    own = preproc_resize_norm_sources(srcs, [hw for _t, hw in kernel_sources[:5]], interp=1, swap_rb=True, **DET_NORM)
    for t, (_s, hw), g in zip(srcs, kernel_sources, own):
        assert same_bits(g, preproc_resize_norm(t.contiguous(), hw, interp=1, swap_rb=True, **DET_NORM))


def test_refused_calls_launch_nothing():
    from rapiddoc_amd import _lib
    from rapiddoc_amd.engine import pack_resize_sources
    lib = _lib.load()
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    p = src.data_ptr()
    good = dict(ptrs=[p, p], pitches=[24, 24], hws=[(8, 8), (8, 8)], out_hws=[(4, 4), (4, 4)], out_offs=[0, 48])
    m, s = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    stream = torch.cuda.current_stream().cuda_stream

    def refused(match, host=True, dev=True, out=True, n=None, interp=1, out_floats=96, **change):
        descs = pack_resize_sources(**{**good, **change})
        d_dev = torch.from_numpy(descs.view(np.uint8).copy()).cuda()
        buf = torch.full((128,), SENTINEL, device="cuda")
        rc = lib.rd_preproc_resize_norm_sources(0, descs.ctypes.data if host else None, d_dev.data_ptr() if dev else None,
                                                len(descs) if n is None else n, m, s, 1.0, interp, 0, buf.data_ptr() if out else None,
                                                C.c_int64(out_floats), stream)
        torch.cuda.synchronize()
        assert rc != 0 and match in lib.rd_create_error().decode(), (match, rc, lib.rd_create_error())
        assert float((buf - SENTINEL).abs().max()) == 0.0       # a fresh output buffer is untouched

    refused("NULL", host=False)
    refused("NULL", dev=False)
    refused("NULL", out=False)
    refused("n outside", n=0)
    refused("n outside", n=65536)
    refused("src is NULL", ptrs=[p, 0])
    refused("pitch", pitches=[24, 23])
    refused("source size", hws=[(8, 8), (0, 8)])
    refused("source size", hws=[(32769, 8), (8, 8)])
    refused("output size", out_hws=[(4, 4), (4, 0)])
    refused("output size", out_hws=[(4, 32769), (4, 4)])
    refused("interp", interp=0)
    refused("interp", interp=3)
    refused("negative", out_offs=[-1, 48])
    refused("overruns", out_floats=95)
    refused("overlap", out_offs=[0, 47])
    descs = pack_resize_sources(**good)                              # the accepted twin of the calls above
    d_dev = torch.from_numpy(descs.view(np.uint8).copy()).cuda()
    buf = torch.full((128,), SENTINEL, device="cuda")
    assert lib.rd_preproc_resize_norm_sources(0, descs.ctypes.data, d_dev.data_ptr(), 2, m, s, 1.0, 1, 0, buf.data_ptr(), C.c_int64(96), stream) == 0
    torch.cuda.synchronize()
    assert float(buf[:96].abs().max()) == 0.0 and float((buf[96:] - SENTINEL).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- the pipeline
PAGE_HW = [(200, 140), (140, 200), (200, 140), (120, 260), (140, 200)]
# text lines (x0, y0, x1, y1) per page: 12 px tall, aspect ratios between 5 and 20, so that the strict mode's chunks of six pad to
# widths above 320 and the chunk a line falls into decides its padded width
PAGE_BOXES = [
    [(8, 16, 70, 28), (8, 60, 100, 72), (8, 104, 120, 116), (8, 150, 133, 162)],
    [(8, 14, 90, 26), (8, 44, 140, 56), (8, 74, 180, 86), (8, 106, 195, 118)],
    [(8, 20, 78, 32), (8, 62, 108, 74), (8, 110, 126, 122), (8, 160, 131, 172)],
    [(8, 12, 130, 24), (8, 46, 210, 58), (8, 84, 252, 96)],
    [(8, 16, 98, 28), (8, 46, 150, 58), (8, 76, 172, 88), (8, 108, 188, 120)],
]


@pytest.fixture(scope="module")
def pipe(golden_dir):
    from rapiddoc_amd.pipeline import PagePipeline
    states = {k: W.synth_state_dict(W.load_manifest(golden_dir / f"manifest_{k}.json"), 0) for k in ("ppocrv6_det", "ppocrv6_rec", "pphgnetv2_b4")}
    p = PagePipeline(states, n_rec_streams=2)
    assert p.rec_mode == "strict"
    return p


@pytest.fixture(scope="module")
def pages_np():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in PAGE_HW]


def _maps(hw, boxes, device):
    from rapiddoc_amd.pipeline import page_det_shape, render_text_maps
    return render_text_maps([np.float32(boxes)], hw, page_det_shape(*hw), device)


def _strings(res):
    return [[(t, s) for _q, t, s in r.lines] for r in res]


@pytest.fixture(scope="module")
def mixed(pipe, pages_np):
    """the mixed list through run_batch ONCE, with everything the tests below look at copied out"""
    pages = [torch.from_numpy(p).cuda() for p in pages_np]
    maps = [_maps(hw, b, pipe.tdev) for hw, b in zip(PAGE_HW, PAGE_BOXES)]
    pipe.keep_rec_inputs = True
    res = pipe.run_batch(pages, None, det_maps_override=maps)
    torch.cuda.synchronize()
    out = dict(pages=pages, maps=maps, res=res, stats=dict(pipe.stats),
               det=[(m.clone(), hw, list(ix)) for m, hw, ix in pipe.last_det],
               widths={int(i): int(w) for chunk, _x, lw, _i, _p in pipe.last_rec_batches for i, w in zip(chunk.tolist(), lw)},
               crop_sizes=tuple(np.array(a) for a in pipe.last_rec_crop_sizes))
    pipe.keep_rec_inputs = False
    pipe.last_rec_batches = []
    return out


def test_det_groups_and_launch_counts(mixed):
    assert [(hw, ix) for _m, hw, ix in mixed["det"]] == [((320, 256), [0, 2]), ((256, 320), [1, 4]), ((256, 384), [3])]
    st = mixed["stats"]
    assert st["det_groups"] == 3 and st["preproc_launches"] == 2                     # det + layout: one sources launch each
    assert st["rec_batches"] >= 1 and st["warp_source_launches"] == st["rec_batches"]       # one warp launch per rec launch
    assert st["front_prefetched"] == 0.0


def test_every_page_of_the_mixed_list_gets_the_det_map_it_gets_alone(pipe, mixed):
    for maps, hw, members in mixed["det"]:
        assert tuple(maps.shape) == (len(members), 1) + hw
        for j, i in enumerate(members):
            alone, alone_hw = pipe.det_forward(mixed["pages"][i][None].contiguous())
            assert alone_hw == hw and same_bits(maps[j], alone[0]), i


def test_mixed_list_pools_every_line_into_one_strict_plan(pipe, mixed):
    res = mixed["res"]
    n_lines = [len(r.lines) for r in res]
    assert n_lines == [len(b) for b in PAGE_BOXES]                                   # caller order: page 3 is the one with three lines
    for r, boxes in zip(res, PAGE_BOXES):                                            # ... and every page got its own boxes back
        for (q, _t, _s), b in zip(r.lines, boxes):
            assert abs(float(q[:, 0].mean()) - (b[0] + b[2]) / 2) < 8 and abs(float(q[:, 1].mean()) - (b[1] + b[3]) / 2) < 6
    # texts and scores: rec_forward_sources over the same (page, quads) sources, pooled
    quads = [np.stack([q for q, _t, _s in r.lines]) for r in res]
    want = pipe.rec_forward_sources([(p[None].contiguous(), [q]) for p, q in zip(mixed["pages"], quads)], image_keys=[[i] for i in range(len(res))])
    assert [w[0] for w in want] == _strings(res)
    # padded widths: what the reference's one argsort over the pooled list gives every line
    cw, ch, rot, keep = mixed["crop_sizes"]
    n = sum(n_lines)
    assert len(keep) == n and sorted(mixed["widths"]) == list(range(n))
    ratios = [float(ch[i]) / float(cw[i]) if rot[i] else float(cw[i]) / float(ch[i]) for i in range(n)]

    def widths_of(ids):
        batches, line_w = ocr_host.rec_batches_lines([ratios[i] for i in ids], native=False)
        order = np.concatenate([c for c, _w in batches])
        return {ids[int(k)]: int(w) for k, w in zip(order, line_w)}
    pooled = widths_of(list(range(n)))
    assert mixed["widths"] == pooled
    # ... which is NOT what one call per size group would have given: at least one line changes its width
    first = np.cumsum([0] + n_lines)
    per_group = {}
    for _m, _hw, members in mixed["det"]:
        per_group.update(widths_of([i for p in members for i in range(first[p], first[p + 1])]))
    assert any(per_group[i] != pooled[i] for i in range(n))


def test_list_of_equal_pages_is_the_tensor_path_bit_for_bit(pipe, pages_np):
    rng = np.random.default_rng(9)
    pages = [torch.from_numpy(rng.integers(0, 256, (200, 140, 3), dtype=np.uint8)).cuda() for _ in range(3)]
    boxes = [PAGE_BOXES[0], PAGE_BOXES[2], PAGE_BOXES[0][:2]]
    maps = [_maps((200, 140), b, pipe.tdev) for b in boxes]
    want = pipe.run_batch(torch.stack(pages), None, det_maps_override=torch.cat(maps))
    got = pipe.run_batch(pages, None, det_maps_override=maps)
    assert [len(r.lines) for r in want] == [4, 4, 2] and _strings(got) == _strings(want)
    for a, b in zip(got, want):
        assert all(np.array_equal(qa, qb) for (qa, _t, _s), (qb, _t2, _s2) in zip(a.lines, b.lines))


def test_host_list_and_uploader_list_equal_the_device_list(pipe, mixed, pages_np):
    from rapiddoc_amd.pipeline import PageUploader
    want = _strings(mixed["res"])
    assert _strings(pipe.run_batch(list(pages_np), None, det_maps_override=mixed["maps"])) == want                      # numpy pages
    assert _strings(pipe.run_batch([torch.from_numpy(p) for p in pages_np], None, det_maps_override=mixed["maps"])) == want
    with pytest.raises(ValueError, match="mix"):
        pipe.run_batch([mixed["pages"][0], pages_np[1]])
    up = PageUploader(0)
    for _round in range(3):                                       # the third submit recycles the first buffer
        ticket = up.submit(list(pages_np))
        dev = up.wait(ticket)
        assert isinstance(dev, list) and all(d.is_cuda and torch.equal(d.cpu(), torch.from_numpy(p)) for d, p in zip(dev, pages_np))
        got = pipe.run_batch(dev, None, det_maps_override=mixed["maps"])
        up.release(ticket)
        assert _strings(got) == want
    assert up.bytes_uploaded == 3 * PageUploader.plan_list(PAGE_HW)[1]


def test_prefetch_of_a_list_gives_the_results_of_two_plain_calls(pipe, mixed):
    cur, cur_maps = mixed["pages"], mixed["maps"]
    order = [3, 0, 4]
    nxt = [mixed["pages"][i].clone() for i in order]
    nxt_maps = [mixed["maps"][i] for i in order]
    want_cur, want_nxt = _strings(mixed["res"]), _strings(pipe.run_batch(nxt, None, det_maps_override=nxt_maps))
    assert [len(p) for p in want_nxt] == [len(want_cur[i]) for i in order]
    got_cur = pipe.run_batch(cur, None, det_maps_override=cur_maps, prefetch=nxt)
    assert pipe.stats["front_prefetched"] == 0.0
    got_nxt = pipe.run_batch(nxt, None, det_maps_override=nxt_maps)
    assert pipe.stats["front_prefetched"] == 1.0 and pipe.stats["det_groups"] == 3
    assert _strings(got_cur) == want_cur and _strings(got_nxt) == want_nxt


# ---------------------------------------------------------------------------------------------------------------- the two call sites
def test_layout_preprocess_in_one_launch_equals_the_page_loop(pages_np):
    from rapiddoc_amd.layout_model import LayoutModel, SyntheticBoxSession
    model = LayoutModel(SyntheticBoxSession(["text", "table"], boxes_per_page=2), "pp_doclayoutv3")
    host = [pages_np[0], pages_np[1], pages_np[3]]
    dev = [torch.from_numpy(p).cuda() for p in host]
    for pages in (host, dev, [host[0], dev[1], torch.from_numpy(host[2])]):
        x0, sf0 = model.preprocess_loop(pages)
        x1, sf1 = model.preprocess_sources(pages)
        torch.cuda.synchronize()
        assert same_bits(x0, x1) and sf0.dtype == sf1.dtype and np.array_equal(sf0, sf1)


def test_unitable_linear_preprocess_in_one_launch_equals_the_table_loop(golden_dir, monkeypatch):
    from rapiddoc_amd import table_unitable as TU
    m = TU.Mi355UniTableStructure(R.state(golden_dir), R.dec_state(golden_dir), TU.STAND_IN_IDS, TU.stand_in_tokens(), max_new_tokens=6, resize="linear")
    tables = [W.synth_table_crop(3, 90, 150), W.synth_table_crop(4, 200, 120), torch.from_numpy(W.synth_table_crop(5, 61, 333)).cuda()]
    monkeypatch.setattr(TU.Mi355UniTableStructure, "LINEAR_ROUTE", "loop")
    x0, shapes0 = m.preprocess(tables)
    alone = [m.decode_ids(m.preprocess([t])[0])[0] for t in tables]
    monkeypatch.setattr(TU.Mi355UniTableStructure, "LINEAR_ROUTE", "sources")
    x1, shapes1 = m.preprocess(tables)
    torch.cuda.synchronize()
    assert same_bits(x0, x1) and shapes0 == shapes1 == [(90, 150), (200, 120), (61, 333)]
    assert m.decode_ids(x1) == alone
