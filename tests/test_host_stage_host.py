"""CPU: the host half of the image staging behind the plugin seam (rapiddoc_amd/host_stage.py, csrc/stage_pack.cpp) - `rd_stage_pack`
against numpy byte for byte, the offset plan, and the rd_stage_desc packing against a numpy restatement.  No GPU, no tolerance."""
import ctypes as C

import numpy as np
import pytest

GUARD = 0xA5


@pytest.fixture(scope="module")
def lib():
    from rapiddoc_amd import build as rd_build
    rd_build.build(verbose=False)
    from rapiddoc_amd import _lib
    return _lib.load()


def _images(seed=0):
    """contiguous images, a row-strided window of a larger array, 1 x 1, a zero-area image among the others, one large enough for 16 threads"""
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (90, 140, 3), dtype=np.uint8)
    window = big[7:68, 11:120]                                      # rows 140 * 3 bytes apart, 109 pixels wide
    assert not window.flags.c_contiguous and window.strides == (420, 3, 1)
    return [rng.integers(0, 256, (30, 200, 3), dtype=np.uint8), window, rng.integers(0, 256, (1, 1, 3), dtype=np.uint8),
            np.zeros((0, 5, 3), np.uint8), rng.integers(0, 256, (65, 130, 3), dtype=np.uint8), np.zeros((4, 0, 3), np.uint8),
            rng.integers(0, 256, (611, 701, 3), dtype=np.uint8), rng.integers(0, 256, (3, 7, 3), dtype=np.uint8)]


def _expected(images, offsets, total):
    want = np.full(total, GUARD, np.uint8)
    for im, o in zip(images, offsets):
        want[o: o + im.size] = np.ascontiguousarray(im).reshape(-1)
    return want


def _pack(images, n_threads, slack=64):
    from rapiddoc_amd import host_stage as HS
    arrs = [HS.as_stage_image(im) for im in images]
    offsets, total = HS.plan_offsets([a.shape[:2] for a in arrs])
    buf = np.full(total + slack, GUARD, np.uint8)
    HS.pack_images(arrs, offsets, buf.ctypes.data, total, n_threads)
    return arrs, offsets, total, buf


def test_offsets_are_aligned_ascending_and_disjoint():
    from rapiddoc_amd import host_stage as HS
    shapes = [im.shape[:2] for im in _images()]
    offsets, total = HS.plan_offsets(shapes)
    assert all(o % 16 == 0 for o in offsets) and total % 16 == 0
    ends = [o + 3 * h * w for o, (h, w) in zip(offsets, shapes)]
    assert all(e <= nxt for e, nxt in zip(ends, offsets[1:] + [total]))          # no overlap, in order
    assert offsets[3] == offsets[4] and offsets[5] == offsets[6]                 # zero-area images take no bytes
    assert HS.plan_offsets([]) == ([], 0) and HS.plan_offsets([(1, 1)]) == ([0], 16)


def test_pack_equals_numpy_and_leaves_the_gaps_alone(lib):
    images = _images()
    arrs, offsets, total, buf = _pack(images, 1)
    assert arrs[1].base is not None and not arrs[1].flags.c_contiguous          # the window went in as a view, not as a copy
    assert np.array_equal(buf[:total], _expected(images, offsets, total))       # images equal, bytes between them untouched
    assert bool((buf[total:] == GUARD).all())


def test_one_thread_and_sixteen_threads_give_the_same_buffer(lib):
    images = _images(3)
    assert sum(im.size for im in images) > 16 * 64 * 1024                        # enough bytes for all 16 threads to get rows
    _a, offsets, total, one = _pack(images, 1)
    for n_threads in (2, 7, 16, 1000, 0, -3):                                    # (capped at 16; below 1 means 1)
        _a, _o, _t, many = _pack(images, n_threads)
        assert np.array_equal(one, many), n_threads
    assert np.array_equal(one[:total], _expected(images, offsets, total))


def test_a_single_image_and_other_layouts(lib):
    from rapiddoc_amd import host_stage as HS
    rng = np.random.default_rng(5)
    one = rng.integers(0, 256, (17, 23, 3), dtype=np.uint8)
    _a, offsets, total, buf = _pack([one], 16)
    assert offsets == [0] and np.array_equal(buf[: one.size], one.reshape(-1)) and bool((buf[one.size:] == GUARD).all())
    # what rd_stage_pack does not take is made contiguous first: flipped rows / columns, reversed channels, another dtype, a column window of width 1
    base = rng.integers(0, 256, (12, 9, 3), dtype=np.uint8)
    odd = [base[::-1], base[:, ::-1], base[:, :, ::-1], base.astype(np.int32), base[:, 4:5], base[3:4], base.transpose(1, 0, 2)]
    arrs, offsets, total, buf = _pack(odd, 4)
    assert np.array_equal(buf[:total], _expected([np.asarray(o).astype(np.uint8) for o in odd], offsets, total))
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(HS.StageError):
            HS.as_stage_image(bad)


def test_bad_arguments_return_non_zero_and_write_nothing(lib):
    a = np.arange(5 * 6 * 3, dtype=np.uint8).reshape(5, 6, 3)
    b = np.arange(2 * 2 * 3, dtype=np.uint8).reshape(2, 2, 3)
    buf = np.full(256, GUARD, np.uint8)

    def call(srcs, pitches, hs, ws, offs, n, dst, dst_bytes, threads=4):
        arr = lambda v, t: None if v is None else np.asarray(v, dtype=t)
        keep = [arr(srcs, np.uint64), arr(pitches, np.int64), arr(hs, np.int32), arr(ws, np.int32), arr(offs, np.int64)]
        ptr = lambda x: None if x is None else x.ctypes.data
        return lib.rd_stage_pack(*[ptr(k) for k in keep], n, dst, C.c_int64(dst_bytes), threads)

    good = ([a.ctypes.data, b.ctypes.data], [18, 6], [5, 2], [6, 2], [0, 96], 2, buf.ctypes.data, 256)
    bad = {
        "srcs NULL": (None,) + good[1:],
        "offsets NULL": good[:4] + (None,) + good[5:],
        "dst NULL": good[:6] + (None, 256),
        "n < 0": good[:5] + (-1,) + good[6:],
        "negative height": good[:2] + ([5, -2],) + good[3:],
        "negative width": good[:3] + ([-6, 2],) + good[4:],
        "negative offset": good[:4] + ([0, -16],) + good[5:],
        "second image overruns": good[:4] + ([0, 250],) + good[5:],
        "first image overruns": good[:7] + (89,),
        "image source NULL": ([a.ctypes.data, 0],) + good[1:],
        "pitch below the row": good[:1] + ([17, 6],) + good[2:],
        "negative pitch": good[:1] + ([-18, 6],) + good[2:],
    }
    for name, args in bad.items():
        assert call(*args) != 0, name
        assert bool((buf == GUARD).all()), name                                  # the FIRST image was not written either
    assert call(*good) == 0
    assert np.array_equal(buf[:90], a.reshape(-1)) and np.array_equal(buf[96:108], b.reshape(-1)) and bool((buf[90:96] == GUARD).all())
    assert call(None, None, None, None, None, 0, None, 0) == 0                   # nothing to do is no error


def test_descriptors_equal_a_numpy_restatement():
    """`Staged` + size groups -> rd_stage_desc array: several groups in one array, canvases disjoint"""
    from rapiddoc_amd import host_stage as HS
    assert HS.STAGE_DESC_DTYPE.itemsize == 48
    assert [HS.STAGE_DESC_DTYPE.fields[n][1] for n in ("src", "pitch", "canvas", "w", "h", "gh", "gw", "flags", "reserved")] == [0, 8, 16, 24, 28, 32, 36, 40, 44]
    shapes = [(30, 200), (64, 64), (65, 130), (1, 1), (60, 190), (100, 129), (7, 5)]
    offsets, total = HS.plan_offsets(shapes)
    base = 0x7F00_0000_1000
    groups = [((64, 256), [0, 4]), ((64, 64), [1, 3, 6]), ((128, 192), [2, 5])]
    sizes = [len(m) * gh * gw * 3 for (gh, gw), m in groups]
    canvas_ptrs = [0x7E00_0000_0000, 0x7E00_0000_0000 + sizes[0] + 512, 0x7E10_0000_0000]
    descs = HS.pack_stage_descs(base, offsets, shapes, groups, canvas_ptrs, swap_rb=True)
    want = []
    for ((gh, gw), members), cp in zip(groups, canvas_ptrs):
        for j, i in enumerate(members):
            h, w = shapes[i]
            want.append((base + offsets[i], 3 * w, cp + j * gh * gw * 3, w, h, gh, gw, 1, 0))
    assert descs.dtype == HS.STAGE_DESC_DTYPE and descs.tolist() == want and len(descs) == 7
    spans = sorted((int(d["canvas"]), int(d["canvas"]) + int(d["gh"]) * int(d["gw"]) * 3) for d in descs)
    assert all(a_end <= b_beg for (_a, a_end), (b_beg, _b) in zip(spans, spans[1:]))        # canvas addresses are disjoint
    assert all(int(d["w"]) <= int(d["gw"]) and int(d["h"]) <= int(d["gh"]) and int(d["gw"]) % 4 == 0 for d in descs)
    assert HS.pack_stage_descs(base, offsets, shapes, groups, canvas_ptrs, swap_rb=False)["flags"].tolist() == [0] * 7
    assert len(HS.pack_stage_descs(base, offsets, shapes, [], [])) == 0
