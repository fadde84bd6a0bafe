"""GPU: host images behind the plugin seam - `rd_stage_canvases` (csrc/kernels_stage.hip) against a numpy restatement byte for byte,
`HostImageStage.upload`, and the two seams' "stage" routes against their default routes (`RegionTextModel`: canvases and strings;
`FormulaRecognizer`: token ids and routes, chunk and stream batching, and through `plugin.custom_configs`).  Every comparison is equality
of bytes, ids or strings."""
from abc import ABC, abstractmethod

import numpy as np
import pytest
import torch

import formula_pre_reference as R
from rapiddoc_amd import weights as W

pytestmark = pytest.mark.gpu
GUARD = 0xA5


# ---------------------------------------------------------------------------------------------------------------- rd_stage_canvases
def _canvas(crop: np.ndarray, gh: int, gw: int, swap: bool) -> np.ndarray:
    """the restatement: 255 everywhere, the crop at (0, 0), first and third channel exchanged when asked"""
    out = np.full((gh, gw, 3), 255, np.uint8)
    out[: crop.shape[0], : crop.shape[1]] = crop[:, :, ::-1] if swap else crop
    return out


class _Launch:
    """crops in one device source buffer (each at a chosen byte address and pitch), canvases in one guarded device buffer"""

    def __init__(self, cases, seed=0, gap=68):
        from rapiddoc_amd import host_stage as HS
        rng = np.random.default_rng(seed)
        self.cases = cases                                             # (h, w, gh, gw, swap, source address modulo 4, extra pixels per row)
        src_parts, self.crops, src_offs, at = [], [], [], 0
        for h, w, _gh, _gw, _swap, mod, extra in cases:
            at += (mod - at) % 4                                       # the crop's first byte at an address = mod (mod 4)
            pitch = 3 * (w + extra)
            block = rng.integers(0, 255, h * pitch, dtype=np.uint8)    # (never 255: a white byte in the result is the fill, not the crop)
            src_parts.append((at, block))
            self.crops.append(np.lib.stride_tricks.as_strided(block, (h, w, 3), (pitch, 3, 1)).copy())
            src_offs.append(at)
            at += block.size
        src_host = np.zeros(at + 4, np.uint8)
        for o, block in src_parts:
            src_host[o: o + block.size] = block
        self.src = torch.from_numpy(src_host).cuda()
        assert self.src.data_ptr() % 4 == 0
        canv_offs, at = [], 0
        for _h, _w, gh, gw, *_ in cases:
            canv_offs.append(at)
            at += gh * gw * 3 + gap                                    # `gap` guard bytes behind every canvas (a multiple of 4)
        self.canv_host = np.full(at, GUARD, np.uint8)
        self.canv = torch.from_numpy(self.canv_host.copy()).cuda()
        self.canv_offs = canv_offs
        self.descs = np.zeros(len(cases), HS.STAGE_DESC_DTYPE)
        for k, (h, w, gh, gw, swap, _mod, extra) in enumerate(cases):
            self.descs[k] = (self.src.data_ptr() + src_offs[k], 3 * (w + extra), self.canv.data_ptr() + canv_offs[k], w, h, gh, gw, 1 if swap else 0, 0)

    def expected(self) -> np.ndarray:
        want = self.canv_host.copy()
        for crop, o, (_h, _w, gh, gw, swap, *_rest) in zip(self.crops, self.canv_offs, self.cases):
            want[o: o + gh * gw * 3] = _canvas(crop, gh, gw, swap).reshape(-1)
        return want

    def run(self, descs=None) -> np.ndarray:
        from rapiddoc_amd import host_stage as HS
        HS.launch_stage_canvases(self.descs if descs is None else descs, self.src.device)
        torch.cuda.synchronize()
        return self.canv.cpu().numpy()


# (h, w, gh, gw, swap, source address mod 4, extra pixels per source row)
CASES = [(1, 1, 64, 64, True, 0, 0),
         (64, 64, 64, 64, True, 0, 0),                                 # nothing white
         (65, 3, 128, 64, True, 2, 0),                                 # w % 4 = 3: a 4-pixel group that is part crop, part white
         (3, 65, 64, 128, True, 3, 2),                                 # w % 4 = 1
         (7, 5, 64, 64, True, 1, 4),                                   # 5 pixels wide, 7 rows, at an odd byte address, rows 27 bytes apart
         (7, 5, 64, 64, False, 1, 4),                                  # the same crop without the swap
         (63, 127, 64, 128, True, 0, 0)]                               # last row and last column white


def test_canvases_equal_the_numpy_restatement_in_one_launch():
    launch = _Launch(CASES)
    launch.crops[5] = launch.crops[4].copy()                           # "the same crop": case 5 reads case 4's bytes
    launch.descs[5]["src"], launch.descs[5]["pitch"] = launch.descs[4]["src"], launch.descs[4]["pitch"]
    assert int(launch.descs[4]["src"]) % 2 == 1
    assert len({(int(d["gh"]), int(d["gw"])) for d in launch.descs}) == 3          # three size groups share the launch
    got, want = launch.run(), launch.expected()
    for k, (o, (h, w, gh, gw, *_)) in enumerate(zip(launch.canv_offs, CASES)):
        n = gh * gw * 3
        assert np.array_equal(got[o: o + n], want[o: o + n]), f"canvas {k} ({h} x {w} in {gh} x {gw})"
        assert bool((got[o + n: o + n + 68] == GUARD).all()), f"guard behind canvas {k}"
    assert np.array_equal(got, want)
    a, b = got[launch.canv_offs[4]:][: 64 * 64 * 3].reshape(64, 64, 3), got[launch.canv_offs[5]:][: 64 * 64 * 3].reshape(64, 64, 3)
    assert np.array_equal(a, b[:, :, ::-1]) and not np.array_equal(a, b)


def test_a_canvas_beyond_one_pass_of_the_grid_and_many_small_ones():
    """1088 x 1024 canvas pixels are more 4-pixel groups than the widest grid holds threads (the blocks stride on); 40 small crops ride
    along, so blocks past a small canvas's end and the long canvas share a launch"""
    rng = np.random.default_rng(7)
    cases = [(1000, 999, 1088, 1024, True, 1, 3)]
    cases += [(int(rng.integers(1, 65)), int(rng.integers(1, 129)), 64, 128, bool(k % 2), int(rng.integers(0, 4)), int(rng.integers(0, 3))) for k in range(40)]
    launch = _Launch(cases, seed=1)
    assert np.array_equal(launch.run(), launch.expected())


def test_bad_arguments_launch_nothing():
    from rapiddoc_amd import _lib
    from rapiddoc_amd import host_stage as HS
    lib = _lib.load()
    launch = _Launch(CASES[:3])
    stream = torch.cuda.current_stream().cuda_stream

    def changed(k, **fields):
        d = launch.descs.copy()
        for name, v in fields.items():
            d[k][name] = v
        return d
    bad = {"w > gw": changed(1, w=65), "h > gh": changed(0, h=65), "gw % 4 != 0": changed(2, gw=66), "gw = 0": changed(0, gw=0, w=0),
           "gh beyond 16384": changed(0, gh=16385), "canvas NULL": changed(1, canvas=0), "canvas misaligned": changed(1, canvas=int(launch.descs[1]["canvas"]) + 2),
           "src NULL": changed(1, src=0), "pitch below the row": changed(1, pitch=3 * 64 - 1), "negative width": changed(0, w=-1)}
    for name, descs in bad.items():
        with pytest.raises(HS.StageError, match="rd_stage_canvases"):
            HS.launch_stage_canvases(descs, launch.src.device)
    dev = torch.from_numpy(launch.descs.view(np.uint8).reshape(-1).copy()).cuda()
    host = launch.descs
    for args in ((None, dev.data_ptr(), 3), (host.ctypes.data, None, 3), (host.ctypes.data, dev.data_ptr(), 0), (host.ctypes.data, dev.data_ptr(), -1),
                 (host.ctypes.data, dev.data_ptr(), 65536)):
        assert lib.rd_stage_canvases(0, args[0], args[1], args[2], stream) == 1
        assert b"rd_stage_canvases" in lib.rd_create_error()
    torch.cuda.synchronize()
    assert bool((launch.canv.cpu().numpy() == GUARD).all())            # canvases and guards untouched by every refused call
    assert np.array_equal(launch.run(), launch.expected())             # and the good descriptors run


# ---------------------------------------------------------------------------------------------------------------- HostImageStage
def test_upload_views_equal_the_inputs_and_the_buffers_are_reused():
    from rapiddoc_amd.host_stage import HostImageStage
    rng = np.random.default_rng(11)
    big = rng.integers(0, 256, (80, 300, 3), dtype=np.uint8)
    first = [rng.integers(0, 256, (30, 200, 3), dtype=np.uint8), big[5:70, 17:290], rng.integers(0, 256, (1, 1, 3), dtype=np.uint8),
             np.zeros((0, 5, 3), np.uint8), rng.integers(0, 256, (65, 130, 3), dtype=np.uint8)]
    stage = HostImageStage(torch.device("cuda", 0))
    staged = stage.upload(first)
    got = [v.cpu().numpy() for v in staged.views]                      # the consumer of the first upload
    stage.release()
    assert [tuple(v.shape) for v in staged.views] == [im.shape for im in first] and all(v.is_cuda and v.dtype == torch.uint8 for v in staged.views)
    assert all(np.array_equal(g, im) for g, im in zip(got, first))
    assert all(o % 16 == 0 for o in staged.offsets) and staged.base == stage._dev.data_ptr() and staged.shapes == [im.shape[:2] for im in first]
    pin, dev = stage._pin.data_ptr(), stage._dev.data_ptr()
    second = [rng.integers(0, 256, (64, 64, 3), dtype=np.uint8), rng.integers(0, 256, (3, 7, 3), dtype=np.uint8)]
    staged2 = stage.upload(second)                                     # smaller: the same two buffers, behind the first upload's event
    assert (stage._pin.data_ptr(), stage._dev.data_ptr()) == (pin, dev) and stage.uploads == 2
    assert all(np.array_equal(v.cpu().numpy(), im) for v, im in zip(staged2.views, second))
    third = [rng.integers(0, 256, (700, 800, 3), dtype=np.uint8)]      # larger than the buffer: it grows, no release in between
    staged3 = stage.upload(third)
    assert stage._pin.numel() >= third[0].size and np.array_equal(staged3.views[0].cpu().numpy(), third[0])
    assert stage.upload([]).views == []


# ---------------------------------------------------------------------------------------------------------------- RegionTextModel
@pytest.fixture(scope="module")
def pipeline(golden_dir):
    from rapiddoc_amd.pipeline import PagePipeline
    states = {k: W.synth_state_dict(W.load_manifest(golden_dir / f"manifest_{k}.json"), 0) for k in ("ppocrv6_det", "ppocrv6_rec")}
    return PagePipeline(states, rec_batch_num=32)


def test_region_text_model_stage_route_equals_the_copy_route(pipeline):
    from rapiddoc_amd.analyze import RegionTextModel
    from rapiddoc_amd.pages import synth_page
    page, _boxes = synth_page(0)                                       # real glyphs, so that the recogniser has something to read
    bgr = np.ascontiguousarray(page[:, :, ::-1])
    sizes = [(30, 200), (64, 64), (65, 130), (1, 1), (0, 5), (60, 250), (100, 129), (40, 33), (20, 256)]
    crops = [bgr[40 + 3 * k: 40 + 3 * k + h, 30 + 5 * k: 30 + 5 * k + w] for k, (h, w) in enumerate(sizes)]      # windows of the page: strided rows
    crops[1] = np.ascontiguousarray(crops[1])
    assert [c.shape[:2] for c in crops] == sizes

    def maps_fn(ids, ghw, dhw):                                        # fixed maps: two text boxes in every region
        m = torch.zeros((len(ids), 1, dhw[0], dhw[1]), dtype=torch.float32)
        m[:, 0, 4: dhw[0] // 2 - 2, 4: dhw[1] - 6] = 0.95
        m[:, 0, dhw[0] // 2 + 2: dhw[0] - 4, 8: dhw[1] // 2 + 8] = 0.9
        return m.cuda()

    copy_model, stage_model = RegionTextModel(pipeline), RegionTextModel(pipeline, host_images="stage")
    assert copy_model.host_images == "copy"
    want = copy_model.batch_predict(crops, det_maps_fn=maps_fn, batch_size=4)
    got = stage_model.batch_predict(crops, det_maps_fn=maps_fn, batch_size=4)
    assert len(copy_model.last_canvases) == len(stage_model.last_canvases) == 3
    assert sorted(tuple(c.shape) for c in copy_model.last_canvases) == [(2, 128, 192, 3), (3, 64, 64, 3), (3, 64, 256, 3)]
    for a, b in zip(copy_model.last_canvases, stage_model.last_canvases):
        assert a.shape == b.shape and torch.equal(a, b)
    assert got == want and len(got) == 9 and all(isinstance(t, str) for t in got) and got[4] == ""
    assert stage_model._stage.uploads == 1
    assert stage_model.batch_predict(crops[:3], det_maps_fn=maps_fn) == want[:3] and stage_model._stage.uploads == 2       # the stage is re-used
    assert stage_model.batch_predict([crops[4]]) == [""] and stage_model.last_canvases == []
    with pytest.raises(ValueError):
        RegionTextModel(pipeline, host_images="device")


# ---------------------------------------------------------------------------------------------------------------- FormulaRecognizer
NAMES = ["box_60x400", "box_5x700", "box_50x51", "uniform", "box_200x90"]          # four device-route sizes, one the device plan declines


@pytest.fixture(scope="module")
def formula_state(golden_dir):
    return W.synth_state_dict(W.load_manifest(golden_dir / "manifest_ppformulanet_plus_m_m8.json"), 0)


@pytest.fixture(scope="module")
def formula_crops(golden_dir):
    cases = {c["name"]: c for c in R.load_cases(golden_dir)}
    crops = [cases[n]["crop"] for n in NAMES]
    h, w = crops[2].shape[:2]                                          # one of them as a window of a larger array (strided rows)
    frame = np.random.default_rng(2).integers(0, 256, (h + 5, w + 9, 3), dtype=np.uint8)
    frame[2: 2 + h, 3: 3 + w] = crops[2]
    crops[2] = frame[2: 2 + h, 3: 3 + w]
    return crops


@pytest.fixture(scope="module")
def default_ids(formula_state, formula_crops):
    """the default instance on the same crops: (ids, routes).  It is handed the crops that have pixels: a numpy image without any is
    refused by the host pre-process (numpy's max of an empty array), which the default route leaves as it is."""
    from rapiddoc_amd.formula_host import FormulaRecognizer
    rec = FormulaRecognizer(formula_state, max_new_tokens=6)
    assert rec.host_images == "host"
    return rec.batch_predict(formula_crops, batch_size=2), list(rec.last_routes)


@pytest.mark.parametrize("batching", ["chunk", "stream"])
def test_formula_stage_route_equals_the_default_route(formula_state, formula_crops, default_ids, batching, monkeypatch):
    from rapiddoc_amd import formula_host as FH
    from rapiddoc_amd import plugin
    monkeypatch.setattr(FH, "PREPROC_SWITCH", "device")
    want, default_routes = default_ids
    assert default_routes == ["numpy"] * 5 and all(isinstance(r, list) for r in want)
    rec = FH.FormulaRecognizer(formula_state, max_new_tokens=6, host_images="stage", batching=batching)
    crops = formula_crops[:3] + [np.zeros((0, 5, 3), np.uint8)] + formula_crops[3:]            # one empty among them
    got = rec.batch_predict(crops, batch_size=2)                       # chunks of 2, 2, 1; one of them holds the declined crop
    assert rec.last_routes == ["staged", "host", "staged", "empty", "staged", "staged"]
    assert got[:3] + got[4:] == want and got[3] == []
    assert rec._stage.uploads == 1                                     # ONE upload for the call, not one per chunk

    class Base(ABC):                                                   # through the plugin, as the reference calls it
        @abstractmethod
        def batch_predict(self, image_list, **kwargs):
            pass
    model = plugin.custom_configs(formula=rec, base=Base)["formula_config"]["custom_model"]
    assert model is rec and isinstance(model, Base)
    assert model.batch_predict(crops, batch_size=16) == got
    assert rec.last_routes == ["staged", "host", "staged", "empty", "staged", "staged"] and rec._stage.uploads == 2
    monkeypatch.setattr(FH, "PREPROC_SWITCH", "host")                  # RD_FORMULA_PREPROC=host still forces the host
    assert rec.batch_predict(formula_crops, batch_size=2) == want and rec.last_routes == ["numpy"] * 5 and rec._stage.uploads == 2
