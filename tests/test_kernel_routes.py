"""CPU: the kernel routes of the dense and depthwise convolutions, asked through the two host-only developer entries rd_debug_conv_route /
rd_debug_dw_route (no HIP call: they run without a GPU).  The launchers, the planner (Builder::conv / deconv2x2 / dwconv) and rd_debug_conv /
rd_debug_dwconv all decide through the same functions (conv_split_route, conv_f32_route, dw_route), so what is pinned here is what runs.
Route table and names: docs/notebook/kernel_routes.md.

Run as a script (`python tests/test_kernel_routes.py`) it prints the depthwise sweep's violations as JSON: the switches are read once
per process, so the test repeats the sweep under RD_DW_LDS=0 / RD_DW_COL=1 in fresh interpreters."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

WH, W1, W3, W9 = 1, 2, 4, 8          # rd_debug_conv_route's `images` bits
NONE, GELU = 0, 2                    # rd::Act


def _load():
    """the library without the torch import of _lib.load(): nothing here touches the GPU"""
    from rapiddoc_amd import _lib, build as rd_build
    rd_build.build(verbose=False)       # (as tests/test_cabi.py: a no-op when the library is up to date)
    lib = C.CDLL(str(_lib.LIB_PATH))
    for name in ("rd_debug_conv_route", "rd_debug_dw_route"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.DEBUG_SYMBOLS[name]
    return lib


def conv_route(lib, n, h, w, cin, cout, k=1, s=1, pad=0, act=NONE, images=WH, has_ascale=0, allow_skinny=0, split=1):
    name = C.create_string_buffer(32)
    code = lib.rd_debug_conv_route(n, h, w, cin, cout, k, k, s, pad, pad, pad, pad, act, images, has_ascale, allow_skinny, split, name, 32)
    return name.value.decode(), code


def dw_route(lib, h, w, c, k, sh, ragged=0, has_line_w=0, wants_gap=0, n=2):
    """(kernel name, the route's chunk count, the planner's chunk count)"""
    name, chunks = C.create_string_buffer(32), C.c_int(-7)
    planned = lib.rd_debug_dw_route(n, h, w, c, k, sh, ragged, has_line_w, wants_gap, name, 32, C.byref(chunks))
    return name.value.decode(), chunks.value, planned


# ------------------------------------------------------------------------------------------------------------------------------ convolution
# (expected name, expected *used_direct code of rd_debug_conv, arguments).  The condition behind each row is the *_applies / *_shape_ok
# predicate documented next to the kernel; the tile rows follow h3_pick_tile (kernels_conv_h3.hip) and conv_f32_route (kernels_conv.hip).
CONV_TABLE = [
    # the specialised split kernels
    ("c3h1", 3, dict(n=1, h=32, w=32, cin=64, cout=64, k=3, pad=1, images=WH | W3)),
    ("direct", 1, dict(n=1, h=32, w=32, cin=64, cout=64, k=3, pad=1, images=WH)),
    ("c9h1", 4, dict(n=1, h=32, w=32, cin=64, cout=64, k=9, pad=4, images=WH | W9)),
    ("128x64", 0, dict(n=1, h=32, w=32, cin=64, cout=64, k=9, pad=4, images=WH)),                  # the implicit GEMM the 9x9 kernel displaces
    ("stream", 2, dict(n=1, h=32, w=32, cin=16, cout=24, k=3, pad=1, images=WH)),
    ("h1w256x128", 0, dict(n=1, h=64, w=64, cin=384, cout=768, images=WH | W1)),
    ("dma256x128", 0, dict(n=1, h=64, w=64, cin=384, cout=768, images=WH)),
    ("dma16w256x128", 0, dict(n=1, h=64, w=64, cin=192, cout=384, act=GELU, images=WH)),
    ("dma256x128", 0, dict(n=1, h=64, w=64, cin=192, cout=384, act=NONE, images=WH)),             # the 16-wavefront kernel is for short-K GELU layers
    # a gated (ascale) layer: none of the kernels above scales its rows on load, the staged tiles do
    ("256x128", 0, dict(n=1, h=64, w=64, cin=384, cout=768, images=WH | W1, has_ascale=1)),
    ("256x128", 0, dict(n=1, h=64, w=64, cin=192, cout=384, act=GELU, images=WH, has_ascale=1)),
    ("128x96", 0, dict(n=1, h=64, w=64, cin=384, cout=96, images=WH, has_ascale=1)),
    ("256x64", 0, dict(n=1, h=256, w=256, cin=384, cout=64, images=WH, has_ascale=1)),            # 33 .. 64 columns at M >= 65536
    ("128x64", 0, dict(n=1, h=64, w=64, cin=384, cout=64, images=WH, has_ascale=1)),
    ("128x32", 0, dict(n=1, h=64, w=64, cin=256, cout=64, images=WH, has_ascale=1)),              # K <= 256
    ("128x32", 0, dict(n=1, h=64, w=64, cin=384, cout=32, images=WH, has_ascale=1)),
    # ... and so do the layers no specialised kernel serves (stride 2)
    ("256x128", 0, dict(n=1, h=32, w=32, cin=64, cout=128, k=3, s=2, pad=1, images=WH | W3)),
    ("128x96", 0, dict(n=1, h=32, w=32, cin=64, cout=96, k=3, s=2, pad=1, images=WH | W3)),
    # weights beyond the staged kernels' 32-bit offsets (Ng x K = 2^32): the fp32 MFMA kernel
    ("f32", 0, dict(n=1, h=2, w=2, cin=65536, cout=65536, images=WH, has_ascale=1)),
    ("f32", 0, dict(n=1, h=2, w=2, cin=65536, cout=65536, s=2, images=WH)),
    # fp32 path
    ("skinny", 0, dict(n=1, h=1, w=8, cin=256, cout=512, images=0, allow_skinny=1, split=0)),
    ("skinny", 0, dict(n=1, h=1, w=32, cin=2048, cout=512, images=0, allow_skinny=1, split=0)),
    ("128x128", 0, dict(n=1, h=1, w=8, cin=256, cout=512, images=0, split=0)),                     # image layers never set allow_skinny
    ("128x128", 0, dict(n=1, h=1, w=33, cin=256, cout=512, images=0, allow_skinny=1, split=0)),   # M > 32
    ("128x32", 0, dict(n=1, h=16, w=16, cin=64, cout=32, images=0, split=0)),
    ("128x64", 0, dict(n=1, h=16, w=16, cin=64, cout=64, images=0, split=0)),
    ("128x96", 0, dict(n=1, h=16, w=16, cin=64, cout=96, images=0, split=0)),
    ("128x96", 0, dict(n=1, h=16, w=16, cin=64, cout=192, images=0, split=0)),                    # fewest padded columns: 2 x 96 < 2 x 128
    ("128x128", 0, dict(n=1, h=16, w=16, cin=64, cout=128, images=0, split=0)),
]
ALL_NAMES = {"stream", "c3h1", "c9h1", "direct", "h1w256x128", "dma16w256x128", "dma256x128", "256x128", "128x96", "256x64", "128x32", "128x64",
             "f32", "skinny", "128x128"}
CODES = {"direct": 1, "stream": 2, "c3h1": 3, "c9h1": 4}      # rd_debug_conv's *used_direct; every other route reports 0


def test_conv_route_table():
    lib = _load()
    got = [conv_route(lib, **kw) for _, _, kw in CONV_TABLE]
    assert [g[0] for g in got] == [name for name, _, _ in CONV_TABLE]
    assert {g[0] for g in got} == ALL_NAMES, "one case per route"
    split_tiles = {name for name, _, kw in CONV_TABLE if kw.get("split", 1) and "x" in name and name[0].isdigit()}
    assert split_tiles == {"256x128", "128x96", "256x64", "128x32", "128x64"}
    fp32_tiles = {name for name, _, kw in CONV_TABLE if not kw.get("split", 1)} - {"skinny"}
    assert fp32_tiles == {"128x32", "128x64", "128x96", "128x128"}


def test_conv_route_maps_to_the_codes_rd_debug_conv_reports():
    lib = _load()
    for name, code, kw in CONV_TABLE:
        assert code == CODES.get(name, 0)
        assert conv_route(lib, **kw) == (name, code), kw
    assert lib.rd_debug_conv_route(0, 1, 1, 4, 4, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, None, 0) == -1


def test_ascale_moves_every_pointwise_case_to_a_tile():
    lib = _load()
    for name, _, kw in CONV_TABLE:
        if name in ("h1w256x128", "dma256x128", "dma16w256x128"):
            assert conv_route(lib, **{**kw, "has_ascale": 1})[0] == "256x128", kw


# ------------------------------------------------------------------------------------------------------------------------------ depthwise
def lds_variant(h, c, k, sh):
    """the (H, C, SH) rows dwconv_lds_variant lists (kernels_dw_lds.hip), 3x3 only: 0 = none"""
    if k != 3:
        return 0
    if sh == 2:
        return 4 if h == 12 and c % 32 == 0 else 5 if h == 6 and c % 64 == 0 else 0
    return 1 if h == 6 and c % 64 == 0 else 2 if h == 12 and c % 32 == 0 else 3 if h == 3 and c % 64 == 0 else 0


def dw_sweep(lib, lds_on=True):
    """the violations of the sweep's properties (empty = all hold), and the set of kernel names seen"""
    bad, seen = [], set()
    for k, sh, h, w, c in itertools.product(("ragged", 3, 5, 7), (1, 2), (3, 6, 12, 20), (9, 17, 40), (8, 32, 64, 96, 192)):
        ragged = int(k == "ragged")
        kk = 1 if ragged else k
        row = (k, sh, h, w, c)
        want_lds = 0 if ragged or not lds_on else lds_variant(h, c, kk, sh)
        for has_line_w, wants_gap in itertools.product((0, 1), (0, 1)):
            name, chunks, planned = dw_route(lib, h, w, c, kk, sh, ragged, has_line_w, wants_gap)
            seen.add(name)
            if wants_gap and chunks != planned:
                bad.append(("the planner's chunk count is not the launch's", row, has_line_w, name, chunks, planned))
            if wants_gap and name.startswith("kxk_lds"):
                bad.append(("kxk_lds with the gap wanted", row, has_line_w, name))
            if ragged and name != "pixel":
                bad.append(("a ragged op off the pixel kernel", row, name))
            if name.startswith("lds") != bool(want_lds) or (want_lds and name != "lds%d" % want_lds):
                bad.append(("lds variant", row, name, want_lds))
            want_kxk = lds_on and not ragged and kk in (5, 7) and sh == 1 and c % 32 == 0 and not has_line_w and not wants_gap
            if name.startswith("kxk_lds") != want_kxk or (want_kxk and name != "kxk_lds%d" % kk):
                bad.append(("kxk_lds", row, has_line_w, wants_gap, name))
    return bad, seen


def test_dw_route_sweep():
    bad, seen = dw_sweep(_load())
    assert bad == []
    assert seen == {"pixel", "lds1", "lds2", "lds3", "lds4", "lds5", "kxk_lds5", "kxk_lds7", "tiled4", "tiled8"}


def test_dw_route_sweep_under_switches():
    """RD_DW_LDS and RD_DW_COL are read once per process: a fresh interpreter each"""
    for switch, names in (({"RD_DW_LDS": "0"}, {"pixel", "tiled4", "tiled8"}), ({"RD_DW_COL": "1"}, None)):
        env = {k: v for k, v in os.environ.items() if k not in ("RD_DW_LDS", "RD_DW_COL")}
        r = subprocess.run([sys.executable, __file__], env={**env, **switch}, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-800:]
        out = json.loads(r.stdout.strip().splitlines()[-1])
        assert out["bad"] == [], switch
        if names is not None:
            assert set(out["seen"]) == names
        else:
            assert "col" in out["seen"]


if __name__ == "__main__":
    bad_, seen_ = dw_sweep(_load(), lds_on=os.environ.get("RD_DW_LDS") != "0")
    print(json.dumps({"bad": bad_, "seen": sorted(seen_)}))
