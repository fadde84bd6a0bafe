"""CPU: the host side of the UniTable table-structure encoder (`unitable_encoder`: ViT-B, 12 pre-norm layers of d = 768 and 12 heads of 64) -
the reference-minted fixtures and their summary, the manifest, a float64 restatement of the graph the engine runs (the patch gather in
front of one GEMM, packed in_proj, erf GELU) against the fixtures, the kind lists and the C-ABI symbols."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import unitable_reference as R
from rapiddoc_amd import weights as W

ROOT = Path(__file__).resolve().parents[1]


def test_manifest_is_the_reference_encoder(golden_dir):
    man = W.load_manifest(golden_dir / f"manifest_{R.KIND}.json")
    summary = json.loads((golden_dir / "summary_unitable.json").read_text())
    assert len(man) == 149 == summary["tensors"]
    assert sum(int(np.prod(s)) for _, s, _ in man) == 86_433_024 == summary["parameters"]
    shapes = {n: s for n, s, _ in man}
    assert shapes["backbone.conv_proj.weight"] == (768, 3, 16, 16) and shapes["pos_embed.embedding.weight"] == (1024, 768)
    for i in range(12):
        p = f"encoder.layers.{i}."
        assert shapes[p + "self_attn.in_proj_weight"] == (2304, 768) and shapes[p + "self_attn.in_proj_bias"] == (2304,)
        assert shapes[p + "self_attn.out_proj.weight"] == (768, 768)
        assert shapes[p + "linear1.weight"] == (3072, 768) and shapes[p + "linear2.weight"] == (768, 3072)
        assert shapes[p + "norm1.weight"] == shapes[p + "norm2.bias"] == (768,)
    assert shapes["norm.weight"] == (768,)
    assert all(d == "float32" for _, _, d in man)


def test_synthetic_weights_are_pinned_and_every_layernorm_gain_is_a_gain(golden_dir):
    st = R.state(golden_dir)
    summary = json.loads((golden_dir / "summary_unitable.json").read_text())
    assert W.checksum(st) == pytest.approx(summary["checksum"], rel=0, abs=1e-6)
    for name, v in st.items():
        if name.endswith(("norm1.weight", "norm2.weight")) or name == "norm.weight":
            assert 0.8 <= float(v.min()) and float(v.max()) <= 1.2, name


def test_fixtures_hold_what_the_summary_says(golden_dir):
    summary = json.loads((golden_dir / "summary_unitable.json").read_text())
    assert set(summary["fixtures"]) == set(R.TAGS)
    for tag in R.TAGS:
        x, g = R.fixture(golden_dir, tag)
        B, _, H, W_ = x.shape
        T = (H // 16) * (W_ // 16)
        assert T == summary["fixtures"][tag]["T"]
        for name in R.TAPS:
            ts, cs = int(g[name + "_ts"]), int(g[name + "_cs"])
            assert ts % 2 == 1 and g[name].shape == (B, -(-T // ts), -(-768 // cs)) and g[name].dtype == np.float32
        assert (golden_dir / f"unitable_enc_seed0_{tag}.npz").stat().st_size <= 1 << 20
        assert summary["fixtures"][tag]["taps"]["memory"]["std"] > 0.5          # the output is alive
    assert sorted(summary["fixtures"][t]["T"] for t in R.TAGS) == [6, 39, 68, 784]   # one tile, < a tile, across a 64-key tile, the product shape


@pytest.mark.parametrize("tag", R.TAGS)
def test_float64_restatement_of_the_engine_graph_matches_the_fixtures(golden_dir, tag):
    torch.set_num_threads(8)
    x, g = R.fixture(golden_dir, tag)
    out = R.encoder_forward(R.state(golden_dir), x)
    msgs = []
    for name in R.TAPS:
        ref = torch.from_numpy(g[name]).double()
        err = float((R.sub(out[name], g, name) - ref).abs().max())
        bound = R.FIXTURE_TOL * max(1.0, float(ref.abs().max()))
        msgs.append(f"{name} {err:.2e} / {bound:.2e}")
        assert err <= bound, (tag, name, err, bound)
    print(f"\n[unitable encoder {tag} float64 restatement] " + ", ".join(msgs))


def test_patch_rows_are_the_convolution(golden_dir):
    """the gather order of the restatement (and of vit_patchify_kernel) against F.conv2d itself, with an asymmetric weight"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 3, 32, 48), generator=g, dtype=torch.float64)
    w = torch.randn((8, 3, 16, 16), generator=g, dtype=torch.float64)
    ref = torch.nn.functional.conv2d(x, w, stride=16).flatten(2).transpose(1, 2)
    got = R.patch_rows(x) @ w.reshape(8, -1).T
    assert float((got - ref).abs().max()) < 1e-10


def test_the_kind_is_listed_everywhere():
    from rapiddoc_amd import _lib, engine
    assert R.KIND in engine.KINDS
    from rapiddoc_amd import build as rd_build
    rd_build.build(verbose=False)
    lib = _lib.load()
    h = lib.rd_create(0, R.KIND.encode())       # registered in the engine's model table: the kind is looked up before the device
    if h:
        lib.rd_destroy(h)
    else:
        assert b"unknown model kind" not in lib.rd_create_error(), lib.rd_create_error()
    header = (ROOT / "include/rapiddoc_mi355.h").read_text()
    assert f'"{R.KIND}"' in header and re.search(r"\brd_table_encoder_forward\s*\(", header)
    assert "rd_table_encoder_forward" in _lib.SYMBOLS
    assert "kernels_vit_attn.hip" in __import__("rapiddoc_amd.build", fromlist=["SOURCES"]).SOURCES


def test_the_library_exports_the_entries():
    from rapiddoc_amd import build as rd_build
    rd_build.build(verbose=False)
    from rapiddoc_amd import _lib
    lib = _lib.load()
    for name in ("rd_table_encoder_forward", "rd_debug_table_encoder_taps", "rd_debug_vit_attention", "rd_debug_td_gemv", "rd_debug_td_attention",
                 "rd_debug_td_select"):
        assert hasattr(lib, name), name
