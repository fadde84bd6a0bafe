"""CPU: the host side of the PP-OCRv5 mobile detector (`ppocrv5_det_mobile`) - kind selection by stem / tensor names, the reference-minted
fixtures and their summary, that the opt-in synthetic-weight gains of this kind leave every earlier manifest's tensors alone, and the
load-time folds (read back through the host-only entry rd_debug_derived_tensor) against float64 restatements from the state dict."""
import json

import numpy as np
import pytest

from kind_helpers import synth_state
from rapiddoc_amd import weights as W

KIND = "ppocrv5_det_mobile"
TAGS = ("b2_h64_w96", "b1_h160_w224", "b3_h96_w352", "b1_h960_w704")

# W.checksum(W.synth_state_dict(manifest, 0)) of every manifest that existed before this kind, recorded from the parent commit
PARENT_CHECKSUMS = {
    "ppocrv6_det": 14701.04590420073,
    "ppocrv6_rec": 17709.145076912035,
    "ppocrv5_rec_server": 46946.86280644165,
    "ppocrv5_rec_mobile": 61158.90317963697,
    "ppocrv5_det_server": 46393.608183482786,
    "pphgnetv2_b4": 45585.55140473513,
    "pphgnetv2_b6_formula": 166178.757858917,
    "ppformulanet_head_dec_a": 9853.409859141924,
    "ppformulanet_head_dec_b": 9855.135469193363,
    "ppformulanet_head_dec_long": 9864.32405567255,
    "ppformulanet_plus_m_m8": 176028.79909001882,
}


def _state(golden_dir):
    return synth_state(golden_dir, KIND, kind=KIND)


def test_kind_is_listed():
    from rapiddoc_amd.engine import DET_NECK_CHANNELS, KINDS
    assert KIND in KINDS and "ppocrv5_det_server" in KINDS and "ppocrv6_det" in KINDS
    assert DET_NECK_CHANNELS == {"ppocrv5_det_server": 256, KIND: 96}


def test_resolve_det_kind_by_stem_and_by_tensor_names(golden_dir):
    from rapiddoc_amd.session import DET_ARCH_BY_STEM_V5_MOBILE, resolve_det_kind
    assert DET_ARCH_BY_STEM_V5_MOBILE == {"ch_PP-OCRv5_det_mobile": KIND}
    assert resolve_det_kind("/some/dir/ch_PP-OCRv5_det_mobile.safetensors") == KIND
    assert resolve_det_kind("ch_PP-OCRv5_det_mobile.pth") == KIND
    assert resolve_det_kind("ch_PP-OCRv5_det_server.safetensors") == "ppocrv5_det_server"
    assert resolve_det_kind("ch_PP-OCRv6_det_small.safetensors") == "ppocrv6_det"
    with pytest.raises(ValueError) as e:
        resolve_det_kind("ch_PP-OCRv4_det_mobile.safetensors")
    for stem in ("ch_PP-OCRv5_det_mobile", "ch_PP-OCRv5_det_server", "ch_PP-OCRv6_det_small"):
        assert stem in str(e.value)                                    # the message lists every served stem
    for kind in (KIND, "ppocrv5_det_server", "ppocrv6_det"):
        names = [n for n, _, _ in W.load_manifest(golden_dir / f"manifest_{kind}.json")]
        assert resolve_det_kind({n: None for n in names}) == kind
        assert resolve_det_kind({"model." + n: None for n in names}) == kind
    small = {"model.backbone.layer_list.0.weight": np.zeros((12, 48, 1, 1), np.float32),
             "model.head.binarize.conv1.weight": np.zeros((24, 96, 3, 3), np.float32)}
    assert resolve_det_kind(W.to_safetensors_bytes(small)) == KIND
    assert resolve_det_kind({k[len("model."):]: v for k, v in small.items()}) == KIND
    # the server detector carries head.binarize.conv1 too: its own head decides
    assert resolve_det_kind({**small, "model.head.cbn_layer.last_1.weight": None}) == "ppocrv5_det_server"
    with pytest.raises(ValueError):
        resolve_det_kind({"head.binarize.conv1.weight": None})          # the DB head alone (a MobileNetV3 detector) is not served
    with pytest.raises(ValueError):
        resolve_det_kind({"head.something_else.weight": None})


def test_manifest_and_summary_checksum(golden_dir):
    man = W.load_manifest(golden_dir / f"manifest_{KIND}.json")
    summary = json.loads((golden_dir / "summary_det_mobile.json").read_text())
    assert len(man) == summary["tensors"] == 1055
    assert summary["parameters"] == sum(int(np.prod(s)) for _n, s, d in man if d == "float32")    # every branch and BatchNorm statistic counted
    names = {n for n, _, _ in man}
    assert {"head.thresh.conv1.weight", "backbone.layer_list.3.weight", "neck.inp_conv.3.se_block.conv2.bias", "backbone.blocks3.0.dw_conv.act.lab.scale",
            "backbone.blocks6.1.se.conv1.weight"} <= names
    assert "backbone.blocks3.0.dw_conv.identity.weight" not in names and "backbone.blocks3.1.dw_conv.identity.weight" in names
    assert W.checksum(_state(golden_dir)) == summary["checksum"]
    assert W.checksum(W.synth_state_dict(man, 0)) != summary["checksum"]   # the gains are opt-in
    with pytest.raises(ValueError):
        W.synth_state_dict(man, 0, kind="no_such_kind")


def test_summary_meets_the_mint_conditions(golden_dir):
    summary = json.loads((golden_dir / "summary_det_mobile.json").read_text())
    assert set(summary["fixtures"]) == set(TAGS)
    for tag, s in summary["fixtures"].items():
        assert s["maps_share_05_95"] >= 0.75, (tag, s)
        assert s["maps_std"] >= 0.15, (tag, s)
        assert s["fuse_absmax"] > 0
        assert s["x_seed"] >= 300 + int(tag.rsplit("_w", 1)[1])


def test_fixture_files_are_small_and_complete(golden_dir):
    for tag in TAGS:
        f = golden_dir / f"det5m_seed0_{tag}.npz"
        assert f.stat().st_size <= 1 << 20, (tag, f.stat().st_size)
        g = np.load(f)
        assert str(g["x_kind"]) == "pm1"
        B, _, H, W_ = (int(v) for v in g["x_shape"])
        ps = int(g["maps_ps"])
        assert ps % 2 == 1
        for k in ("maps", "shrink_logit"):
            assert g[k].shape == (B, 1, -(-H // ps), -(-W_ // ps)), (tag, k)
        cs, p = int(g["fuse_cs"]), int(g["fuse_ps"])
        assert g["fuse"].shape == (B, -(-96 // cs), -(-(H // 4) // p), -(-(W_ // 4) // p)), tag
        assert p % 2 == 1          # odd pixel strides meet every row / column parity
        m = 1 / (1 + np.exp(-g["shrink_logit"].astype(np.float64)))
        assert np.abs(m - g["maps"]).max() < 1e-6


@pytest.mark.parametrize("kind", sorted(PARENT_CHECKSUMS))
def test_earlier_manifests_are_untouched_by_the_new_gains(golden_dir, kind):
    man = W.load_manifest(golden_dir / f"manifest_{kind}.json")
    assert W.checksum(W.synth_state_dict(man, 0)) == PARENT_CHECKSUMS[kind]


# ---------------------------------------------------------------------------------------------------------------- load-time folds
def _derived(blob, name, shape):
    from rapiddoc_amd import _lib
    lib = _lib.load()
    fn = lib.rd_debug_derived_tensor
    out = np.full(shape, np.nan, np.float32)
    n = fn(KIND.encode(), blob, len(blob), name.encode(), out.ctypes.data, out.size)
    assert n == out.size, (name, n, shape)
    return out


def test_the_derived_tensor_entry_serves_this_kind_only(golden_dir):
    from rapiddoc_amd import _lib
    fn = _lib.load().rd_debug_derived_tensor
    blob = W.to_safetensors_bytes(_state(golden_dir))
    assert fn(b"ppocrv5_rec_mobile", blob, len(blob), b"backbone.blocks2.0.dw_conv.fold.weight", None, 0) == -1
    assert fn(KIND.encode(), blob, len(blob), b"no.such.tensor", None, 0) == -1
    assert fn(KIND.encode(), blob, len(blob), b"backbone.blocks2.0.dw_conv.fold.weight", None, 0) == 16 * 9


@pytest.fixture(scope="module")
def state_and_blob(golden_dir):
    st = _state(golden_dir)
    return st, W.to_safetensors_bytes(st)


@pytest.mark.parametrize("level,k", [(0, 48), (1, 96), (2, 192), (3, 384)])
def test_layer_list_and_ins_conv_fold_into_one_1x1(state_and_blob, level, k):
    """W = W_ins W_ll and b = W_ins b_ll against float64: one rounding of the exact product, so half an ulp of the largest entry (2^-24
    relative) plus the double sum's own error, far below it - bound 2^-23 max |ref|."""
    st, blob = state_and_blob
    wl = st[f"backbone.layer_list.{level}.weight"].astype(np.float64)[:, :, 0, 0]
    bl = st[f"backbone.layer_list.{level}.bias"].astype(np.float64)
    wi = st[f"neck.ins_conv.{level}.in_conv.weight"].astype(np.float64)[:, :, 0, 0]
    assert wl.shape[1] == k and wi.shape == (96, wl.shape[0])
    w = _derived(blob, f"neck.ins_conv.{level}.fold.weight", (96, k, 1, 1))[:, :, 0, 0]
    b = _derived(blob, f"neck.ins_conv.{level}.fold.bias", (96,))
    ref_w, ref_b = wi @ wl, wi @ bl
    e_w, e_b = np.abs(w - ref_w).max(), np.abs(b - ref_b).max()
    print(f"\n[ins fold level {level}] max |W - fp64| = {e_w:.3e} (max |ref| {np.abs(ref_w).max():.3f}), max |b - fp64| = {e_b:.3e}")
    assert e_w <= 2.0 ** -23 * np.abs(ref_w).max() and e_b <= 2.0 ** -23 * max(np.abs(ref_b).max(), 1e-30)
    # the two 1x1s applied one after the other to a feature vector, in float64, against the folded layer
    x = np.random.default_rng(level).uniform(-4, 4, (k, 64))
    two = wi @ (wl @ x + bl[:, None])
    one = w.astype(np.float64) @ x + b.astype(np.float64)[:, None]
    assert np.abs(one - two).max() <= 1e-5 * max(1.0, np.abs(two).max())


def _fold_fp64(st, p, depthwise):
    """lab(sum_i BN_i(conv_i) + BN_1x1(conv_1x1) [+ BN_id]) of one LearnableRepLayer as (weight, bias) in float64 - and nothing of `act`"""
    def bn(q):
        g, be, m, v = (st[f"{q}.{n}"].astype(np.float64) for n in ("weight", "bias", "running_mean", "running_var"))
        s = g / np.sqrt(v + 1e-5)
        return s, be - m * s
    w0 = st[f"{p}.conv_kxk.0.conv.weight"].astype(np.float64)
    k = w0.shape[2]
    w, b = np.zeros_like(w0), np.zeros(w0.shape[0])
    i = 0
    while f"{p}.conv_kxk.{i}.conv.weight" in st:
        s, sh = bn(f"{p}.conv_kxk.{i}.bn")
        w += st[f"{p}.conv_kxk.{i}.conv.weight"].astype(np.float64) * s[:, None, None, None]
        b += sh
        i += 1
    if f"{p}.conv_1x1.conv.weight" in st:
        s, sh = bn(f"{p}.conv_1x1.bn")
        w[:, :, k // 2, k // 2] += st[f"{p}.conv_1x1.conv.weight"].astype(np.float64)[:, :, 0, 0] * s[:, None]
        b += sh
    if f"{p}.identity.weight" in st:
        s, sh = bn(f"{p}.identity")
        for o in range(w.shape[0]):
            w[o, 0 if depthwise else o, k // 2, k // 2] += s[o]
        b += sh
    ls, lb = float(st[f"{p}.lab.scale"][0]), float(st[f"{p}.lab.bias"][0])
    return w * ls, b * ls + lb


@pytest.mark.parametrize("layer,shape,depthwise", [
    ("backbone.blocks3.0.dw_conv", (32, 1, 3, 3), True),     # stride 2: no identity branch; its act.lab is in the file and must not be folded in
    ("backbone.blocks3.0.pw_conv", (48, 32, 1, 1), False),
    ("backbone.blocks3.1.dw_conv", (48, 1, 3, 3), True),     # stride 1: the identity BatchNorm on the centre tap
    ("backbone.blocks6.0.dw_conv", (192, 1, 5, 5), True),
    ("backbone.blocks6.3.pw_conv", (384, 384, 1, 1), False),  # cin == cout: the identity of a pointwise layer
])
def test_rep_layer_fold_matches_fp64(state_and_blob, layer, shape, depthwise):
    st, blob = state_and_blob
    stride2 = layer in ("backbone.blocks3.0.dw_conv", "backbone.blocks6.0.dw_conv")
    assert (f"{layer}.identity.weight" in st) == (not stride2 and (depthwise or shape[0] == shape[1]))    # only where cin == cout and stride 1
    assert f"{layer}.act.lab.scale" in st                             # present for every layer, the stride-2 ones included
    ref_w, ref_b = _fold_fp64(st, layer, depthwise)
    w = _derived(blob, layer + ".fold.weight", shape)
    b = _derived(blob, layer + ".fold.bias", (shape[0],))
    e_w, e_b = np.abs(w - ref_w).max(), np.abs(b - ref_b).max()
    print(f"\n[{layer}] max |W - fp64| = {e_w:.3e} (max |ref| {np.abs(ref_w).max():.3f}), max |b - fp64| = {e_b:.3e} (max |ref| {np.abs(ref_b).max():.3f})")
    assert e_w <= 2.0 ** -23 * np.abs(ref_w).max() and e_b <= 2.0 ** -23 * np.abs(ref_b).max()
    # had act.lab been multiplied in, the fold would be off by its scale (0.8 .. 1.2, never exactly 1 here)
    a = float(st[f"{layer}.act.lab.scale"][0])
    assert abs(a - 1.0) > 1e-3 and np.abs(w - ref_w * a).max() > 100 * max(e_w, 1e-12)
