"""CPU: the host side of the PP-OCRv3 multilingual detector (`ppocrv3_det_mobile`: MobileNetV3 large scale 0.5 without SE + RSEFPN +
DBHead; the files multi_PP-OCRv3_det_mobile and en_PP-OCRv3_det_mobile) - kind selection by stem / tensor names, the reference-minted
fixtures and their summary, the opt-in synthetic-weight gains, the load-time Conv + BatchNorm folds (read back through the host-only entry
rd_debug_derived_tensor) against float64, and a float64 restatement of the FOLDED graph - the graph the engine runs - against the
fixtures."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kind_helpers import hswish64, synth_state
from rapiddoc_amd import weights as W

KIND = "ppocrv3_det_mobile"
TAGS = ("b2_h64_w96", "b1_h160_w224", "b3_h96_w352", "b1_h960_w704")
STEMS = ("multi_PP-OCRv3_det_mobile", "en_PP-OCRv3_det_mobile")
# (stage, index, k, cin, mid, cout, stride, act) of the fifteen inverted-residual blocks, as probed on the reference
BLOCKS = [(0, 0, 3, 8, 8, 8, 1, "relu"), (0, 1, 3, 8, 32, 16, 2, "relu"), (0, 2, 3, 16, 40, 16, 1, "relu"),
          (1, 0, 5, 16, 40, 24, 2, "relu"), (1, 1, 5, 24, 64, 24, 1, "relu"), (1, 2, 5, 24, 64, 24, 1, "relu"),
          (2, 0, 3, 24, 120, 40, 2, "hswish"), (2, 1, 3, 40, 104, 40, 1, "hswish"), (2, 2, 3, 40, 96, 40, 1, "hswish"),
          (2, 3, 3, 40, 96, 40, 1, "hswish"), (2, 4, 3, 40, 240, 56, 1, "hswish"), (2, 5, 3, 56, 336, 56, 1, "hswish"),
          (3, 0, 5, 56, 336, 80, 2, "hswish"), (3, 1, 5, 80, 480, 80, 1, "hswish"), (3, 2, 5, 80, 480, 80, 1, "hswish")]

# W.checksum(W.synth_state_dict(manifest, 0)) of every manifest that existed before this kind (tests/test_det_mobile_host.py holds the
# same table for the kinds before the v5 mobile detector), and with their own opt-in gains the two kinds that have some
EARLIER_CHECKSUMS = {
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
    from rapiddoc_amd.engine import DET_NECK_CHANNELS, DET_NECK_CHANNELS_V3_MOBILE, KINDS
    assert KIND in KINDS and "ppocrv5_det_mobile" in KINDS
    assert DET_NECK_CHANNELS_V3_MOBILE == {KIND: 96} and KIND not in DET_NECK_CHANNELS


def test_resolve_det_kind_by_stem_and_by_tensor_names(golden_dir):
    from rapiddoc_amd.session import DET_ARCH_BY_STEM, DET_ARCH_BY_STEM_V3_MOBILE, DET_ARCH_BY_STEM_V5_MOBILE, resolve_det_kind
    assert DET_ARCH_BY_STEM_V3_MOBILE == {s: KIND for s in STEMS}
    for stem in STEMS:
        assert resolve_det_kind(f"/some/dir/{stem}.safetensors") == KIND
        assert resolve_det_kind(f"{stem}.pth") == KIND
    assert resolve_det_kind("ch_PP-OCRv5_det_mobile.safetensors") == "ppocrv5_det_mobile"
    for v4 in ("ch_PP-OCRv4_det_mobile", "ch_PP-OCRv4_det_server"):
        with pytest.raises(ValueError) as e:
            resolve_det_kind(v4 + ".safetensors")
        for stem in (*DET_ARCH_BY_STEM, *DET_ARCH_BY_STEM_V5_MOBILE, *STEMS):
            assert stem in str(e.value)                                 # the message lists every served stem
    names = [n for n, _, _ in W.load_manifest(golden_dir / f"manifest_{KIND}.json")]
    assert resolve_det_kind({n: None for n in names}) == KIND
    assert resolve_det_kind({"model." + n: None for n in names}) == KIND
    small = {"model.backbone.stages.0.0.expand_conv.conv.weight": np.zeros((8, 8, 1, 1), np.float32),
             "model.head.binarize.conv1.weight": np.zeros((24, 96, 3, 3), np.float32)}
    assert resolve_det_kind(W.to_safetensors_bytes(small)) == KIND
    assert resolve_det_kind({**small, "model.head.cbn_layer.last_1.weight": None}) == "ppocrv5_det_server"   # its own head decides
    with pytest.raises(ValueError):
        resolve_det_kind({"head.binarize.conv1.weight": None})          # the DB head alone names no backbone
    with pytest.raises(ValueError):
        resolve_det_kind({"backbone.stages.0.0.expand_conv.conv.weight": None})
    for kind in ("ppocrv5_det_mobile", "ppocrv5_det_server", "ppocrv6_det"):   # the other kinds resolve as before
        other = [n for n, _, _ in W.load_manifest(golden_dir / f"manifest_{kind}.json")]
        assert resolve_det_kind({n: None for n in other}) == kind


def test_manifest_and_summary_checksum(golden_dir):
    man = W.load_manifest(golden_dir / f"manifest_{KIND}.json")
    summary = json.loads((golden_dir / "summary_det_v3_mobile.json").read_text())
    assert len(man) == summary["tensors"] == 352
    assert summary["parameters"] == 603418
    names = {n for n, _, _ in man}
    assert {"backbone.conv.conv.weight", "backbone.stages.3.3.bn.running_var", "head.thresh.conv1.weight", "neck.ins_conv.3.in_conv.weight"} <= names
    assert not any(".mid_se." in n or "layer_list" in n for n in names)          # no SE in the backbone, no layer_list in front of the neck
    for s, i, k, cin, mid, cout, stride, act in BLOCKS:
        p = f"backbone.stages.{s}.{i}"
        shapes = {n: sh for n, sh, _ in man}
        assert shapes[p + ".expand_conv.conv.weight"] == (mid, cin, 1, 1)
        assert shapes[p + ".bottleneck_conv.conv.weight"] == (mid, 1, k, k)
        assert shapes[p + ".linear_conv.conv.weight"] == (cout, mid, 1, 1)
    assert W.checksum(_state(golden_dir)) == summary["checksum"]
    assert W.checksum(W.synth_state_dict(man, 0)) != summary["checksum"]          # the gains are opt-in


def test_summary_meets_the_mint_conditions_and_fixtures_are_small_and_complete(golden_dir):
    summary = json.loads((golden_dir / "summary_det_v3_mobile.json").read_text())
    assert set(summary["fixtures"]) == set(TAGS)
    for tag, s in summary["fixtures"].items():
        assert s["maps_share_05_95"] >= 0.75 and s["maps_std"] >= 0.15, (tag, s)
        f = golden_dir / f"det3m_seed0_{tag}.npz"
        assert f.stat().st_size <= 1 << 20, (tag, f.stat().st_size)
        g = np.load(f)
        B, _, H, W_ = (int(v) for v in g["x_shape"])
        ps = int(g["maps_ps"])
        for k in ("maps", "shrink_logit"):
            assert g[k].shape == (B, 1, -(-H // ps), -(-W_ // ps)), (tag, k)
        for name, ch, red in (("fuse", 96, 4), ("stage0", 16, 4), ("stage1", 24, 8), ("stage2", 56, 16), ("stage3", 480, 32)):
            cs, p = int(g[name + "_cs"]), int(g[name + "_ps"])
            assert p % 2 == 1 and g[name].shape == (B, -(-ch // cs), -(-(H // red) // p), -(-(W_ // red) // p)), (tag, name)
        m = 1 / (1 + np.exp(-g["shrink_logit"].astype(np.float64)))
        assert np.abs(m - g["maps"]).max() < 1e-6


@pytest.mark.parametrize("kind", sorted(EARLIER_CHECKSUMS))
def test_earlier_manifests_are_untouched_by_the_new_gains(golden_dir, kind):
    man = W.load_manifest(golden_dir / f"manifest_{kind}.json")
    assert W.checksum(W.synth_state_dict(man, 0)) == EARLIER_CHECKSUMS[kind]


def test_the_earlier_kind_with_gains_keeps_its_summary(golden_dir):
    man = W.load_manifest(golden_dir / "manifest_ppocrv5_det_mobile.json")
    assert W.checksum(W.synth_state_dict(man, 0, kind="ppocrv5_det_mobile")) == json.loads((golden_dir / "summary_det_mobile.json").read_text())["checksum"]


# ---------------------------------------------------------------------------------------------------------------- load-time folds
def _derived_fn():
    from rapiddoc_amd import _lib
    fn = _lib.load().rd_debug_derived_tensor
    return fn


def _derived(blob, name, shape):
    out = np.full(shape, np.nan, np.float32)
    n = _derived_fn()(KIND.encode(), blob, len(blob), name.encode(), out.ctypes.data, out.size)
    assert n == out.size, (name, n, shape)
    return out


@pytest.fixture(scope="module")
def state_and_blob(golden_dir):
    st = _state(golden_dir)
    return st, W.to_safetensors_bytes(st)


def _fold_fp64(st, conv, bn):
    g, be, m, v = (st[f"{bn}.{n}"].astype(np.float64) for n in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(v + 1e-5)
    return st[conv + ".weight"].astype(np.float64) * s[:, None, None, None], be - m * s


@pytest.mark.parametrize("layer,shape", [
    ("backbone.stages.0.0.expand_conv", (8, 8, 1, 1)),
    ("backbone.stages.1.0.bottleneck_conv", (40, 1, 5, 5)),
    ("backbone.stages.2.5.linear_conv", (56, 336, 1, 1)),
])
def test_conv_bn_fold_is_within_one_rounding_of_fp64(state_and_blob, layer, shape):
    """weight * scale and beta - mean * scale computed in double and rounded once: half an ulp of the value, 2^-24 relative."""
    st, blob = state_and_blob
    ref_w, ref_b = _fold_fp64(st, layer + ".conv", layer + ".bn")
    w = _derived(blob, layer + ".fold.weight", shape)
    b = _derived(blob, layer + ".fold.bias", (shape[0],))
    assert np.array_equal(w, ref_w.astype(np.float32)) and np.array_equal(b, ref_b.astype(np.float32))
    assert np.all(np.abs(w - ref_w) <= 2.0 ** -24 * np.abs(ref_w)) and np.all(np.abs(b - ref_b) <= 2.0 ** -24 * np.abs(ref_b))


def test_the_derived_tensor_entry_knows_the_kind(state_and_blob):
    _st, blob = state_and_blob
    fn = _derived_fn()
    assert fn(KIND.encode(), blob, len(blob), b"backbone.stages.3.3.fold.weight", None, 0) == 480 * 80
    assert fn(KIND.encode(), blob, len(blob), b"no.such.tensor", None, 0) == -1
    assert fn(b"ppocrv5_det_mobile", blob, len(blob), b"backbone.stages.3.3.fold.weight", None, 0) == -1    # that kind's folds want its own tensors


def test_c_abi_accepts_the_kind_name():
    """Host only: rd_create reaches the device check (or succeeds) for this kind, and still names an unknown kind as unknown."""
    from rapiddoc_amd import _lib
    lib = _lib.load()
    for name in ("rd_debug_mbv3_dw", "rd_debug_mbv3_block", "rd_debug_mbv3_block_ok"):
        assert hasattr(lib, name)
    h = lib.rd_create(0, b"ppocrv3_det_mobile_x")
    assert not h and b"unknown model kind" in lib.rd_create_error()
    h = lib.rd_create(0, KIND.encode())
    if h:
        lib.rd_destroy(h)
    else:
        assert b"unknown model kind" not in lib.rd_create_error() and b"no HIP device" in lib.rd_create_error()


def test_block_launch_ok_refuses_what_the_kernel_does_not_serve():
    """Host only (rd_debug_mbv3_block_ok): every block of the 1/2, 1/4 and 1/8 levels but the 120-wide one is served, and each refusal."""
    from rapiddoc_amd import _lib
    fn = _lib.load().rd_debug_mbv3_block_ok

    def ok(N=2, H=9, W_=35, cin=16, mid=40, cout=16, K=3, S=1, act=1, shortcut=0, xld=None, yld=None):
        return fn(N, H, W_, cin, mid, cout, K, S, act, shortcut, cin if xld is None else xld, cout if yld is None else yld)

    for s, i, k, cin, mid, cout, stride, act in BLOCKS[:6]:
        assert ok(cin=cin, mid=mid, cout=cout, K=k, S=stride, shortcut=int(stride == 1 and cin == cout)) == 1
    assert ok(act=2) == 1 and ok(xld=24, yld=40) == 1
    assert ok(cin=24, mid=120, cout=40, K=3, S=2) == 0      # 147 KB of LDS
    assert ok(cin=80, mid=480, cout=80, K=5, S=1) == 0
    assert ok(K=7) == 0 and ok(K=4) == 0 and ok(S=3) == 0
    assert ok(cin=6) == 0 and ok(mid=36) == 0 and ok(cout=12) == 0
    assert ok(act=0) == 0 and ok(act=3) == 0
    assert ok(cout=24, shortcut=1) == 0 and ok(S=2, shortcut=1) == 0          # a shortcut needs stride 1 and cin == cout
    assert ok(xld=18) == 0 and ok(xld=8) == 0 and ok(yld=8) == 0
    assert ok(N=0) == 0 and ok(H=0) == 0
    assert ok(N=1 << 30, H=64, W_=64) == 0                                      # a grid beyond 2^31 workgroups


# ---------------------------------------------------------------------------------------------------------------- the folded graph in float64
def folded_graph_fp64(st, blob, x):
    """What the engine computes, restated in float64 from the FOLDED tensors (float32 values, as rounded at load time) and the rest of
    the state dict: conv1 + hardswish, fifteen blocks (expand + act, zero padding, depthwise + act, linear, shortcut), conv_last +
    hardswish, RSEFPN with the paddle hard-sigmoid (0.2 x + 0.5) gates and shortcuts, DBHead."""
    d = lambda a: torch.from_numpy(np.asarray(a)).double()
    t = lambda n: d(st[n])

    def fold(p, shape):
        return d(_derived(blob, p + ".fold.weight", shape)), d(_derived(blob, p + ".fold.bias", (shape[0],)))

    def bn(y, q):
        s = t(q + ".weight") / torch.sqrt(t(q + ".running_var") + 1e-5)
        return y * s[None, :, None, None] + (t(q + ".bias") - t(q + ".running_mean") * s)[None, :, None, None]

    def rse(y, p):
        g = y.mean((2, 3), keepdim=True)
        g = F.relu(F.conv2d(g, t(p + ".se_block.conv1.weight"), t(p + ".se_block.conv1.bias")))
        g = torch.clamp(0.2 * F.conv2d(g, t(p + ".se_block.conv2.weight"), t(p + ".se_block.conv2.bias")) + 0.5, 0.0, 1.0)
        return y + y * g

    h = hswish64(bn(F.conv2d(d(x), t("backbone.conv.conv.weight"), stride=2, padding=1), "backbone.conv.bn"))
    feats = []
    for n, (s, i, k, cin, mid, cout, stride, act) in enumerate(BLOCKS):
        if stride == 2 and n > 2:
            feats.append(h)
        a = F.relu if act == "relu" else hswish64
        p = f"backbone.stages.{s}.{i}"
        e = a(F.conv2d(h, *fold(p + ".expand_conv", (mid, cin, 1, 1))))
        w, b = fold(p + ".bottleneck_conv", (mid, 1, k, k))
        dw = a(F.conv2d(F.pad(e, (k // 2,) * 4), w, b, stride=stride, groups=mid))
        y = F.conv2d(dw, *fold(p + ".linear_conv", (cout, mid, 1, 1)))
        h = h + y if stride == 1 and cin == cout else y
    feats.append(hswish64(F.conv2d(h, *fold("backbone.stages.3.3", (480, 80, 1, 1)))))
    ins = [rse(F.conv2d(f, t(f"neck.ins_conv.{i}.in_conv.weight")), f"neck.ins_conv.{i}") for i, f in enumerate(feats)]
    for i in (2, 1, 0):
        ins[i] = ins[i] + F.interpolate(ins[i + 1], scale_factor=2, mode="nearest")
    ps = [rse(F.conv2d(ins[i], t(f"neck.inp_conv.{i}.in_conv.weight"), padding=1), f"neck.inp_conv.{i}") for i in range(4)]
    fuse = torch.cat([F.interpolate(ps[3], scale_factor=8, mode="nearest"), F.interpolate(ps[2], scale_factor=4, mode="nearest"),
                      F.interpolate(ps[1], scale_factor=2, mode="nearest"), ps[0]], 1)
    c = F.relu(bn(F.conv2d(fuse, t("head.binarize.conv1.weight"), padding=1), "head.binarize.conv_bn1"))
    c = F.relu(bn(F.conv_transpose2d(c, t("head.binarize.conv2.weight"), t("head.binarize.conv2.bias"), stride=2), "head.binarize.conv_bn2"))
    logit = F.conv_transpose2d(c, t("head.binarize.conv3.weight"), t("head.binarize.conv3.bias"), stride=2)
    return feats, fuse, logit, torch.sigmoid(logit)


@pytest.mark.parametrize("tag", TAGS)
def test_the_folded_graph_in_fp64_reproduces_the_fixtures(state_and_blob, golden_dir, tag):
    """Bound 1e-3 * max(1, max |ref|) per tensor, the project's bound for a whole network against its fixture."""
    st, blob = state_and_blob
    g = np.load(golden_dir / f"det3m_seed0_{tag}.npz")
    x = np.random.default_rng(int(g["x_seed"])).uniform(-1.0, 1.0, tuple(int(v) for v in g["x_shape"])).astype(np.float32)
    torch.set_num_threads(4)
    feats, fuse, logit, maps = folded_graph_fp64(st, blob, x)
    got = {"maps": maps, "shrink_logit": logit, "fuse": fuse, **{f"stage{i}": f for i, f in enumerate(feats)}}
    for name, y in got.items():
        ref = g[name].astype(np.float64)
        cs = int(g[name + "_cs"]) if name + "_cs" in g else 1
        ps = int(g[name + "_ps"]) if name + "_ps" in g else int(g["maps_ps"])
        e = float(np.abs(y[:, ::cs, ::ps, ::ps].numpy() - ref).max())
        bound = 1e-3 * max(1.0, float(np.abs(ref).max()))
        print(f"\n[det v3 mobile {tag} fp64 folded graph] {name}: max-abs error {e:.3e} (bound {bound:.3e})")
        assert e <= bound, name
