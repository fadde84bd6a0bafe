"""CPU: the host side of the multilingual PP-OCRv3 / v4 mobile recognisers (`model_kind "ppocr_rec_mv1e"`: MobileNetV1Enhance scale 0.5 + SVTR
neck dims 64 + CTCHead): how the session tells the kind (ten stems, tensor names), the manifests and fixtures against their summary
(tests/golden/make_golden_rec_mv1e.py), that the synthetic-weight gains are opt-in, a float64 restatement of the FOLDED graph the engine
runs (BatchNorm folded into weight + bias, hardswish applied by the consumer, the neck's 3 x 3 convolutions cut to their middle row, the
pool over rows 0-1, the SE gate) against the fixtures, and dictionaries with multi-codepoint entries."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from kind_helpers import golden_x, hswish64
from rapiddoc_amd import ocr_host
from rapiddoc_amd import weights as W

KIND = "ppocr_rec_mv1e"
STEMS = ["latin_PP-OCRv3_rec_mobile", "cyrillic_PP-OCRv3_rec_mobile", "chinese_cht_PP-OCRv3_rec_mobile", "arabic_PP-OCRv4_rec_mobile",
         "korean_PP-OCRv4_rec_mobile", "japan_PP-OCRv4_rec_mobile", "ta_PP-OCRv4_rec_mobile", "te_PP-OCRv4_rec_mobile", "ka_PP-OCRv4_rec_mobile",
         "devanagari_PP-OCRv4_rec_mobile"]
FIXTURES = [("korean", "b2_w320", (2, 3, 48, 320)), ("korean", "b1_w96", (1, 3, 48, 96)), ("korean", "b3_w640", (3, 3, 48, 640)),
            ("korean", "b6_w1088", (6, 3, 48, 1088)), ("latin", "b6_w1088", (6, 3, 48, 1088)), ("latin", "b1_w96", (1, 3, 48, 96))]
CLASSES = {"korean": 3690, "latin": 187}
# W.checksum(W.synth_state_dict(manifest, 0)) of every manifest that existed before this kind, recorded from the parent commit
PARENT_CHECKSUMS = {
    "ppocrv6_det": 14701.04590420073,
    "ppocrv6_rec": 17709.145076912035,
    "ppocrv5_rec_server": 46946.86280644165,
    "ppocrv5_rec_mobile": 61158.90317963697,
    "ppocrv5_det_server": 46393.608183482786,
    "pphgnetv2_b4": 45585.55140473513,
    "pphgnetv2_b6_formula": 166178.757858917,
}


def _manifest(golden_dir, lang):
    return W.load_manifest(golden_dir / f"manifest_{KIND}_{lang}.json")


def _summary(golden_dir):
    return json.loads((golden_dir / "summary_rec_mv1e.json").read_text())


def test_the_kind_is_offered():
    from rapiddoc_amd.engine import KINDS
    assert KIND in KINDS and "ppocrv5_rec_mobile" in KINDS and "ppocrv5_rec_server" in KINDS and "ppocrv6_rec" in KINDS


def test_every_stem_of_the_graph_resolves(tmp_path):
    from rapiddoc_amd.session import REC_ARCH_BY_STEM, REC_ARCH_BY_STEM_MV1E, resolve_rec_kind
    assert sorted(REC_ARCH_BY_STEM_MV1E) == sorted(STEMS) and set(REC_ARCH_BY_STEM_MV1E.values()) == {KIND}
    assert not set(REC_ARCH_BY_STEM_MV1E) & set(REC_ARCH_BY_STEM)
    for stem in STEMS:
        assert resolve_rec_kind(str(tmp_path / (stem + ".safetensors"))) == KIND
        assert resolve_rec_kind(stem + ".pth") == KIND
    assert resolve_rec_kind("ch_PP-OCRv5_rec_mobile.safetensors") == "ppocrv5_rec_mobile"


def test_tensor_names_resolve_and_refusals_stay(golden_dir):
    from rapiddoc_amd.session import resolve_rec_kind
    for lang in ("korean", "latin"):
        names = {n: None for n, _s, _d in _manifest(golden_dir, lang)}
        assert resolve_rec_kind(names) == KIND
        assert resolve_rec_kind({"model." + n: v for n, v in names.items()}) == KIND
    small = {"model.head.fc.weight": np.zeros((130, 64), np.float32),
             "model.backbone.block_list.0._depthwise_conv._conv.weight": np.zeros((16, 1, 3, 3), np.float32)}
    assert resolve_rec_kind(W.to_safetensors_bytes(small)) == KIND
    assert resolve_rec_kind(W.to_safetensors_bytes({k[len("model."):]: v for k, v in small.items()})) == KIND
    for kind in ("ppocrv5_rec_mobile", "ppocrv5_rec_server", "ppocrv6_rec"):
        assert resolve_rec_kind({n: None for n, _s, _d in W.load_manifest(golden_dir / f"manifest_{kind}.json")}) == kind
    # still refused: a v4 Chinese stem, a lone backbone tensor of either naming, the classifier without this backbone
    with pytest.raises(ValueError, match="is not in the recognisers this engine serves"):
        resolve_rec_kind("ch_PP-OCRv4_rec_server.safetensors")
    with pytest.raises(ValueError, match="is not in the recognisers this engine serves"):
        resolve_rec_kind("ch_PP-OCRv4_rec_infer.pth")
    for keys in ({"backbone.conv.weight": None}, {"backbone.conv1.conv.weight": None}, {"head.fc.weight": None},
                 {"backbone.block_list.0._depthwise_conv._conv.weight": None}):
        with pytest.raises(ValueError, match="is not in"):
            resolve_rec_kind(keys)


@pytest.mark.parametrize("lang", ["korean", "latin"])
def test_manifest_is_the_reference_architecture(golden_dir, lang):
    man = _manifest(golden_dir, lang)
    shapes = {n: s for n, s, _d in man}
    s = _summary(golden_dir)["files"][lang]
    assert len(man) == s["tensors"] == 228 and s["classes"] == CLASSES[lang]
    assert shapes["backbone.conv1._conv.weight"] == (16, 3, 3, 3)
    assert shapes["backbone.block_list.5._depthwise_conv._conv.weight"] == (128, 1, 3, 3)
    assert shapes["backbone.block_list.6._depthwise_conv._conv.weight"] == (256, 1, 5, 5)
    assert shapes["backbone.block_list.11._pointwise_conv._conv.weight"] == (512, 256, 1, 1)
    assert shapes["backbone.block_list.12._depthwise_conv._conv.weight"] == (512, 1, 5, 5)
    assert shapes["backbone.block_list.12._se.conv1.weight"] == (128, 512, 1, 1) and "backbone.block_list.10._se.conv1.weight" not in shapes
    assert shapes["neck.encoder.conv1.conv.weight"] == (64, 512, 3, 3) and shapes["neck.encoder.conv4.conv.weight"] == (64, 1024, 3, 3)
    assert shapes["neck.encoder.conv1x1.conv.weight"] == (64, 64, 1, 1)
    assert shapes["head.fc.weight"] == (CLASSES[lang], 64)
    st = W.synth_state_dict(man, 0, kind=KIND)
    assert abs(W.checksum(st) - s["checksum"]) <= 1e-9 * max(1.0, abs(s["checksum"]))
    if lang == "latin":
        assert s["parameters"] == sum(int(np.prod(sh)) for _n, sh, d in man if d == "float32") and 2.2e6 < s["parameters"] < 2.3e6


def test_the_gains_are_opt_in(golden_dir):
    """Without `kind=` every tensor is the plain rule's - this kind's own manifest included - and every earlier manifest keeps the
    checksum of the parent commit."""
    for kind, c in PARENT_CHECKSUMS.items():
        st = W.synth_state_dict(W.load_manifest(golden_dir / f"manifest_{kind}.json"), 0)
        assert abs(W.checksum(st) - c) <= 1e-9 * max(1.0, abs(c)), kind
    man = _manifest(golden_dir, "latin")
    plain, gained = W.synth_state_dict(man, 0), W.synth_state_dict(man, 0, kind=KIND)
    want = {"backbone.conv1._conv.weight": 2.2, "head.fc.weight": 30.0, "backbone.block_list.0._depthwise_conv._conv.weight": 0.7,
            "backbone.block_list.12._pointwise_conv._conv.weight": 4.0, "backbone.block_list.10._depthwise_conv._conv.weight": 0.5}
    changed = 0
    for n in plain:
        if np.array_equal(plain[n], gained[n]):
            assert n not in want
            continue
        changed += 1
        assert n.endswith("._conv.weight") or n == "head.fc.weight", n
        if n in want:
            assert np.array_equal(gained[n], (plain[n] * np.float32(want[n])).astype(np.float32)), n
    assert changed == 1 + 26 + 1 - 1          # conv1, 13 x (depthwise, pointwise), the classifier; block 6's depthwise gain is 1.0
    for n, sh, d in man:
        assert np.array_equal(plain[n], W.synth_tensor(n, sh, d, 0))


@pytest.mark.parametrize("lang,tag,shape", FIXTURES)
def test_fixtures_agree_with_their_summary(golden_dir, lang, tag, shape):
    full = _summary(golden_dir)
    s, step, ncls = full["fixtures"][f"{lang}_{tag}"], full["files"][lang]["logits_step"], CLASSES[lang]
    f = golden_dir / f"recmv1e_{lang}_seed0_{tag}.npz"
    assert f.stat().st_size == s["bytes"] <= 1 << 20
    g = np.load(f)
    B, T = shape[0], ocr_host.rec_seq_len(shape[3])
    assert tuple(int(v) for v in g["x_shape"]) == shape and int(g["x_seed"]) == s["x_seed"] >= 200 + shape[3]
    if "x" in g.files:
        assert np.array_equal(np.random.default_rng(int(g["x_seed"])).uniform(-1.0, 1.0, shape).astype(np.float32), g["x"])
    cs = int(g["backbone_cs"])
    assert g["backbone"].shape == (B, 512 // cs, 1, T) and g["neck"].shape == (B, T, 64)
    assert g["idx"].shape == g["prob"].shape == g["top2gap"].shape == (B, T) and g["top2idx"].shape == (B, T, 2)
    assert g["logits_sub"].shape == (B, T, len(range(0, ncls, step))) and g["logits_t0"].shape == (B, ncls)
    assert np.array_equal(g["top2idx"][..., 0], g["idx"]) and np.array_equal(g["logits_sub"][:, 0, :], g["logits_t0"][:, ::step])
    assert float((g["top2gap"] <= 1e-2).mean()) == s["masked_share"] <= 0.01
    assert s["backbone_std_over_T_rel"] >= 0.01
    assert len(np.unique(g["idx"])) == s["distinct_argmax"] and (lang != "korean" or B * T < 80 or s["distinct_argmax"] >= 5)


def test_width_pair_fixture_separates_the_two_widths(golden_dir):
    s = _summary(golden_dir)["width_pair"]
    g = np.load(golden_dir / "recmv1e_width_pair.npz")
    d = np.abs(g["neck200"][0] - g["neck320"][0, :25]).max(axis=1)
    assert g["backbone200"].shape == (1, 512, 1, 25) and g["backbone320"].shape == (1, 512, 1, 40) and np.array_equal(d, g["d"])
    assert float(d.min()) == s["d_min"] >= 10 * 1e-3 and float(d.max()) == s["d_max"]


# ------------------------------------------------------------------------------------------------ the folded graph in float64
_BLOCKS = [(3, 1, 1, False), (3, 1, 1, False), (3, 1, 1, False), (3, 2, 1, False), (3, 1, 1, False), (3, 2, 1, False)] + \
          [(5, 1, 1, False)] * 5 + [(5, 2, 1, True), (5, 1, 2, True)]


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _fold(st, conv, bn):
    """Conv (no bias) + BatchNorm (eps 1e-5) -> weight, bias in double"""
    sc = _t(st[bn + ".weight"]) / torch.sqrt(_t(st[bn + ".running_var"]) + 1e-5)
    w = _t(st[conv])
    return w * sc.reshape(-1, 1, 1, 1), _t(st[bn + ".bias"]) - _t(st[bn + ".running_mean"]) * sc


def _swish(v):
    return v * torch.sigmoid(v)


def folded_graph_float64(st, x):
    """The graph as the engine runs it.  Every producer (conv1, the pointwise layers) hands on convolution + bias; the consumer applies
    the hardswish.  Returns tokens [B, T, 512], neck [B, T, 64], logits [B, T, C]."""
    F = torch.nn.functional
    w, b = _fold(st, "backbone.conv1._conv.weight", "backbone.conv1._batch_norm")
    h = F.conv2d(_t(x), w, b, stride=2, padding=1)
    for i, (k, sh, sw, se) in enumerate(_BLOCKS):
        p = f"backbone.block_list.{i}"
        w, b = _fold(st, p + "._depthwise_conv._conv.weight", p + "._depthwise_conv._batch_norm")
        t = hswish64(F.conv2d(hswish64(h), w, b, stride=(sh, sw), padding=k // 2, groups=w.shape[0]))     # on-load hardswish, then zero padding
        if se:
            m = t.mean(dim=(2, 3), keepdim=True)
            m = torch.relu(F.conv2d(m, _t(st[p + "._se.conv1.weight"]), _t(st[p + "._se.conv1.bias"])))
            m = F.conv2d(m, _t(st[p + "._se.conv2.weight"]), _t(st[p + "._se.conv2.bias"]))
            t = t * (torch.clamp(m + 3.0, 0.0, 6.0) / 6.0)
        w, b = _fold(st, p + "._pointwise_conv._conv.weight", p + "._pointwise_conv._batch_norm")
        h = F.conv2d(t, w, b)
    assert h.shape[2] == 3
    a = hswish64(h[:, :, :2, : h.shape[3] // 2 * 2])                                  # AvgPool2d(2, 2) of a 3-row map: rows 0 and 1 only
    tok = (a[:, :, 0, 0::2] + a[:, :, 0, 1::2] + a[:, :, 1, 0::2] + a[:, :, 1, 1::2]) / 4.0       # [B, 512, T]
    e = "neck.encoder"

    def seqconv(name, z):        # of the 3 x 3 kernel only the middle row meets the one-row map
        w, b = _fold(st, f"{e}.{name}.conv.weight", f"{e}.{name}.norm")
        return _swish(F.conv1d(z, w[:, :, w.shape[2] // 2, :], b, padding=1))

    def conv1x1(name, z):
        w, b = _fold(st, f"{e}.{name}.conv.weight", f"{e}.{name}.norm")
        return _swish(F.conv1d(z, w[:, :, 0, :], b))

    z = conv1x1("conv2", seqconv("conv1", tok)).permute(0, 2, 1)                     # [B, T, 120]
    B, T, Cn = z.shape
    for d in range(2):
        p = f"{e}.svtr_block.{d}"
        y = F.layer_norm(z, (Cn,), _t(st[p + ".norm1.weight"]), _t(st[p + ".norm1.bias"]), 1e-5)
        qkv = F.linear(y, _t(st[p + ".mixer.qkv.weight"]), _t(st[p + ".mixer.qkv.bias"])).reshape(B, T, 3, 8, Cn // 8).permute(2, 0, 3, 1, 4)
        att = torch.softmax((qkv[0] * (Cn // 8) ** -0.5) @ qkv[1].transpose(-1, -2), dim=-1)
        y = (att @ qkv[2]).permute(0, 2, 1, 3).reshape(B, T, Cn)
        z = z + F.linear(y, _t(st[p + ".mixer.proj.weight"]), _t(st[p + ".mixer.proj.bias"]))
        y = F.layer_norm(z, (Cn,), _t(st[p + ".norm2.weight"]), _t(st[p + ".norm2.bias"]), 1e-5)
        y = F.linear(_swish(F.linear(y, _t(st[p + ".mlp.fc1.weight"]), _t(st[p + ".mlp.fc1.bias"]))), _t(st[p + ".mlp.fc2.weight"]),
                     _t(st[p + ".mlp.fc2.bias"]))
        z = z + y
    z = F.layer_norm(z, (Cn,), _t(st[e + ".norm.weight"]), _t(st[e + ".norm.bias"]), 1e-6).permute(0, 2, 1)
    z = conv1x1("conv3", z)
    neck = conv1x1("conv1x1", seqconv("conv4", torch.cat((tok, z), dim=1))).permute(0, 2, 1)
    logits = F.linear(neck, _t(st["head.fc.weight"]), _t(st["head.fc.bias"]))
    return tok.permute(0, 2, 1), neck, logits


@pytest.mark.parametrize("lang,tag", [("korean", "b2_w320"), ("latin", "b1_w96")])
def test_float64_restatement_of_the_folded_graph_reproduces_the_fixtures(golden_dir, lang, tag):
    """The reference computed the fixtures in fp32 with BatchNorm and activation in their own places; the folded form in float64 must
    agree within the engine's bound 1e-3 max(1, max |ref|) - in fact far inside it (fp32 rounding of the reference only)."""
    st = W.synth_state_dict(_manifest(golden_dir, lang), 0, kind=KIND)
    g = np.load(golden_dir / f"recmv1e_{lang}_seed0_{tag}.npz")
    x = golden_x(g)
    tok, neck, logits = folded_graph_float64(st, x)
    cs, step = int(g["backbone_cs"]), _summary(golden_dir)["files"][lang]["logits_step"]
    ref_tok = g["backbone"][:, :, 0, :].transpose(0, 2, 1)
    for name, got, ref in (("tokens", tok.numpy()[:, :, ::cs], ref_tok), ("neck", neck.numpy(), g["neck"]),
                           ("logits", logits.numpy()[:, :, ::step], g["logits_sub"])):
        err, bound = float(np.abs(got - ref).max()), 1e-3 * max(1.0, float(np.abs(ref).max()))
        print(f"[{lang} {tag}] {name}: max-abs error {err:.3e} (bound {bound:.3e})")
        assert got.shape == ref.shape and err < bound, name
    safe = g["top2gap"] > 1e-2
    assert (logits.numpy().argmax(axis=2) == g["idx"])[safe].all()


# ------------------------------------------------------------------------------------------------ dictionaries, exports
def test_char_table_and_decode_take_multi_codepoint_entries():
    """Devanagari / Tamil dictionaries hold whole clusters (several code points, up to 9+ UTF-8 bytes) as ONE class."""
    chars = ["blank", "a", "क्ष", "நி", "श्री", " "]       # ksha, ni, shri
    tab, max_len = ocr_host.char_table(chars)
    assert max_len == len(chars[4].encode()) == 12 and tab.shape == (6, 13)
    for i, c in enumerate(chars):
        assert tab[i, 0] == len(c.encode()) and bytes(tab[i, 1:1 + tab[i, 0]]).decode() == c
    idx = np.array([[0, 2, 2, 0, 2, 3, 4, 4, 1, 0]])
    prob = np.full(idx.shape, 0.5, np.float32)
    (text, conf), = ocr_host.ctc_decode(idx, prob, chars)
    assert text == chars[2] + chars[2] + chars[3] + chars[4] + "a" and abs(conf - 0.5) < 1e-7


def test_the_library_exports_the_new_entries():
    from rapiddoc_amd import _lib
    lib = _lib.load()
    for name in ("rd_debug_dw5_strip", "rd_debug_mv1e_pool", "rd_rec_backbone_forward_lines", "rd_rec_seq_len", "rd_rec_token_dim"):
        assert hasattr(lib, name), name
    header = (Path(__file__).resolve().parents[1] / "include" / "rapiddoc_mi355.h").read_text()
    assert header.count('"ppocr_rec_mv1e"') >= 3          # rd_create, RD_REC_WANT_NECK, RD_REC_LINE_WIDTHS
    assert isinstance(lib.rd_debug_dw5_strip, C._CFuncPtr)
