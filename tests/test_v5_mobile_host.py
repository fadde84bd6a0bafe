"""CPU: the host side of the PP-OCRv5 mobile recogniser (`model_kind "ppocrv5_rec_mobile"`): the manifest and fixtures against their summary
(tests/golden/make_golden_v5_mobile.py), the synthetic-weight rule of its branch convolutions and that it touches no other kind, and how
the session tells the three recognisers apart."""
import json

import numpy as np
import pytest

from rapiddoc_amd import ocr_host
from rapiddoc_amd import weights as W

KIND = "ppocrv5_rec_mobile"
TAGS = [("b2_w320", (2, 3, 48, 320)), ("b1_w96", (1, 3, 48, 96)), ("b3_w640", (3, 3, 48, 640)), ("b6_w1088", (6, 3, 48, 1088))]


def test_the_kind_is_offered():
    from rapiddoc_amd.engine import KINDS
    assert KIND in KINDS and "ppocrv5_rec_server" in KINDS and "ppocrv6_rec" in KINDS


def test_manifest_is_the_reference_architecture(golden_dir):
    man = W.load_manifest(golden_dir / f"manifest_{KIND}.json")
    shapes = {n: s for n, s, _d in man}
    s = json.loads((golden_dir / "summary_v5_mobile.json").read_text())
    assert len(man) == s["tensors"]
    assert shapes["backbone.conv1.conv.weight"] == (16, 3, 3, 3)
    assert shapes["backbone.blocks2.0.dw_conv.conv_kxk.3.conv.weight"] == (16, 1, 3, 3)
    assert shapes["backbone.blocks5.0.pw_conv.conv_kxk.0.conv.weight"] == (240, 128, 1, 1)
    assert shapes["backbone.blocks6.3.dw_conv.conv_kxk.0.conv.weight"] == (480, 1, 5, 5)
    assert shapes["backbone.blocks6.1.se.conv1.weight"] == (120, 480, 1, 1)
    assert "backbone.blocks4.0.dw_conv.identity.weight" not in shapes and "backbone.blocks4.1.dw_conv.identity.weight" in shapes
    assert "backbone.blocks2.0.pw_conv.conv_1x1.conv.weight" not in shapes          # a 1 x 1 layer has no 1 x 1 branch
    assert shapes["head.ctc_encoder.encoder.conv1.conv.weight"] == (60, 480, 1, 3)
    assert shapes["head.ctc_encoder.encoder.conv4.conv.weight"] == (60, 960, 3, 3)
    assert shapes["head.ctc_head.fc.weight"] == (18385, 120)
    assert abs(W.checksum(W.synth_state_dict(man, 0)) - s["checksum"]) <= 1e-9 * max(1.0, abs(s["checksum"]))


def test_earlier_manifests_keep_their_checksums(golden_dir):
    """The per-group damping of this kind's branch convolutions must touch no other kind: every recorded checksum is reproduced."""
    s = json.loads((golden_dir / "summary.json").read_text())
    want = {"ppocrv6_det": s["det_checksum"], "ppocrv6_rec": s["rec_checksum"], "pphgnetv2_b4": s["b4_checksum"],
            "pphgnetv2_b6_formula": s["b6_checksum"],
            "ppocrv5_rec_server": json.loads((golden_dir / "summary_v5_server.json").read_text())["checksum"],
            "ppocrv5_det_server": json.loads((golden_dir / "summary_det_server.json").read_text())["checksum"]}
    for kind, c in want.items():
        st = W.synth_state_dict(W.load_manifest(golden_dir / f"manifest_{kind}.json"), 0)
        assert abs(W.checksum(st) - c) <= 1e-9 * max(1.0, abs(c)), kind


def test_the_synth_rule_damps_the_branch_convolutions_by_group():
    base = W.synth_tensor("backbone.blocksX.0.dw_conv.conv_kxk.0.conv.weight", (480, 1, 5, 5), "float32", 0).std()
    for group, f in (("blocks2", 0.65), ("blocks3", 0.65), ("blocks4", 0.6), ("blocks5", 0.6), ("blocks6", 0.7)):
        for branch in ("conv_kxk.0", "conv_1x1"):
            a = W.synth_tensor(f"backbone.{group}.0.dw_conv.{branch}.conv.weight", (480, 1, 5, 5), "float32", 0).std()
            assert abs(float(a / base) - f) < 0.03, (group, branch)
    # the server neck's `.conv1x1.` is not `.conv_1x1.`; a name outside the backbone is left alone
    a = W.synth_tensor("head.ctc_encoder.encoder.conv1x1.conv.weight", (120, 60, 1, 1), "float32", 0).std()
    b = W.synth_tensor("head.ctc_encoder.encoder.conv1y1.conv.weight", (120, 60, 1, 1), "float32", 0).std()
    assert abs(float(a / b) - 1.0) < 0.05
    a = W.synth_tensor("neck.blocks2.0.conv_kxk.0.conv.weight", (64, 64, 3, 3), "float32", 0).std()
    assert abs(float(a) - (1.6 / 576) ** 0.5) < 0.05 * (1.6 / 576) ** 0.5


def test_session_kind_follows_the_stem_and_the_state_dict_keys(tmp_path, golden_dir):
    from rapiddoc_amd.session import resolve_rec_kind
    assert resolve_rec_kind(str(tmp_path / "ch_PP-OCRv5_rec_mobile.safetensors")) == KIND
    assert resolve_rec_kind(tmp_path / "ch_PP-OCRv5_rec_server.safetensors") == "ppocrv5_rec_server"
    assert resolve_rec_kind("ch_PP-OCRv6_small_rec_infer.safetensors") == "ppocrv6_rec"
    keys = {k: {n: None for n, _s, _d in W.load_manifest(golden_dir / f"manifest_{k}.json")} for k in (KIND, "ppocrv5_rec_server", "ppocrv6_rec")}
    assert "head.ctc_head.fc.weight" in keys[KIND] and "head.ctc_head.fc.weight" in keys["ppocrv5_rec_server"]
    for k, names in keys.items():
        assert resolve_rec_kind(names) == k
        assert resolve_rec_kind({"model." + n: v for n, v in names.items()}) == k
    blob = W.to_safetensors_bytes({"head.ctc_head.fc.weight": np.zeros((4, 120), np.float32), "backbone.conv1.conv.weight": np.zeros((16, 3, 3, 3), np.float32)})
    assert resolve_rec_kind(blob) == KIND
    blob = W.to_safetensors_bytes({"head.ctc_head.fc.weight": np.zeros((4, 120), np.float32), "backbone.blocks2.0.x": np.zeros(1, np.float32)})
    assert resolve_rec_kind(blob) == KIND
    with pytest.raises(ValueError, match="is not in"):
        resolve_rec_kind({"backbone.conv1.conv.weight": None})


@pytest.mark.parametrize("tag,shape", TAGS)
def test_fixtures_agree_with_their_summary(golden_dir, tag, shape):
    s = json.loads((golden_dir / "summary_v5_mobile.json").read_text())["fixtures"][tag]
    f = golden_dir / f"rec5m_seed0_{tag}.npz"
    assert f.stat().st_size == s["bytes"] <= 1 << 20
    g = np.load(f)
    B, T = shape[0], ocr_host.rec_seq_len(shape[3])
    assert tuple(int(v) for v in g["x_shape"]) == shape
    if "x" in g.files:
        assert np.array_equal(np.random.default_rng(int(g["x_seed"])).uniform(-1.0, 1.0, shape).astype(np.float32), g["x"])
    cs = int(g["backbone_cs"])
    assert g["backbone"].shape == (B, 480 // cs, 1, T) and g["neck"].shape == (B, T, 120)
    assert g["idx"].shape == g["prob"].shape == g["top2gap"].shape == (B, T) and g["top2idx"].shape == (B, T, 2)
    sub = g["logits_sub"] if "logits_sub" in g.files else np.load(golden_dir / f"rec5m_seed0_{tag}_logits.npz")["logits_sub"]
    assert sub.shape == (B, T, len(range(0, 18385, 61))) and g["logits_t0"].shape == (B, 18385)
    assert np.array_equal(g["top2idx"][..., 0], g["idx"]) and np.array_equal(sub[:, 0, :], g["logits_t0"][:, ::61])
    assert float((g["top2gap"] <= 1e-2).mean()) == s["masked_share"] <= 0.01
    assert s["backbone_std_over_T_rel"] >= 0.02
    assert len(np.unique(g["idx"])) == s["distinct_argmax"] and (B * T < 80 or s["distinct_argmax"] >= 5)


def test_width_pair_fixture_separates_the_two_widths(golden_dir):
    s = json.loads((golden_dir / "summary_v5_mobile.json").read_text())["width_pair"]
    g = np.load(golden_dir / "rec5m_width_pair.npz")
    d = np.abs(g["neck200"][0] - g["neck320"][0, :25]).max(axis=1)
    assert g["backbone200"].shape == (1, 480, 1, 25) and g["backbone320"].shape == (1, 480, 1, 40) and np.array_equal(d, g["d"])
    assert float(d.min()) == s["d_min"] >= 10 * 1e-3 and float(d.max()) == s["d_max"]
