"""CPU: the host side of the PP-OCRv5 server recogniser (`model_kind "ppocrv5_rec_server"`): how the session picks the kind from the
weights, the synthetic-weight rule of its CTC classifier, the launches of one padded width each, and the minted fixtures against their
summary (tests/golden/make_golden_v5_server.py)."""
import json

import numpy as np
import pytest

from rapiddoc_amd import ocr_host
from rapiddoc_amd import weights as W

KIND = "ppocrv5_rec_server"


def test_the_kind_is_offered():
    from rapiddoc_amd.engine import KINDS
    assert KIND in KINDS and "ppocrv6_rec" in KINDS


@pytest.mark.parametrize("stem,kind", [("ch_PP-OCRv6_rec_small", "ppocrv6_rec"), ("ch_PP-OCRv6_small_rec_infer", "ppocrv6_rec"),
                                       ("ch_PP-OCRv5_rec_server", KIND)])
def test_session_kind_follows_the_file_stem(tmp_path, stem, kind):
    from rapiddoc_amd.session import resolve_rec_kind
    assert resolve_rec_kind(str(tmp_path / f"{stem}.safetensors")) == kind
    assert resolve_rec_kind(tmp_path / f"{stem}.safetensors") == kind


def test_an_unknown_stem_is_an_error_not_a_guess(tmp_path):
    from rapiddoc_amd.session import resolve_rec_kind
    with pytest.raises(ValueError, match=r"architecture ch_PP-OCRv4_rec_server is not in"):
        resolve_rec_kind(str(tmp_path / "ch_PP-OCRv4_rec_server.safetensors"))
    with pytest.raises(ValueError, match=r"architecture weights is not in"):
        resolve_rec_kind("weights.safetensors")


def test_session_kind_follows_the_state_dict_keys(golden_dir):
    from rapiddoc_amd.session import resolve_rec_kind
    v5 = {n: None for n, _s, _d in W.load_manifest(golden_dir / f"manifest_{KIND}.json")}
    v6 = {n: None for n, _s, _d in W.load_manifest(golden_dir / "manifest_ppocrv6_rec.json")}
    assert "head.ctc_head.fc.weight" in v5 and "head.head.weight" in v6
    assert resolve_rec_kind(v5) == KIND and resolve_rec_kind(v6) == "ppocrv6_rec"
    assert resolve_rec_kind({"model." + k: v for k, v in v5.items()}) == KIND            # the prefix the reference strips
    blob = W.to_safetensors_bytes({"head.ctc_head.fc.weight": np.zeros((4, 120), np.float32), "head.ctc_head.fc.bias": np.zeros(4, np.float32)})
    assert resolve_rec_kind(blob) == KIND
    with pytest.raises(ValueError, match="is not in"):
        resolve_rec_kind({"backbone.conv.weight": None})


def test_the_new_synth_rule_widens_only_the_server_classifier(golden_dir):
    s = json.loads((golden_dir / "summary.json").read_text())
    for kind, key in (("ppocrv6_det", "det_checksum"), ("ppocrv6_rec", "rec_checksum"), ("pphgnetv2_b4", "b4_checksum"),
                      ("pphgnetv2_b6_formula", "b6_checksum")):
        st = W.synth_state_dict(W.load_manifest(golden_dir / f"manifest_{kind}.json"), 0)
        assert abs(W.checksum(st) - s[key]) <= 1e-9 * max(1.0, abs(s[key])), kind
    a = W.synth_tensor("head.ctc_head.fc.weight", (500, 120), "float32", 0)
    b = W.synth_tensor("head.ctc_head.fcx.weight", (500, 120), "float32", 0)
    assert 25.0 < float(a.std() / b.std()) < 35.0


def test_manifest_is_the_reference_architecture(golden_dir):
    man = W.load_manifest(golden_dir / f"manifest_{KIND}.json")
    shapes = {n: s for n, s, _d in man}
    s = json.loads((golden_dir / "summary_v5_server.json").read_text())
    assert len(man) == s["tensors"] == 547
    assert shapes["head.ctc_head.fc.weight"] == (18385, 120)
    assert shapes["head.ctc_encoder.encoder.conv1.conv.weight"] == (256, 2048, 1, 3)
    assert shapes["head.ctc_encoder.encoder.conv4.conv.weight"] == (256, 4096, 3, 3)
    assert shapes["backbone.stages.0.downsample.conv.weight"] == (48, 1, 3, 3)          # text_rec: stage 1 downsamples too
    assert abs(W.checksum(W.synth_state_dict(man, 0)) - s["checksum"]) <= 1e-9 * max(1.0, abs(s["checksum"]))


@pytest.mark.parametrize("tag,shape", [("b2_w320", (2, 3, 48, 320)), ("b1_w96", (1, 3, 48, 96)), ("b3_w640", (3, 3, 48, 640)),
                                       ("b6_w1088", (6, 3, 48, 1088))])
def test_fixtures_agree_with_their_summary(golden_dir, tag, shape):
    s = json.loads((golden_dir / "summary_v5_server.json").read_text())["fixtures"][tag]
    f = golden_dir / f"rec5s_seed0_{tag}.npz"
    assert f.stat().st_size == s["bytes"] <= 1 << 20
    g = np.load(f)
    B, T = shape[0], ocr_host.rec_seq_len(shape[3])
    assert tuple(int(v) for v in g["x_shape"]) == shape
    if "x" in g.files:
        x = np.random.default_rng(int(g["x_seed"])).uniform(-1.0, 1.0, shape).astype(np.float32)
        assert np.array_equal(x, g["x"])
    cs = int(g["backbone_cs"])
    assert g["backbone"].shape == (B, 2048 // cs, 1, T) and g["neck"].shape == (B, T, 120)
    assert g["idx"].shape == g["prob"].shape == g["top2gap"].shape == (B, T) and g["top2idx"].shape == (B, T, 2)
    sub = g["logits_sub"] if "logits_sub" in g.files else np.load(golden_dir / f"rec5s_seed0_{tag}_logits.npz")["logits_sub"]
    assert sub.shape == (B, T, len(range(0, 18385, 61))) and g["logits_t0"].shape == (B, 18385)
    assert np.array_equal(g["top2idx"][..., 0], g["idx"]) and np.array_equal(sub[:, 0, :], g["logits_t0"][:, ::61])
    share = float((g["top2gap"] <= 1e-2).mean())
    assert share == s["masked_share"] <= 0.01
    assert abs(float(g["neck"].std(axis=1).mean()) - s["neck_std_over_T"]) < 1e-6
    p0 = np.exp(g["logits_t0"] - g["logits_t0"].max(axis=1, keepdims=True))
    assert np.abs((p0 / p0.sum(axis=1, keepdims=True)).max(axis=1) - g["prob"][:, 0]).max() < 1e-5


def test_width_pair_fixture_separates_the_two_widths(golden_dir):
    s = json.loads((golden_dir / "summary_v5_server.json").read_text())["width_pair"]
    g = np.load(golden_dir / "rec5s_width_pair.npz")
    d = np.abs(g["neck200"][0] - g["neck320"][0, :25]).max(axis=1)
    assert g["neck200"].shape == (1, 25, 120) and g["neck320"].shape == (1, 40, 120) and np.array_equal(d, g["d"])
    assert float(d.min()) == s["d_min"] >= 10 * 1e-3 and float(d.max()) == s["d_max"]


def test_equal_width_launches_keep_order_and_widths():
    order = np.arange(20)[::-1].copy()
    line_w = np.array([320] * 9 + [400] * 4 + [1088] * 7)
    out = ocr_host.rec_batches_equal_width(order, line_w, max_columns=6 * 1088, n_max=8)
    assert np.array_equal(np.concatenate([c for c, _w in out]), order)
    assert [(len(c), w) for c, w in out] == [(8, 320), (1, 320), (4, 400), (6, 1088), (1, 1088)]
