"""CPU: the host side of the text-line direction classifier (`ppocr_cls_mobile`: MobileNetV3 small scale 0.35 with squeeze-excite +
ClsHead; the file ch_ptocr_mobile_v2.0_cls_mobile) - the reference-minted fixtures and their summary, the opt-in synthetic-weight gains
and bias offsets, kind selection by stem / tensor names, a float64 restatement of the FOLDED graph - the graph the engine runs - against
the fixtures, the 180-degree rule on numpy crops, and the opt-in switch of the page pipeline."""
import json
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kind_helpers import synth_state
from rapiddoc_amd import weights as W

KIND = "ppocr_cls_mobile"
STEM = "ch_ptocr_mobile_v2.0_cls_mobile"
TAGS = ("b7_h48_w192", "b1_h48_w192", "b3_h40_w100")
# (k, cin, mid, cout, row stride, squeeze-excite, act) of the eleven inverted-residual blocks, as probed on the reference; the column
# stride is 1 everywhere
BLOCKS = [(3, 8, 8, 8, 2, True, "relu"), (3, 8, 24, 8, 2, False, "relu"), (3, 8, 32, 8, 1, False, "relu"),
          (5, 8, 32, 16, 2, True, "hswish"), (5, 16, 88, 16, 1, True, "hswish"), (5, 16, 88, 16, 1, True, "hswish"),
          (5, 16, 40, 16, 1, True, "hswish"), (5, 16, 48, 16, 1, True, "hswish"), (5, 16, 104, 32, 2, True, "hswish"),
          (5, 32, 200, 32, 1, True, "hswish"), (5, 32, 200, 32, 1, True, "hswish")]
TAPS = {0: "b0", 3: "b3", 8: "b8", 10: "b10"}
FIXTURE_TOL = 1e-3          # the project's fixture bound


def state(golden_dir):
    return synth_state(golden_dir, KIND, kind=KIND)


def golden_x(g):
    assert str(g["x_kind"]) == "cls_lines"
    B, _, H, W_ = (int(v) for v in g["x_shape"])
    x, widths = W.synth_cls_lines(int(g["x_seed"]), B, H, W_)
    assert np.array_equal(widths, g["widths"])
    return x


# ---------------------------------------------------------------------------------------------------------------- float64 oracle
def fold64(st, p):
    """Conv + BatchNorm (eps 1e-5) of `p` as (weight, bias) in float64"""
    w = torch.from_numpy(st[p + ".conv.weight"]).double()
    g, b, m, v = (torch.from_numpy(st[p + ".bn." + k]).double() for k in ("weight", "bias", "running_mean", "running_var"))
    s = g / torch.sqrt(v + 1e-5)
    return w * s.view(-1, 1, 1, 1), b - m * s


def act64(t, a):
    return F.relu(t) if a == "relu" else t * torch.clamp(t + 3.0, 0.0, 6.0) / 6.0 if a == "hswish" else t


def hsig_paddle64(t):
    return torch.clamp(0.2 * t + 0.5, 0.0, 1.0)


def block64(x, we, be, wd, bd, wl, bl, k, sh, act, se=None, shortcut=False, gate_fn=hsig_paddle64):
    """One inverted-residual block on folded weights, float64, NCHW.  `se` = (w1, b1, w2, b2) as 2-D / 1-D tensors."""
    e = act64(F.conv2d(x, we, be), act)
    d = act64(F.conv2d(e, wd, bd, stride=(sh, 1), padding=k // 2, groups=wd.shape[0]), act)
    gate = None
    if se is not None:
        w1, b1, w2, b2 = se
        pooled = d.mean(dim=(2, 3))
        gate = gate_fn(F.relu(pooled @ w1.t() + b1) @ w2.t() + b2)
        d = d * gate[:, :, None, None]
    y = F.conv2d(d, wl, bl)
    return (x + y if shortcut else y), gate


def oracle64(st, x):
    """The folded graph in float64: {prob, logits, feat, b0, b3, b8, b10, gates}"""
    out = {}
    h = torch.from_numpy(x).double()
    w, b = fold64(st, "backbone.conv1")
    h = act64(F.conv2d(h, w, b, stride=2, padding=1), "hswish")
    gates = []
    for i, (k, cin, mid, cout, sh, se, act) in enumerate(BLOCKS):
        p = f"backbone.blocks.{i}"
        we, be = fold64(st, p + ".expand_conv")
        wd, bd = fold64(st, p + ".bottleneck_conv")
        wl, bl = fold64(st, p + ".linear_conv")
        sew = None
        if se:
            sew = tuple(torch.from_numpy(st[f"{p}.mid_se.{n}"]).double() for n in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"))
            sew = (sew[0].flatten(1), sew[1], sew[2].flatten(1), sew[3])
        assert we.shape[:2] == (mid, cin) and wl.shape[:2] == (cout, mid) and wd.shape == (mid, 1, k, k)
        h, gate = block64(h, we, be, wd, bd, wl, bl, k, sh, act, sew, shortcut=sh == 1 and cin == cout)
        if gate is not None:
            gates.append(gate)
        if i in TAPS:
            out[TAPS[i]] = h.numpy()
    w, b = fold64(st, "backbone.conv2")
    h = F.max_pool2d(act64(F.conv2d(h, w, b), "hswish"), 2, 2)
    feat = h.mean(dim=(2, 3))
    logits = feat @ torch.from_numpy(st["head.fc.weight"]).double().t() + torch.from_numpy(st["head.fc.bias"]).double()
    out.update(feat=feat.numpy(), logits=logits.numpy(), prob=torch.softmax(logits, dim=1).numpy(), gates=torch.cat(gates, dim=1).numpy())
    return out


_ORACLE = {}


def oracle_for(golden_dir, tag):
    """computed once per fixture, shared, left unchanged"""
    if tag not in _ORACLE:
        g = np.load(golden_dir / f"cls_seed0_{tag}.npz")
        _ORACLE[tag] = oracle64(state(golden_dir), golden_x(g))
    return _ORACLE[tag]


# ---------------------------------------------------------------------------------------------------------------- tests
def test_kind_is_listed_and_symbols_are_bound():
    from rapiddoc_amd import _lib
    from rapiddoc_amd.engine import CLS_FEATURES, CLS_WANT_AUX, KINDS
    assert KIND in KINDS and CLS_WANT_AUX == 1 and CLS_FEATURES == 200
    assert {"rd_cls_forward", "rd_line_flip180_batch"} <= set(_lib.SYMBOLS)


def test_manifest_and_summary_checksum(golden_dir):
    man = W.load_manifest(golden_dir / f"manifest_{KIND}.json")
    summary = json.loads((golden_dir / "summary_cls_mobile.json").read_text())
    assert len(man) == summary["tensors"] == 248
    assert summary["parameters"] == 129356
    shapes = {n: sh for n, sh, _ in man}
    assert shapes["backbone.conv1.conv.weight"] == (8, 3, 3, 3) and shapes["backbone.conv2.conv.weight"] == (200, 32, 1, 1)
    assert shapes["head.fc.weight"] == (2, 200) and shapes["head.fc.bias"] == (2,)
    for i, (k, cin, mid, cout, sh, se, act) in enumerate(BLOCKS):
        p = f"backbone.blocks.{i}"
        assert shapes[p + ".expand_conv.conv.weight"] == (mid, cin, 1, 1)
        assert shapes[p + ".bottleneck_conv.conv.weight"] == (mid, 1, k, k)
        assert shapes[p + ".linear_conv.conv.weight"] == (cout, mid, 1, 1)
        assert ((p + ".mid_se.conv1.weight") in shapes) == se
        if se:
            assert shapes[p + ".mid_se.conv1.weight"] == (mid // 4, mid, 1, 1) and shapes[p + ".mid_se.conv2.weight"] == (mid, mid // 4, 1, 1)
    assert W.checksum(state(golden_dir)) == summary["checksum"] == 4427.555996501413
    assert W.checksum(W.synth_state_dict(man, 0)) != summary["checksum"]          # gain and offset are opt-in
    plain = W.synth_state_dict(man, 0)
    st = state(golden_dir)
    changed = sorted(n for n in st if not np.array_equal(st[n], plain[n]))
    assert changed == ["head.fc.bias", "head.fc.weight"]                          # the gain on the head, the additive term on its bias
    assert np.array_equal(st["head.fc.bias"], (plain["head.fc.bias"] + np.float32([-11.6, 11.6])).astype(np.float32))


def test_summary_meets_the_mint_conditions_and_fixtures_are_complete(golden_dir):
    summary = json.loads((golden_dir / "summary_cls_mobile.json").read_text())
    assert set(summary["fixtures"]) == set(TAGS)
    p1 = np.concatenate([np.asarray(summary["fixtures"]["b7_h48_w192"]["prob"])[:, 1], np.asarray(summary["draw48"]["p1"])])
    n = p1.size
    assert n == 55
    assert (p1 < 0.5).sum() * 4 >= n and (p1 > 0.5).sum() * 4 >= n
    assert ((p1 > 0.5) & (p1 < 0.9)).sum() >= 3 and (p1 >= 0.9).sum() >= 3
    near = (np.abs(p1 - 0.5) <= 1e-3) | (np.abs(p1 - 0.9) <= 1e-3)
    assert near.sum() * 10 <= n
    assert int(near.sum()) == len(summary["fixtures"]["b7_h48_w192"]["left_out"]) + len(summary["draw48"]["left_out"])
    for tag in TAGS:
        f = golden_dir / f"cls_seed0_{tag}.npz"
        assert f.stat().st_size <= 1 << 20
        g = np.load(f)
        B, _, H, W_ = (int(v) for v in g["x_shape"])
        assert g["prob"].shape == g["logits"].shape == (B, 2) and g["feat"].shape == (B, 200)
        rows, h = {}, (H - 1) // 2 + 1
        for i, blk in enumerate(BLOCKS):
            h = (h - 1) // blk[4] + 1
            rows[i] = h
        for i, name in TAPS.items():
            assert g[name].shape == (B, BLOCKS[i][3], rows[i], (W_ - 1) // 2 + 1), (tag, name)
        x = golden_x(g)
        for i, w in enumerate(g["widths"]):
            assert not x[i, :, :, w:].any() and x[i, :, :, :w].any()              # zero right-padding behind the content
    g = np.load(golden_dir / "cls_seed0_b7_h48_w192.npz")
    assert sorted(g["widths"].tolist()) == [12, 42, 72, 102, 132, 162, 192]


@pytest.mark.parametrize("tag", TAGS)
def test_float64_restatement_of_the_folded_graph_reproduces_the_fixture(golden_dir, tag):
    g = np.load(golden_dir / f"cls_seed0_{tag}.npz")
    o = oracle_for(golden_dir, tag)
    msgs = []
    for name in ("prob", "logits", "feat", "b0", "b3", "b8", "b10"):
        ref = g[name]
        e = float(np.abs(o[name] - ref).max())
        bound = FIXTURE_TOL if name == "prob" else FIXTURE_TOL * max(1.0, float(np.abs(ref).max()))
        msgs.append(f"{name} {e:.2e} (bound {bound:.2e})")
        assert e <= bound, (tag, name, e, bound)
    print(f"\n[cls mobile {tag}] float64 folded graph against the fixture: " + ", ".join(msgs))
    # the fixture weights never clamp the squeeze-excite gate (the kernel tests draw weights that do)
    assert 0.0 < o["gates"].min() and o["gates"].max() < 1.0


def test_resolve_cls_kind_by_stem_and_by_tensor_names(golden_dir):
    from rapiddoc_amd.session import CLS_ARCH_BY_STEM, resolve_cls_kind, resolve_det_kind, resolve_rec_kind
    assert CLS_ARCH_BY_STEM == {STEM: KIND}
    assert resolve_cls_kind(f"/some/dir/{STEM}.safetensors") == KIND
    with pytest.raises(ValueError):
        resolve_cls_kind("ch_PP-OCRv5_rec_mobile.safetensors")
    man = W.load_manifest(golden_dir / f"manifest_{KIND}.json")
    shaped = {n: np.zeros(sh, np.float32) for n, sh, d in man if d == "float32"}
    assert resolve_cls_kind(shaped) == KIND
    assert resolve_cls_kind({"model." + n: v for n, v in shaped.items()}) == KIND
    small = {"model.head.fc.weight": np.zeros((2, 200), np.float32), "model.backbone.blocks.0.mid_se.conv1.weight": np.zeros((2, 8, 1, 1), np.float32)}
    assert resolve_cls_kind(W.to_safetensors_bytes(small)) == KIND
    with pytest.raises(ValueError):                                            # a head with another class count is no direction classifier
        resolve_cls_kind({**small, "model.head.fc.weight": np.zeros((4, 200), np.float32)})
    with pytest.raises(ValueError):
        resolve_cls_kind({"head.fc.weight": np.zeros((2, 200), np.float32)})   # the head alone names no backbone
    for kind, man_name in (("ppocr_rec_mv1e", "ppocr_rec_mv1e_latin"), ("ppocrv5_rec_mobile",) * 2, ("ppocrv6_rec",) * 2,
                           ("ppocrv3_det_mobile",) * 2, ("ppocrv5_det_mobile",) * 2):
        other = {n: np.zeros(sh, np.float32) for n, sh, d in W.load_manifest(golden_dir / f"manifest_{man_name}.json") if d == "float32"}
        with pytest.raises(ValueError):
            resolve_cls_kind(other)
        assert (resolve_rec_kind if "rec" in kind else resolve_det_kind)(other) == kind      # ... and they resolve as before
    # the classifier is neither a recogniser nor a detector
    with pytest.raises(ValueError):
        resolve_rec_kind(f"{STEM}.safetensors")
    with pytest.raises(ValueError):
        resolve_det_kind(f"{STEM}.safetensors")
    with pytest.raises(ValueError):
        resolve_rec_kind(shaped)


def test_dispatch_sends_a_cls_config_to_the_classifier_session(monkeypatch):
    from rapiddoc_amd import session as S
    mods = {"rapidocr": types.ModuleType("rapidocr"), "rapidocr.inference_engine": types.ModuleType("rapidocr.inference_engine"),
            "rapidocr.inference_engine.torch": types.ModuleType("rapidocr.inference_engine.torch")}
    mods["rapidocr"].__path__ = mods["rapidocr.inference_engine"].__path__ = []
    mods["rapidocr.inference_engine.torch"].TorchInferSession = object
    for k, v in mods.items():
        monkeypatch.setitem(sys.modules, k, v)
    for cls, name in ((S.Mi355DetSession, "det"), (S.Mi355RecSession, "rec"), (S.Mi355ClsSession, "cls")):
        monkeypatch.setattr(cls, "from_cfg", classmethod(lambda c, cfg, name=name: name))
    S.install_into_rapidocr()
    d = mods["rapidocr.inference_engine.torch"].TorchInferSession
    assert d({"task_type": "TaskType.CLS", "model_path": "x.safetensors"}) == "cls"
    assert d(types.SimpleNamespace(task_type="cls", model_path="y.safetensors")) == "cls"
    assert d({"model_path": f"/w/{STEM}.safetensors"}) == "cls"                     # no task type: the stem decides
    assert d({"task_type": "TaskType.DET", "model_path": "x.safetensors"}) == "det"
    assert d({"task_type": "rec", "model_path": "x.safetensors"}) == "rec"
    assert d({"model_path": "/w/ch_PP-OCRv6_det_small.safetensors"}) == "det"
    assert d({"model_path": "/w/ch_PP-OCRv6_rec_small.safetensors"}) == "rec"


def test_flip_rule_and_pixel_reversal_on_numpy_crops():
    from rapiddoc_amd.pipeline import cls_flip_rule, flip180
    prob = np.float32([[0.7, 0.3], [0.3, 0.7], [0.05, 0.95], [0.1, 0.9], [0.5, 0.5], [0.100001, 0.899999]])
    assert cls_flip_rule(prob, 0.9).tolist() == [False, False, True, True, False, False]       # label 1 AND score >= threshold
    assert cls_flip_rule(prob, 0.6).tolist() == [False, True, True, True, False, True]
    assert cls_flip_rule(prob, 0.0).tolist() == [False, True, True, True, False, True]         # equal scores: label 0 (argmax takes the first)
    rng = np.random.default_rng(0)
    for h, w in ((1, 1), (1, 7), (5, 4), (37, 211)):
        x = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        y = flip180(x)
        assert y.flags.c_contiguous and np.array_equal(y, x[::-1, ::-1])
        assert np.array_equal(y.reshape(-1, 3), x.reshape(-1, 3)[::-1])                         # = the packed pixel order reversed
        assert np.array_equal(flip180(y), x)
        # rotations commute: turning the crop in front of np.rot90 (what the scratch holds) equals turning the crop the classifier saw
        assert np.array_equal(np.rot90(flip180(x)), flip180(np.rot90(x)))


def test_pipeline_use_cls_needs_the_classifier_weights_and_is_off_by_default():
    import inspect
    from rapiddoc_amd.pipeline import PagePipeline, PageResult
    sig = inspect.signature(PagePipeline.__init__)
    assert sig.parameters["use_cls"].default is False and sig.parameters["cls_thresh"].default == 0.9
    with pytest.raises(ValueError, match="ppocr_cls_mobile"):
        PagePipeline({"ppocrv6_det": {}, "ppocrv6_rec": {}}, use_cls=True)
    assert PageResult().cls is None
