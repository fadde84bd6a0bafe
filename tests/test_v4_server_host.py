"""CPU: the PP-OCRv4 server detector and recogniser (PPHGNet_small) as data and host code: the two manifests resolve by their tensor names
to the two v5 server kinds, their non-backbone parts are those of the v5 manifests but for the widths that follow from the backbone, the
fixture summary meets its gates, the new symbols are exported, and conv3x3_wide_shape_ok takes the network's shapes and nothing beside
them.  (The path stems of the v4 server files stay refused: tests/test_det_server_host.py and tests/test_v5_server_host.py assert that.)"""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

from rapiddoc_amd import weights as W

ROOT = Path(__file__).resolve().parents[1]
DET, REC = "ppocrv5_det_server", "ppocrv5_rec_server"
MARKER = "backbone.stages.0.blocks.0.att.conv.weight"
LIB = ROOT / "rapiddoc_amd" / "librapiddoc_mi355.so"


def _manifest(golden_dir, stem):
    return W.load_manifest(golden_dir / f"manifest_{stem}.json")


def test_manifests_are_the_reference_state_dicts(golden_dir):
    det, rec = _manifest(golden_dir, "ppocrv4_det_server"), _manifest(golden_dir, "ppocrv4_rec_server")
    count = lambda man: sum(int(__import__("numpy").prod(s)) for _n, s, d in man if d == "float32")
    assert len(det) == 417 and count(det) == 28486083
    assert len(rec) == 320 and count(rec) == 24184473
    for man in (det, rec):
        names = {n for n, _s, _d in man}
        assert MARKER in names and "backbone.stem.2.conv.weight" in names and "backbone.stages.2.blocks.1.layers.5.conv.weight" in names
    assert dict((n, s) for n, s, _d in rec)["head.ctc_head.fc.weight"] == (6625, 120)


def test_both_resolve_by_tensor_names_to_the_server_kinds(golden_dir):
    from rapiddoc_amd.session import resolve_det_kind, resolve_rec_kind
    for stem, resolve, kind in (("ppocrv4_det_server", resolve_det_kind, DET), ("ppocrv4_rec_server", resolve_rec_kind, REC)):
        names = [n for n, _s, _d in _manifest(golden_dir, stem)]
        assert resolve({n: None for n in names}) == kind
        assert resolve({"model." + n: None for n in names}) == kind                     # the prefix the reference strips
        small = {n: __import__("numpy").zeros((1,), "float32") for n in names}
        assert resolve(W.to_safetensors_bytes(small)) == kind
        assert resolve(W.to_safetensors_bytes({"model." + n: v for n, v in small.items()})) == kind


def test_non_backbone_parts_equal_the_v5_manifests_but_for_the_backbone_widths(golden_dir):
    def rest(stem):
        return {n: (s, d) for n, s, d in _manifest(golden_dir, stem) if not n.startswith("backbone.")}
    d4, d5 = rest("ppocrv4_det_server"), rest(DET)
    assert set(d4) == set(d5)
    assert sorted(n for n in d4 if d4[n] != d5[n]) == ["neck.ins_conv.0.weight", "neck.ins_conv.2.weight", "neck.ins_conv.3.weight"]
    assert [d4[f"neck.ins_conv.{i}.weight"][0] for i in range(4)] == [(256, c, 1, 1) for c in (256, 512, 768, 1024)]
    r4, r5 = rest("ppocrv4_rec_server"), rest(REC)
    assert set(r4) == set(r5)
    diff = {n.rsplit(".", 1)[0] for n in r4 if r4[n] != r5[n]}
    enc = "head.ctc_encoder.encoder."
    # a 1024-channel backbone output: conv1 / conv4 halve (1024 -> 128, 2048 -> 128), conv2 and conv1x1 read 128, conv3 returns 1024; 6625 classes
    assert diff == {enc + "conv1.conv", enc + "conv1.norm", enc + "conv2.conv", enc + "conv3.conv", enc + "conv3.norm", enc + "conv4.conv",
                    enc + "conv4.norm", enc + "conv1x1.conv", "head.ctc_head.fc"}, sorted(diff)
    assert r4[enc + "conv1.conv.weight"][0] == (128, 1024, 1, 3) and r5[enc + "conv1.conv.weight"][0] == (256, 2048, 1, 3)
    assert r4["head.ctc_head.fc.weight"][0] == (6625, 120) and r5["head.ctc_head.fc.weight"][0] == (18385, 120)


def test_summary_meets_the_generators_gates(golden_dir):
    s = json.loads((golden_dir / "summary_v4_server.json").read_text())
    assert s["gates"] == {"min_share": 0.75, "min_std": 0.15, "min_top2_gap": 1e-2, "min_gate_logit_std": 0.5}
    assert sorted(s["det"]["fixtures"]) == sorted(["b2_h64_w96", "b1_h160_w224", "b3_h96_w352"])
    for f in s["det"]["fixtures"].values():
        assert f["maps_share_05_95"] >= 0.75 and f["maps_std"] >= 0.15 and f["bytes"] <= 1 << 20
    assert {t: f["tokens"] for t, f in s["rec"]["fixtures"].items()} == {"b2_w64": 8, "b3_w104": 13, "b2_w100": 12, "b3_w320": 40}
    for f in s["rec"]["fixtures"].values():
        assert f["min_top2_gap"] >= 1e-2 and f["bytes"] <= 1 << 20
    for net in ("det", "rec"):
        assert len(s[net]["gate_logits"]) == 5
        for blk in s[net]["gate_logits"].values():
            assert blk["std"] >= 0.5 and blk["min"] < -2.0 and blk["max"] > 2.0
        man = _manifest(golden_dir, f"ppocrv4_{net}_server")
        st = W.synth_state_dict(man, 0, kind="ppocrv4_server")
        assert abs(W.checksum(st) - s[net]["checksum"]) < 1e-6 * max(1.0, abs(s[net]["checksum"]))


def test_the_gain_set_is_opt_in_and_touches_the_gate_weights_only(golden_dir):
    import numpy as np
    man = _manifest(golden_dir, "ppocrv4_rec_server")
    plain, gained = W.synth_state_dict(man, 0), W.synth_state_dict(man, 0, kind="ppocrv4_server")
    moved = sorted(n for n in plain if not np.array_equal(plain[n], gained[n]))
    assert moved == sorted(f"backbone.{b}.att.conv.weight" for b in ("stages.0.blocks.0", "stages.1.blocks.0", "stages.2.blocks.0", "stages.2.blocks.1",
                                                                      "stages.3.blocks.0"))
    assert np.array_equal(W.synth_state_dict(_manifest(golden_dir, REC), 0)["head.ctc_head.fc.weight"],
                          W.synth_tensor("head.ctc_head.fc.weight", (18385, 120), "float32", 0))     # the default draw is unchanged


def test_new_symbols_sources_and_docs():
    from rapiddoc_amd import _lib, build, engine
    assert "kernels_conv3x3_wide.hip" in build.SOURCES and "kernels_ese.hip" in build.SOURCES
    assert (build.CSRC / "kernels_conv3x3_wide.hip").exists() and (build.CSRC / "kernels_ese.hip").exists()
    assert "rd_backbone_name" in _lib.SYMBOLS
    assert {"rd_debug_conv3x3_wide", "rd_debug_ese", "rd_debug_maxpool3x3s2"} <= set(_lib.DEBUG_SYMBOLS)
    assert isinstance(engine.RdEngine.backbone, property) and engine.RdEngine.backbone.fset is None
    assert len(engine.KINDS) == 14 and DET in engine.KINDS and REC in engine.KINDS           # no new kind
    readme, integ = (ROOT / "README.md").read_text(), (ROOT / "INTEGRATION.md").read_text()
    assert "RD_CONV3X3_WIDE" in readme and "ch_PP-OCRv4_det_server" in readme and "ch_PP-OCRv4_rec_server" in integ and "state dict" in integ
    header = (ROOT / "include" / "rapiddoc_mi355.h").read_text()
    assert re.search(r"const char\* rd_backbone_name\(rd_handle\* h\);", header)


def test_exported_from_the_library():
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    for sym in ("rd_backbone_name", "rd_debug_conv3x3_wide", "rd_debug_ese", "rd_debug_maxpool3x3s2"):
        assert re.search(rf"\bT {sym}\b", out), sym
    for sym in ("conv3x3_wide_shape_ok", "prepare_conv3x3_wide_weights", "launch_conv3x3_wide", "conv3x3_wide_applies", "launch_ese_gate", "launch_ese_apply",
                "launch_maxpool3x3s2"):
        assert sym in out, sym


def test_shape_predicate_takes_the_networks_shapes_and_nothing_beside_them():
    """rd::conv3x3_wide_shape_ok through its mangled name (host code: no HIP call is made)."""
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    sym = [ln.split()[-1] for ln in out.splitlines() if "conv3x3_wide_shape_ok" in ln]
    assert len(sym) == 1
    fn = getattr(C.CDLL(str(LIB)), sym[0])
    fn.restype, fn.argtypes = C.c_bool, [C.c_int] * 4
    for cin, cout in ((64, 128), (128, 128), (256, 160), (160, 160), (512, 192), (192, 192), (768, 192), (768, 224), (224, 224)):
        assert fn(3, 3, cin, cout), (cin, cout)
    for cin, cout in ((128, 96), (128, 288), (48, 128), (784, 128), (128, 144), (72, 128)):
        assert not fn(3, 3, cin, cout), (cin, cout)
    assert not fn(1, 1, 128, 128) and not fn(3, 1, 128, 128) and not fn(5, 5, 128, 128)


def test_route_is_asked_for_by_the_builder_and_refused_beyond_32_bit_offsets():
    """rd_debug_conv_route (host only): the shape alone never gives "c3w" - only the image bit a builder's opt-in sets does; with it, an
    image of 2^31 bytes (H W xld 4) or more goes back to the generic route, whatever the batch."""
    from rapiddoc_amd import _lib
    lib = C.CDLL(str(LIB))
    fn = lib.rd_debug_conv_route
    fn.restype, fn.argtypes = _lib.DEBUG_SYMBOLS["rd_debug_conv_route"]

    def route(n, h, w, cin, cout, images):
        name = C.create_string_buffer(32)
        assert fn(n, h, w, cin, cout, 3, 3, 1, 1, 1, 1, 1, 1, images, 0, 0, 1, name, 32) >= 0
        return name.value.decode()

    for cin, cout in ((64, 128), (128, 128), (256, 160), (512, 192), (768, 224)):
        assert route(2, 24, 40, cin, cout, 1 | 16) == "c3w"
        assert route(2, 24, 40, cin, cout, 1 | 4) != "c3w" and route(2, 24, 40, cin, cout, 1) != "c3w"       # (192 -> 192 of the B6 encoder: it stays)
    assert route(1, 2047, 2048, 128, 128, 1 | 16) == "c3w" and route(32, 2047, 2048, 128, 128, 1 | 16) == "c3w"     # 2^31 - 2^20 bytes per image
    assert route(1, 2048, 2048, 128, 128, 1 | 16) != "c3w" and route(1, 4096, 4096, 64, 128, 1 | 16) != "c3w"
    assert route(2, 24, 40, 64, 96, 1 | 4 | 16) == "c3h1"                                                     # below the new kernel's widths
