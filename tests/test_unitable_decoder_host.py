"""CPU: the host side of the UniTable decoder (`unitable_decoder`) - the manifest, a float64 restatement of the decoder graph against the
teacher-forced fixtures, the loop restatement (bbox rule, EOS) against the bbox and EOS fixture ids, `decode_tokens` / `rescale_bboxes` /
`wrap_with_html_struct` against recorded outputs of the reference's own functions on the stand-in vocabulary, the kind lists and symbols."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import unitable_reference as R
from rapiddoc_amd import table_unitable as TU
from rapiddoc_amd import weights as W

ROOT = Path(__file__).resolve().parents[1]
IDS = TU.STAND_IN_IDS


def test_manifest_is_the_reference_decoder(golden_dir):
    man = W.load_manifest(golden_dir / f"manifest_{R.DEC_KIND}.json")
    summary = json.loads((golden_dir / "summary_unitable.json").read_text())["decoder"]
    assert len(man) == 92 == summary["tensors"]
    assert sum(int(np.prod(s)) for _, s, _ in man) == 40_069_056 == summary["parameters"]
    shapes = {n: s for n, s, _ in man}
    assert shapes["token_embed.embedding.weight"] == (960, 768) and shapes["generator.weight"] == (960, 768)
    assert shapes["layers.3.self_attn.wqkv.weight"] == (2304, 768) and shapes["layers.0.multihead_attn.key.weight"] == (768, 768)
    assert W.checksum(R.dec_state(golden_dir)) == pytest.approx(summary["checksum"], rel=0, abs=1e-6)


def test_stand_in_vocabulary_matches_the_whitelist():
    toks = TU.stand_in_tokens()
    assert len(toks) == 960 and toks[IDS.eos] == "<eos>" and toks[IDS.bbox_close] == "]</td>" and toks[IDS.prefix] == "[html+bbox]"
    assert toks[IDS.bbox_first] == "bbox-0" and toks[IDS.bbox_last] == "bbox-448" and toks[60] == ' colspan="25"'
    assert len(R.WHITE) == 499 == 1 + len(TU.HTML_TOKENS) + 449


@pytest.mark.parametrize("tag", ["forced_s39", "free_s6", "bbox_s6"])
def test_float64_restatement_matches_the_teacher_forced_fixtures(golden_dir, tag):
    mem, g = R.dec_fixture(golden_dir, tag)
    toks = R.fed_tokens(g)
    hid, lg = R.decoder_forward(R.dec_state(golden_dir, g), mem[0], toks)
    n = len(toks)
    for name, got, ref in (("hidden", hid[:, :, ::4], torch.from_numpy(g["hidden"][:n, :, 0]).double()), ("logits", lg, torch.from_numpy(g["logits"][:n, 0]).double())):
        err, bound = float((got - ref).abs().max()), R.FIXTURE_TOL * max(1.0, float(ref.abs().max()))
        print(f"\n[unitable decoder {tag} float64] {name} {err:.2e} / {bound:.2e}")
        assert err <= bound, (tag, name, err, bound)
    cmp_ = g["compare"][:n, 0]
    assert np.array_equal(R.whitelist_argmax(lg.numpy())[cmp_], g["chosen"][:n, 0][cmp_])


@pytest.mark.parametrize("tag", ["bbox_s6", "eos_b3_s6"])
def test_loop_restatement_reproduces_the_fixture_ids(golden_dir, tag):
    """the rule, the EOS stop and nothing else: fed with the fixture's chosen tokens, the loop gives the fixture's contexts"""
    _, g = R.dec_fixture(golden_dir, tag)
    for b in range(g["ids"].shape[0]):
        chosen = [int(v) for v in g["chosen"][:, b] if v >= 0]
        it = iter(chosen)
        ctx = TU.loop_reference(lambda c: next(it), IDS, len(chosen))
        assert ctx == [int(v) for v in g["ids"][b] if v >= 0]
        if tag == "bbox_s6":
            assert all((t == IDS.bbox_close) == (i % 5 == 4) for i, t in enumerate(ctx[1:]))
        else:
            assert ctx[-1] == IDS.eos and ctx.count(IDS.eos) == 1
    if tag == "eos_b3_s6":
        lens = [int((g["ids"][b] >= 0).sum()) for b in range(3)]
        assert len(set(lens)) == 3 and all(7 <= n <= 62 for n in lens)


def test_the_counter_is_not_reset_by_other_tokens():
    seq = iter([61, 62, 20, 63, 64, 65, 30, 66, 1])
    ctx = TU.loop_reference(lambda c: next(seq), IDS)
    assert ctx == [11, 61, 62, 20, 63, 64, 14, 30, 66, 1]


def test_host_functions_against_the_reference_records(golden_dir):
    rec = json.loads((golden_dir / "summary_unitable.json").read_text())["decoder"]["host"]
    toks = TU.stand_in_tokens()
    assert set(rec) == {"two_rows", "span_no_box", "empty", "after_eos"}
    for name, r in rec.items():
        boxes, html = TU.decode_tokens(r["ids"], toks)
        assert html == r["html"], name
        assert boxes.dtype == np.float32 and boxes.tolist() == r["boxes"], name
        assert TU.wrap_with_html_struct(list(html)) == r["wrapped"]
        if len(boxes):
            assert TU.rescale_bboxes(600, 1000, boxes.copy()).tolist() == r["rescaled_600x1000"]
            assert TU.rescale_bboxes(100, 50, boxes.copy()).tolist() == r["rescaled_100x50"]


def test_preprocess_constants_are_the_reference_ones():
    assert TU.NORM_MEAN == (0.86597056, 0.88463002, 0.87491087) and TU.NORM_STD == (0.20686628, 0.18201602, 0.18485524)
    assert TU.IMG_SIZE == 448 and TU.MAX_SEQ_LEN == 1024


def test_kind_and_symbols_are_listed():
    from rapiddoc_amd import _lib, build, engine
    assert R.DEC_KIND in engine.KINDS and "table_decoder.hip" in build.SOURCES and "rd_table_decode" in _lib.SYMBOLS
    header = (ROOT / "include/rapiddoc_mi355.h").read_text()
    assert re.search(r"\brd_table_decode\s*\(", header) and "rd_table_decode_cfg" in header and f'"{R.DEC_KIND}"' in header
    build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(lib, "rd_table_decode") and hasattr(lib, "rd_debug_table_decode")
