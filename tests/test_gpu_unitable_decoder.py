"""GPU: the UniTable decoder (`unitable_decoder`, csrc/table_decoder.hip), its loop and the class.

Step, through the developer entry `rd_debug_table_decode` with the tokens the reference fed: the hidden row after each block and the logits
of every step within 1e-3 max(1, max|ref|) of the reference-minted fixtures (free runs at S = 6 and 784, the forced run at S = 39, the bbox
variant), the chosen id equal at every step of the fixture's `compare` mask (whitelist top-2 gap >= 10 x the logit bound).  Three tables
together against each alone.  Loop, through `rd_table_decode`: the bbox and EOS variants give the reference's ids, lengths and padding;
`max_new_tokens` caps a table that never stops; B = 9 is declined with a message; a NaN memory row yields in-vocabulary ids.  The class:
`forward_tensor` on a 448 x 448 input gives the ids, structure and boxes the mint recorded from the reference's encoder, decoder, loop and
host functions; the class as `table_model` of analyze.PageAnalyzer puts its HTML on the table detection.

The loop tests compare every id of a free run: their fixtures' seeds were accepted under the loop rule of the mint (LOOP_RULES in
tests/golden/make_golden_unitable.py: EOS at least 0.1 from winning or losing, every other decision at least 0.02 wide, against an engine
logit error of 1e-5), not under the 10 x bound rule of the step tests' `compare` mask."""
import numpy as np
import pytest
import torch

import unitable_reference as R
from rapiddoc_amd import table_unitable as TU

pytestmark = pytest.mark.gpu
IDS = TU.STAND_IN_IDS
_ENG = {}


def _decoder(golden_dir, g=None):
    variant = str(g["variant"]) if g is not None else "plain"
    if variant not in _ENG:
        from rapiddoc_amd.engine import RdEngine
        _ENG[variant] = RdEngine(R.DEC_KIND).load_weights(R.dec_state(golden_dir, g))
    return _ENG[variant]


@pytest.mark.parametrize("tag", ["free_s6", "free_s784", "forced_s39", "bbox_s6"])
def test_step_matches_the_reference_fixtures(golden_dir, tag):
    mem, g = R.dec_fixture(golden_dir, tag)
    toks = R.fed_tokens(g)
    n = len(toks)
    out = _decoder(golden_dir, g).table_decode_debug(torch.from_numpy(mem), IDS, n, forced=torch.tensor([toks], dtype=torch.int32))
    msgs = []
    for name, got, ref in (("hidden", out["hidden"][:, :, 0, ::4].cpu(), torch.from_numpy(g["hidden"][:n, :, 0])),
                           ("logits", out["logits"][:, 0].cpu(), torch.from_numpy(g["logits"][:n, 0]))):
        err, bound = float((got - ref).abs().max()), R.FIXTURE_TOL * max(1.0, float(ref.abs().max()))
        msgs.append(f"{name} {err:.2e} / {bound:.2e}")
        assert err <= bound, (tag, name, err, bound)
    print(f"\n[unitable decoder {tag}] max-abs errors over {n} steps: " + ", ".join(msgs))
    cmp_ = g["compare"][:n, 0]
    assert np.array_equal(out["chosen"][:, 0].cpu().numpy()[cmp_], g["chosen"][:n, 0][cmp_])


def test_three_tables_together_equal_each_alone(golden_dir):
    mem, g = R.dec_fixture(golden_dir, "eos_b3_s6")
    dec = _decoder(golden_dir)
    steps = 24
    forced = torch.tensor([R.fed_tokens(np.load(golden_dir / "unitable_dec_seed0_free_s6.npz"))[:steps]] * 3, dtype=torch.int32)
    both = dec.table_decode_debug(torch.from_numpy(mem), IDS, steps, forced=forced)
    both = {k: v.clone() for k, v in both.items()}
    equal = True
    for b in range(3):
        one = dec.table_decode_debug(torch.from_numpy(mem[b:b + 1].copy()), IDS, steps, forced=forced[b:b + 1])
        lg3, lg1 = both["logits"][:, b], one["logits"][:, 0]
        bound = R.FIXTURE_TOL * max(1.0, float(lg1.abs().max()))
        assert float((lg3 - lg1).abs().max()) <= bound
        assert float((both["hidden"][:, :, b] - one["hidden"][:, :, 0]).abs().max()) <= R.FIXTURE_TOL * max(1.0, float(one["hidden"].abs().max()))
        assert torch.equal(both["chosen"][:, b], one["chosen"][:, 0])
        equal = equal and torch.equal(lg3, lg1)
    print(f"\n[unitable decoder B = 3 against B = 1] logits bit-equal: {equal}")


def test_loop_bbox_rule_and_the_cap(golden_dir):
    mem, g = R.dec_fixture(golden_dir, "bbox_s6")
    dec = _decoder(golden_dir, g)
    ids, n = dec.table_decode(torch.from_numpy(mem), IDS, 24)
    ids = ids.cpu().numpy()[0]
    assert n == [25] and ids[0] == IDS.prefix                 # never stops: capped at max_new_tokens
    assert all((t == IDS.bbox_close) == (i % 5 == 4) for i, t in enumerate(ids[1:]))
    assert all(IDS.bbox_first <= t <= IDS.bbox_last for i, t in enumerate(ids[1:]) if i % 5 != 4)
    ref = g["ids"][0]
    upto = int(np.argmin(g["compare"][:, 0])) if not g["compare"][:, 0].all() else 24       # equal ids while every decision was wide enough
    assert np.array_equal(ids[:upto + 1], ref[:upto + 1])
    ids10, n10 = dec.table_decode(torch.from_numpy(mem), IDS, 10)
    assert n10 == [11] and ids10.shape == (1, 11) and np.array_equal(ids10.cpu().numpy()[0], ids[:11])


def test_loop_eos_latch_lengths_and_padding(golden_dir):
    mem, g = R.dec_fixture(golden_dir, "eos_b3_s6")
    dec = _decoder(golden_dir, g)
    ids, n = dec.table_decode(torch.from_numpy(mem), IDS, 100)
    ids = ids.cpu().numpy()
    for b in range(3):
        ref = [int(v) for v in g["ids"][b] if v >= 0]
        assert n[b] == len(ref) and ids[b, :n[b]].tolist() == ref and ref[-1] == IDS.eos
        assert bool((ids[b, n[b]:] == IDS.pad).all())
        alone, n1 = dec.table_decode(torch.from_numpy(mem[b:b + 1].copy()), IDS, 100)
        assert n1 == [n[b]] and alone.cpu().numpy()[0, :n[b]].tolist() == ref
    assert len(set(n)) == 3


def test_batches_above_eight_are_declined_with_a_message(golden_dir):
    from rapiddoc_amd.engine import EngineError
    dec = _decoder(golden_dir)
    with pytest.raises(EngineError, match="1 .. 8 tables"):
        dec.table_decode(torch.zeros((9, 6, 768)), IDS, 4)
    with pytest.raises(EngineError, match="max_new_tokens"):
        dec.table_decode(torch.zeros((1, 6, 768)), IDS, 1025)


def test_nan_memory_gives_in_vocabulary_ids(golden_dir):
    mem, _ = R.dec_fixture(golden_dir, "free_s6")
    bad = mem.copy()
    bad[0, 2] = np.nan
    ids, n = _decoder(golden_dir).table_decode(torch.from_numpy(bad), IDS, 12)
    ids = ids.cpu().numpy()
    assert ids.shape == (1, 13) and bool(((ids >= 0) & (ids < 960)).all())


def _class448(golden_dir):
    """(the class on the EOS variant the mint tuned for the 448 x 448 input, that input, the recorded expectation)"""
    import json
    from rapiddoc_amd import weights as W
    exp = json.loads((golden_dir / "summary_unitable.json").read_text())["decoder"]["class448"]
    if "cls448" not in _ENG:
        st = dict(R.dec_state(golden_dir))
        b = st["generator.bias"].copy()
        b[IDS.eos] += np.float32(exp["bias_add"])
        st["generator.bias"] = b
        _ENG["cls448"] = TU.Mi355UniTableStructure(R.state(golden_dir), st, IDS, TU.stand_in_tokens(), max_new_tokens=64)
    return _ENG["cls448"], W.synth_normal_image(int(exp["x_seed"]), 1, 448, 448), exp


def test_class_forward_tensor_gives_the_reference_structure_and_boxes(golden_dir):
    """The expectation is the mint's: reference encoder -> the loop around the reference decoder -> the reference's own decode_tokens,
    rescale_bboxes and wrap_with_html_struct, on the same 448 x 448 input.  Ids first (the hand-off and the length), then what the class returns."""
    cls, x, exp = _class448(golden_dir)
    xd = torch.from_numpy(x).cuda()
    assert cls.decode_ids(xd) == [exp["ids"]]
    assert exp["ids"][0] == IDS.prefix and exp["ids"][-1] == IDS.eos and 22 <= len(exp["ids"]) <= 62
    struct, boxes = cls.forward_tensor(xd, [tuple(exp["ori_hw"])])
    assert struct == [(exp["wrapped"], 1.0)]
    assert len(boxes) == 1 and boxes[0].dtype == np.float32 and boxes[0].tolist() == exp["boxes"]


def test_class_runs_inside_the_table_seam_of_the_page_driver(golden_dir):
    """analyze.PageAnalyzer with a stub layout that reports one table: the class is the `table_model` (seam S1: `batch_predict(crops,
    fill_image_res_list=...) -> list[str]`), the driver crops the table from the page, and the HTML lands on that detection."""
    import json
    from rapiddoc_amd import weights as W
    from rapiddoc_amd.analyze import PageAnalyzer, table_crop_rect
    from rapiddoc_amd.layout_model import LayoutModel
    from rapiddoc_amd.pages import synth_batch
    from rapiddoc_amd.pipeline import PagePipeline
    cls, _, _ = _class448(golden_dir)
    maps = json.loads((golden_dir / "layout_category_maps.json").read_text())
    labels = list(maps["label_to_category"]["pp_doclayoutv2"])
    TAB = (80, 500, 1150, 1000)

    class Session:
        characters = labels

        def __call__(self, x, sf):
            rows = [[labels.index("table"), 0.9, *TAB, 0]] * x.shape[0]
            return [np.asarray(rows, np.float32), np.full(x.shape[0], 1, np.int32)]

    seen = []

    class Spy:                      # the class itself, with the crops it is handed recorded
        def batch_predict(self, crops, **kwargs):
            seen.append((crops, kwargs))
            return cls.batch_predict(crops, **kwargs)

    states = {k: W.synth_state_dict(W.load_manifest(golden_dir / f"manifest_{k}.json"), 0) for k in ("ppocrv6_det", "ppocrv6_rec")}
    an = PageAnalyzer(LayoutModel(Session(), "pp_doclayoutv3"), PagePipeline(states, n_rec_streams=2), table_model=Spy())
    pages_np, _ = synth_batch(0, 1)
    out = an(torch.from_numpy(pages_np).cuda(), page_scales=[2.0])[0]
    table = [d for d in out if d["category_id"] == 5][0]
    assert len(seen) == 1 and len(seen[0][0]) == 1 and "fill_image_res_list" in seen[0][1]
    crop = seen[0][0][0]
    assert crop.dtype == np.uint8 and crop.shape == (TAB[3] - TAB[1], TAB[2] - TAB[0], 3)
    html = table["html"]
    assert html.startswith("<html><body><table>") and html.endswith("</table></body></html>")
    assert html == cls.batch_predict([crop])[0]
def test_class_has_the_shape_the_table_seam_takes(golden_dir):
    """seam S1 of analyze (`table_model.batch_predict(crops, fill_image_res_list=...) -> list[str]`): BGR uint8 crops of any size in, one
    HTML string per crop out"""
    _, g = R.dec_fixture(golden_dir, "eos_b3_s6")
    toks = TU.stand_in_tokens()
    cls = TU.Mi355UniTableStructure(R.state(golden_dir), R.dec_state(golden_dir, g), IDS, toks, max_new_tokens=64)
    rng = np.random.default_rng(0)
    crops = [rng.integers(0, 256, (120, 300, 3), dtype=np.uint8), rng.integers(0, 256, (64, 80, 3), dtype=np.uint8)]
    html = cls.batch_predict(crops, fill_image_res_list=[None, None])
    assert len(html) == 2 and all(isinstance(h, str) and h.startswith("<html><body><table>") and h.endswith("</table></body></html>") for h in html)
    assert cls.batch_predict([]) == []
