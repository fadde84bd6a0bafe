"""GPU: the plans of every engine kind are what they were before the host code was split (engine.cpp -> engine / builder / builder_mobile, shared
builder helpers, one model table in models.cpp).  tests/golden/op_lists_all_kinds.json.gz (gzipped JSON) holds, recorded from the parent commit by `record()` below,
(name, kind, cfg, shape, flops, bytes) of every op of one small shape per kind: the whole forward in the default precision and after
set_precision("fp32"); for the recognisers also the REC_STAGE_BACKBONE plan, the REC_STAGE_TAIL plan and, where the kind serves it, the
REC_STAGE_BACKBONE | REC_LINE_WIDTHS plan.  A refactor of the builders must leave every list equal, entry by entry."""
import gzip
import json
import os

import pytest
import torch

from rapiddoc_amd import weights as W

pytestmark = pytest.mark.gpu

FIXTURE = "op_lists_all_kinds.json.gz"
# kind -> (manifest stem, opt-in gains of synth_state_dict as the kind's own GPU tests pass them, input shape)
CASES = {
    "ppocrv6_det": ("ppocrv6_det", None, (1, 3, 96, 160)),
    "ppocrv5_det_server": ("ppocrv5_det_server", None, (1, 3, 96, 160)),
    "ppocrv5_det_mobile": ("ppocrv5_det_mobile", "ppocrv5_det_mobile", (1, 3, 96, 160)),
    "ppocrv3_det_mobile": ("ppocrv3_det_mobile", "ppocrv3_det_mobile", (1, 3, 96, 160)),
    "ppocr_cls_mobile": ("ppocr_cls_mobile", "ppocr_cls_mobile", (2, 3, 48, 192)),
    "unitable_encoder": ("unitable_encoder", None, (1, 3, 32, 48)),
    "ppocrv6_rec": ("ppocrv6_rec", None, (3, 3, 48, 320)),
    "ppocrv5_rec_server": ("ppocrv5_rec_server", None, (3, 3, 48, 320)),
    "ppocrv5_rec_mobile": ("ppocrv5_rec_mobile", None, (3, 3, 48, 320)),
    "ppocr_rec_mv1e": ("ppocr_rec_mv1e_korean", "ppocr_rec_mv1e", (3, 3, 48, 320)),
    "pphgnetv2_b4": ("pphgnetv2_b4", None, (1, 3, 128, 160)),
    "pphgnetv2_b6_formula": ("pphgnetv2_b6_formula", None, (1, 3, 96, 128)),
}
REC_KINDS = ("ppocrv6_rec", "ppocrv5_rec_server", "ppocrv5_rec_mobile", "ppocr_rec_mv1e")
REC_LINES_KINDS = ("ppocrv6_rec", "ppocrv5_rec_mobile", "ppocr_rec_mv1e")     # ppocrv5_rec_server refuses REC_LINE_WIDTHS
LINE_WIDTHS = (320, 200, 96)                                                  # the three lines of the REC_LINE_WIDTHS plan


def _plans(eng, kind, shape):
    """name -> callable that runs one forward of that plan"""
    from rapiddoc_amd.engine import rec_line_table
    x = torch.zeros(shape, device="cuda")
    whole = {"ppocr_cls_mobile": eng.cls_forward, "unitable_encoder": eng.table_encoder_forward, "pphgnetv2_b4": eng.backbone_forward,
             "pphgnetv2_b6_formula": eng.formula_encoder_forward}.get(kind, eng.rec_forward if kind in REC_KINDS else eng.det_forward)
    plans = {"forward": lambda: whole(x)}
    if kind in REC_KINDS:
        B, T, dim = shape[0], eng._l.rd_rec_seq_len(shape[3]), eng.rec_token_dim
        plans["backbone"] = lambda: eng.rec_backbone_forward(x)
        plans["tail"] = lambda: eng.rec_tail_forward(torch.zeros((B * T, dim), device="cuda"), [T] * B)
        if kind in REC_LINES_KINDS:
            Ts = [eng._l.rd_rec_seq_len(w) for w in LINE_WIDTHS]
            tab = torch.from_numpy(rec_line_table(LINE_WIDTHS, [sum(Ts[:i]) for i in range(len(Ts))])).cuda()
            plans["backbone_lines"] = lambda: eng.rec_backbone_forward_lines(x, tab, torch.zeros((sum(Ts), dim), device="cuda"))
    return plans


def _ops_of(eng, run):
    eng.set_profiling(True)
    eng.profile_log.clear()
    run()
    eng.set_profiling(False)
    return [[r["name"], r["kind"], r["cfg"], r["shape"], r["flops"], r["bytes"]] for r in eng.profile_log]


def record_kind(golden_dir, kind):
    """{"shape": [...], "default": {plan: ops}, "fp32": {plan: ops}} of one kind, with RD_PRECISION and every RD_* switch out of the
    environment for the duration (the lists are those of the default routes)."""
    from rapiddoc_amd.engine import RdEngine
    stem, gains, shape = CASES[kind]
    # Every RD_* variable the library reads today is a developer switch of a route or of the precision (getenv("RD_...") in csrc/), so
    # all of them go, not a list that the next switch would be missing from.  None selects a library or a device; one that ever does
    # must be kept here.  The variables come back in `finally`.
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("RD_")}
    try:
        st = W.synth_state_dict(W.load_manifest(golden_dir / f"manifest_{stem}.json"), 0, kind=gains)
        eng = RdEngine(kind, guard="off").load_weights(st)
        out = {"shape": list(shape)}
        for precision in ("default", "fp32"):
            if precision == "fp32":
                eng.set_precision("fp32")
            out[precision] = {name: _ops_of(eng, run) for name, run in _plans(eng, kind, shape).items()}
        torch.cuda.synchronize()
        eng.close()
        return out
    finally:
        os.environ.update(saved)


def record(golden_dir):
    return {kind: record_kind(golden_dir, kind) for kind in CASES}


@pytest.fixture(scope="module")
def want(golden_dir):
    return json.loads(gzip.decompress((golden_dir / FIXTURE).read_bytes()))


def test_the_fixture_covers_every_engine_kind(want):
    from rapiddoc_amd import engine
    assert sorted(want) == sorted(CASES) == sorted(k for k in engine.KINDS if k not in ("unitable_decoder", "ppformulanet_head"))
    for kind, rec in want.items():
        plans = ["forward"] + (["backbone", "tail"] if kind in REC_KINDS else []) + (["backbone_lines"] if kind in REC_LINES_KINDS else [])
        assert rec["shape"] == list(CASES[kind][2])
        for precision in ("default", "fp32"):
            assert list(rec[precision]) == plans, (kind, precision)
            assert all(len(ops) >= 1 and all(len(op) == 6 for op in ops) for ops in rec[precision].values()), (kind, precision)


@pytest.mark.parametrize("kind", list(CASES))
def test_plans_of_every_kind_are_what_they_were(golden_dir, want, kind):
    got = record_kind(golden_dir, kind)
    assert got["shape"] == want[kind]["shape"]
    for precision in ("default", "fp32"):
        for plan, ops in want[kind][precision].items():
            have = got[precision][plan]
            assert len(have) == len(ops), (kind, precision, plan, len(have), len(ops))
            for i, (a, b) in enumerate(zip(have, ops)):
                assert a == b, (kind, precision, plan, i, a, b)
        assert list(got[precision]) == list(want[kind][precision]), (kind, precision)
