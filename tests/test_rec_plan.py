"""CPU: `rec_plan.plan_rec`, the recogniser stage's host arithmetic (needs the built library for the native batcher, no GPU).

1. It plans what the one-body stage planned: tests/golden/rec_plan_parent.npz was recorded on the GPU at the commit before the stage was
   split (tests/golden/make_golden_rec_plan.py) - descriptor bytes, scratch layout, launches, widths, key sort, line table and the padded
   tail calls, all bit for bit, with the native and the Python batcher.
2. What that commit did not expose (the warp launches, the second descriptor arrays, the token ranges) holds as invariants, on the
   fixture's cases and on the benchmark's own 1440 lines.
3. The width collective is called exactly once per plan at each of its four exits."""
import json
from pathlib import Path

import numpy as np
import pytest

from rapiddoc_amd.engine import ragged_tables
from rapiddoc_amd.rec_plan import LINE_DTYPE, plan_rec

GOLDEN = Path(__file__).resolve().parent / "golden" / "rec_plan_parent.npz"
CASE_NAMES = ["a", "b", "c", "d", "e", "f"]


def load_cases():
    """name -> dict(sources=[(image shape, quads per image)], image_keys, kw=the constructor arguments, two_stage, n_cu, S,
    rec_lines_in_launch, kinds, texts, and the recorded arrays)."""
    z = np.load(GOLDEN)
    meta = json.loads(bytes(z["meta"]).decode())
    sets = {}
    for name, m in meta["sets"].items():
        cuts = np.cumsum([0] + [c for counts in m["counts"] for c in counts])
        per_img = [z[f"{name}/quads"][a:e] for a, e in zip(cuts[:-1], cuts[1:])]
        sources, i = [], 0
        for shape, counts in zip(m["shapes"], m["counts"]):
            sources.append((tuple(shape), per_img[i: i + len(counts)]))
            i += len(counts)
        sets[name] = (sources, m["image_keys"])
    cases = {}
    for name, c in meta["cases"].items():
        c = dict(c)
        c["sources"], c["image_keys"] = sets[c["set"]]
        c.update({k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")})
        cases[name] = c
    return cases


def plan_arguments(case):
    """The keyword arguments PagePipeline derives from its constructor arguments (pipeline.PagePipeline.__init__), restated."""
    kw = case["kw"]
    mode = kw.get("rec_mode") or ("strict" if "rec_batch_num" not in kw and "rec_chunking" not in kw else "throughput")
    chunking = kw.get("rec_chunking") or ("adaptive" if "rec_batch_num" not in kw else "fixed")
    strict = mode == "strict"
    return dict(strict=strict, two_stage=case["two_stage"], lines_in_launch=case["rec_lines_in_launch"], chunking=chunking,
                rec_batch_num=6 if strict else kw.get("rec_batch_num", 64), rec_width_multiple=1 if strict else kw.get("rec_width_multiple", 32),
                n_cu=case["n_cu"], n_streams=case["S"])


def plan_of(case, **over):
    return plan_rec([(shape[0], quads) for shape, quads in case["sources"]], case["image_keys"], **{**plan_arguments(case), **over})


@pytest.fixture(scope="module")
def cases():
    return load_cases()


@pytest.mark.parametrize("host_native", [True, False])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_plans_what_the_one_body_stage_planned(cases, name, host_native):
    c = cases[name]
    p = plan_of(c, host_native=host_native)
    same = lambda got, want: np.asarray(got).shape == want.shape and np.asarray(got).astype(want.dtype).tobytes() == want.tobytes()      # noqa: E731
    assert p.descs.dtype == LINE_DTYPE and p.descs.tobytes() == c["descs"].tobytes()
    assert same(p.batch_base, c["batch_base"]) and same(p.starts, c["starts"])
    assert same(p.line_ids, c["ids"]) and same(p.keep, c["keep"]) and p.n == len(c["keep"]) == p.n_all - 2
    assert same(p.crop_w, c["crop_w"]) and same(p.crop_h, c["crop_h"]) and same(p.rot90, c["rot90"]) and int(p.descs["rot90"].sum()) >= 1
    assert [w for _c, w in p.batches] == c["launch_w"].tolist()
    assert [len(ch) for ch, _w in p.batches] == np.diff(c["starts"]).tolist()
    if c["image_keys"] is None:
        assert p.perm is None and len(c["perm"]) == 0
    else:
        assert same(p.perm, c["perm"]) and not np.array_equal(p.perm, np.arange(len(p.perm)))
    if "line_w" in c:           # strict two-stage: every line at its own reference width
        assert p.lines_mode and same(p.line_w, c["line_w"])
    else:                       # every line as wide as its launch
        assert not p.lines_mode and same(p.line_w, np.repeat(c["launch_w"], np.diff(c["starts"])))
    if "linetab" in c:
        assert p.linetab.dtype == np.int32 and same(p.linetab, c["linetab"]) and same(p.first_tok, c["linetab"][:, 3])
    else:
        assert p.linetab is None
    if c["two_stage"]:          # the tail calls: the padded line lengths and the two tables the engine uploads for them
        assert [len(lp) for lp, _t in p.group_pad] == c["tail_n"].tolist()
        assert same(np.concatenate([lp for lp, _t in p.group_pad]), c["tail_lens"])
        cuts = np.cumsum([0] + c["tail_n"].tolist())
        for (lp, _t), a, e in zip(p.group_pad, cuts[:-1], cuts[1:]):
            for got, want in zip(ragged_tables(lp), ragged_tables(c["tail_lens"][a:e])):
                assert got.tobytes() == want.tobytes()
    else:
        assert p.groups is None and p.first_tok is None
    if name in ("a", "b"):
        assert len(p.batches) >= 3 and len(p.groups[-1]) < c["S"] == len(p.groups[0])     # a full group and a partial one


def check_invariants(p, n_sources, S, use_cls):
    n, starts = p.n, p.starts
    assert sorted(p.order_all.tolist()) == list(range(n)) and np.array_equal(p.line_ids, p.keep[p.order_all])
    d = p.descs
    crop_bytes = (d["crop_w"].astype(np.int64) * d["crop_h"] * 3 + 15) // 16 * 16
    assert p.batch_base[0] == 0 and len(p.batch_base) == len(p.batches) + 1 == len(starts) and p.scratch_bytes == int(crop_bytes.sum())
    warp = d if p.descs_warp is None else p.descs_warp
    assert (p.descs_warp is None) == (n_sources == 1)
    for b, (chunk, w) in enumerate(p.batches):
        lo, hi = int(starts[b]), int(starts[b + 1])
        assert np.array_equal(p.order_all[lo:hi], chunk)
        assert (1 <= d["out_w"][lo:hi]).all() and (d["out_w"][lo:hi] <= p.line_w[lo:hi]).all() and (p.line_w[lo:hi] <= w).all()
        # scratch regions: 16-byte aligned, back to back in descriptor order, the launch's base the running sum
        off = d["scratch_off"][lo:hi].astype(np.int64)
        assert (off % 16 == 0).all() and np.array_equal(off, np.cumsum(crop_bytes[lo:hi]) - crop_bytes[lo:hi])
        assert int(p.batch_base[b + 1] - p.batch_base[b]) == int(crop_bytes[lo:hi].sum())
        # warp jobs: the launch's descriptors exactly once, grouped by source, max_px the maximum over the job
        jobs = p.warp_jobs[b]
        assert [j[1] for j in jobs] == [lo] + [j[1] + j[2] for j in jobs[:-1]] and jobs[-1][1] + jobs[-1][2] == hi
        assert [j[0] for j in jobs] == sorted(set(j[0] for j in jobs))
        src_launch = p.src_of[p.keep][p.order_all[lo:hi]]
        for si, first, cnt, max_px in jobs:
            w_ = warp[first: first + cnt]
            assert cnt == int((src_launch == si).sum()) and max_px == int((w_["crop_w"].astype(np.int64) * w_["crop_h"]).max())
        assert sorted(warp[lo:hi].tobytes()[i: i + 96] for i in range(0, 96 * (hi - lo), 96)) == \
            sorted(d[lo:hi].tobytes()[i: i + 96] for i in range(0, 96 * (hi - lo), 96))
    if use_cls:
        want = np.minimum(192, np.ceil(48 * (p.eff_w / p.eff_h)[p.order_all])).astype(np.int32)
        assert np.array_equal(p.descs_cls["out_w"], want)
        rest = [f for f in LINE_DTYPE.names if f != "out_w"]
        assert all(np.array_equal(p.descs_cls[f], d[f]) for f in rest)
    else:
        assert p.descs_cls is None
    if not p.two_stage:
        return
    w2 = (np.asarray(p.line_w, np.int64) - 1) // 2 + 1
    assert np.array_equal(p.seq_line, ((w2 - 1) // 2 + 1) // 2)
    assert p.groups == [list(range(g, min(g + S, len(p.batches)))) for g in range(0, len(p.batches), S)]
    for gi, grp in enumerate(p.groups):
        lo, hi = int(starts[grp[0]]), int(starts[grp[-1] + 1])
        # token ranges: back to back from the group's base (so disjoint), ending inside the group's padded span
        assert p.first_tok[lo] == p.group_base[gi] and np.array_equal(p.first_tok[lo + 1: hi], (p.first_tok + p.seq_line)[lo: hi - 1])
        assert p.first_tok[hi - 1] + p.seq_line[hi - 1] <= p.group_base[gi + 1]
        assert [p.tok_lo[bi] for bi in grp] == [int(p.first_tok[int(starts[bi])]) for bi in grp]
        lp, T = p.group_pad[gi]
        assert np.array_equal(lp[: hi - lo], p.seq_line[lo:hi]) and np.array_equal(p.group_lens[gi], p.seq_line[lo:hi])
        assert len(lp) % 32 == 0 and int(lp.sum()) % 256 == 0 and T % 8 == 0 and T >= int(lp.max()) and T - 8 < int(p.seq_line[lo:hi].max())
        assert len(lp) > hi - lo and (lp[hi - lo:] >= 1).all() and (lp[hi - lo:] <= T).all()
        assert int(p.group_base[gi + 1] - p.group_base[gi]) == int(lp.sum())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_invariants_of_what_the_fixture_does_not_hold(cases, name):
    c = cases[name]
    use_cls = name in ("b", "e")
    check_invariants(plan_of(c, use_cls=use_cls), len(c["sources"]), c["S"], use_cls)


def test_the_benchmarks_own_lines():
    """bench.py's page batch: pages.synth_pages(range(32)) -> 1440 lines, strict two-stage at 256 CUs and 4 streams: 15 launches in 4 groups."""
    from rapiddoc_amd.pages import synth_pages
    from rapiddoc_amd.pipeline import boxes_to_quads
    _pages, boxes = synth_pages(list(range(32)))
    quads = [boxes_to_quads(b) for b in boxes]
    assert sum(len(q) for q in quads) == 1440
    for native in (True, False):
        p = plan_rec([(32, quads)], None, strict=True, two_stage=True, lines_in_launch=True, chunking="adaptive", rec_batch_num=6,
                     rec_width_multiple=1, n_cu=256, n_streams=4, use_cls=True, host_native=native)
        assert p.n == p.n_all == 1440 and len(p.batches) == 15 and len(p.groups) == 4 and p.lines_in_launch
        check_invariants(p, 1, 4, True)


class CountingSync:
    def __init__(self):
        self.calls = []

    def __call__(self, keys, ratios):
        from rapiddoc_amd import ocr_host
        self.calls.append((keys, ratios))
        return ocr_host.rec_reference_widths(list(ratios))


def test_the_width_collective_is_called_once_at_every_exit(cases):
    c = cases["b"]
    kw = plan_arguments(c)
    normal = [(shape[0], quads) for shape, quads in c["sources"]]
    flat = np.array([[0, 0], [5, 5], [10, 10], [20, 20]], np.float64)                # collinear corners: no crop exists
    exits = {"no sources": ([], None), "no quads": ([(2, [np.zeros((0, 4, 2)), []]), (1, [[]])], None),
             "every quad degenerate": ([(2, [np.zeros((3, 4, 2)), flat[None]])], [[5, 1]]), "normal": (normal, c["image_keys"])}
    for what, (sources, keys) in exits.items():
        sync = CountingSync()
        p = plan_rec(sources, keys, width_sync=sync, **kw)
        assert len(sync.calls) == 1, what
        k, r = sync.calls[0]
        assert k.dtype == np.int64 and r.dtype == np.float64 and k.ndim == r.ndim == 1 and len(k) == len(r) == p.n, what
        assert (p.n == 0) == (what != "normal") and p.n_img == [s[0] for s in sources]
        assert p.n_all == sum(len(q) for _k, qs in sources for q in qs) == len(p.src_of) == len(p.page_of)
        if what == "normal":        # the keys are the image keys of the kept lines in pooled order, the widths are the answer's
            assert np.array_equal(k, np.sort(k)) and set(k.tolist()) == {0, 1, 2}       # (the image with key 3 has no line)
            assert np.array_equal(p.line_w, plan_rec(sources, keys, **kw).line_w)     # (this stand-in answers with the local rule)
        plan_rec(sources, keys, **kw)                                               # no callable, no call
        assert len(sync.calls) == 1


def test_errors_come_before_any_gpu_work(cases):
    c = cases["d"]
    with pytest.raises(RuntimeError, match="word boxes need the strict two-stage recogniser"):
        plan_of(c, want_words=True)
    big = np.array([[0, 0], [30000, 0], [30000, 30000], [0, 30000]], np.float64)
    with pytest.raises(RuntimeError, match=">= 2 GB of crop scratch"):
        plan_rec([(1, [big[None]])], None, **plan_arguments(cases["a"]))
