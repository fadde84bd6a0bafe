"""GPU: the UniTable decode through refilled slots (rd_table_decode_stream, csrc/table_decoder.hip) against the batch path, the
reference-minted fixtures and the host restatement of its schedule (tests/stream_reference.py), then the class and the pooled table route.

The yardstick is the batch path (`rd_table_decode` / `rd_debug_table_decode`, itself pinned to the fixtures by
test_gpu_unitable_decoder.py), run over consecutive groups of `slots` tables - never the stream.

Mixed lengths: the EOS-variant state of unitable_dec_seed0_eos_b3_s6.npz on 20 memories default_rng(100 + i).standard_normal((6, 768)),
40 new tokens.  The float32 CPU restatement (unitable_reference.decoder_forward + table_unitable.loop_reference) gives the lengths
2 41 3 6 3 13 41 2 11 3 4 2 3 2 8 4 3 2 2 3 - eight distinct values, two of them at the cap.  The GPU may decide a narrow step differently,
so every test that needs the spread asserts it on the batch path's own lengths first; a failed precondition is a failure, not a skip."""
import copy
import ctypes as C
import json

import numpy as np
import pytest
import torch

import stream_reference as SR
import unitable_reference as R
from rapiddoc_amd import table_unitable as TU

pytestmark = pytest.mark.gpu

IDS = TU.STAND_IN_IDS
V, D, LAYERS = 960, 768, 4
ID_GUARD, LEN_GUARD, SENTINEL = -5, -7, -12345.0
N_MIX, S_MIX, NEW_MIX = 20, 6, 40
_ENG, _BATCH, _RUNS = {}, {}, {}


def decoder(golden_dir, tag):
    """the decoder engine on the variant state fixture `tag` names ("eos_b3_s6": EOS raised, "bbox_s6": the bbox ids raised)"""
    if tag not in _ENG:
        from rapiddoc_amd.engine import RdEngine
        _ENG[tag] = RdEngine(R.DEC_KIND).load_weights(R.dec_state(golden_dir, np.load(golden_dir / f"unitable_dec_seed0_{tag}.npz")))
    return _ENG[tag]


def mixed_memories(n=N_MIX):
    return np.stack([np.random.default_rng(100 + i).standard_normal((S_MIX, D)) for i in range(n)]).astype(np.float32)


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def lens_of(ids):
    """columns that count per row of ids [B][max_new + 1]: the first EOS's position plus one, or the whole row"""
    out = []
    for row in np.asarray(ids):
        eos = np.nonzero(row[1:] == IDS.eos)[0]
        out.append(int(eos[0]) + 2 if len(eos) else len(row))
    return np.asarray(out, dtype=np.int32)


def stream_run(eng, mem, max_new, slots, trace=False, expect_rc=0, n_claimed=None, mem_dev=None, side_stream=False):
    """One call with guard rows around both outputs.  Without `trace` it is the product entry, with it the developer entry and all three
    traces.  On a refusal (`expect_rc` != 0) the outputs are checked to be untouched and the message is returned.  `side_stream`: the call
    goes out on a stream of its own, where the step is captured into a graph and replayed (on the null stream it is launched directly)."""
    from rapiddoc_amd import _lib
    from rapiddoc_amd.engine import TableStreamStats
    m = torch.from_numpy(mem).cuda() if mem_dev is None else mem_dev
    N = m.shape[0] if n_claimed is None else n_claimed
    S = m.shape[1]
    rows, cols = max(N, 1), max(max_new, 0) + 1
    ids = torch.full((rows + 2, cols), ID_GUARD, dtype=torch.int64, device="cuda")
    lens = torch.full((rows + 2,), LEN_GUARD, dtype=torch.int32, device="cuda")
    st, cfg = TableStreamStats(), TU.cfg_struct(IDS)
    side = torch.cuda.Stream() if side_stream else None
    lib, stream = _lib.load(), (side.cuda_stream if side_stream else torch.cuda.current_stream().cuda_stream)
    assert not side_stream or stream != 0
    lg = hid = sched = None
    if trace:
        sched_steps = N * max_new + 8
        lg = torch.full((N, max_new, V), SENTINEL, device="cuda")
        hid = torch.full((N, max_new, LAYERS, D), SENTINEL, device="cuda")
        sched = torch.full((sched_steps, slots, 2), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if trace:
        rc = lib.rd_debug_table_decode_stream(eng._h, m.data_ptr(), N, S, max_new, slots, C.byref(cfg), ids[1:].data_ptr(), lens[1:].data_ptr(),
                                              C.byref(st), stream, lg.data_ptr(), hid.data_ptr(), sched.data_ptr(), sched_steps)
    else:
        rc = lib.rd_table_decode_stream(eng._h, m.data_ptr(), N, S, max_new, slots, C.byref(cfg), ids[1:].data_ptr(), lens[1:].data_ptr(),
                                        C.byref(st), stream)
    torch.cuda.synchronize()
    msg = eng._l.rd_last_error(eng._h).decode()
    if expect_rc == 0:
        assert rc == 0, msg
    else:
        assert rc != 0 and msg, (rc, msg)
        assert bool((ids == ID_GUARD).all()) and bool((lens == LEN_GUARD).all()), "a refused call wrote to its outputs"
        return {"msg": msg}
    assert bool((ids[0] == ID_GUARD).all()) and bool((ids[-1] == ID_GUARD).all()), "guard rows of ids"
    assert int(lens[0]) == LEN_GUARD and int(lens[-1]) == LEN_GUARD, "guard rows of lens"
    return dict(ids=ids[1:-1].cpu().numpy(), lens=lens[1:-1].cpu().numpy(), logits=lg, hidden=hid, sched=None if sched is None else sched.cpu().numpy(),
                stats=dict(steps=st.steps, live_slot_steps=st.live_slot_steps, slots=st.slots, admitted=st.admitted))


def batch_groups(golden_dir, tag, mem, max_new, group, key):
    """The yardstick: rd_debug_table_decode (the free loop) over consecutive groups of `group` tables, computed once per `key` and left
    unchanged.  Returns (ids [N][max_new + 1], lens [N], logits [N][max_new][960], hidden [N][max_new][4][768]); rows of steps a group's
    loop did not run are NaN."""
    key = (tag, key, max_new, group)
    if key not in _BATCH:
        eng = decoder(golden_dir, tag)
        ids, lg, hid = [], [], []
        for g0 in range(0, mem.shape[0], group):
            out = eng.table_decode_debug(torch.from_numpy(mem[g0:g0 + group].copy()), IDS, max_new)
            torch.cuda.synchronize()
            ids.append(out["ids"].cpu().numpy())
            lg.append(out["logits"].permute(1, 0, 2).clone())                 # [B][steps][960]
            hid.append(out["hidden"].permute(2, 0, 1, 3).clone())             # [B][steps][4][768]
        ids = np.concatenate(ids)
        _BATCH[key] = (ids, lens_of(ids), torch.cat(lg), torch.cat(hid))
    return _BATCH[key]


def assert_spread(lens, slots, max_new=NEW_MIX):
    """the conditions under which the length-dependent assertions mean something"""
    lens = np.asarray(lens)
    assert len(set(lens.tolist())) >= 4 and lens.min() <= 4 and lens.max() == max_new + 1, lens
    if slots >= 2:
        assert len(SR.simulate(lens, slots)) < SR.chunk_steps(lens, slots), lens


def check_equals_batch(run, yard, max_new, trace=True):
    """ids and lens equal for every table with `pad` behind every EOS; with traces the logits and the four hidden rows of EVERY live
    (table, position) bit-equal to the batch path's, positions no table reached unwritten"""
    bids, blens, blg, bhid = yard
    ids, lens = run["ids"], run["lens"]
    N = bids.shape[0]
    assert ids.shape == (N, max_new + 1) and lens.shape == (N,)
    assert lens.tolist() == blens.tolist(), (lens, blens)
    unequal = []
    for i in range(N):
        L = int(lens[i])
        assert ids[i, 0] == IDS.prefix and (ids[i, :L] == bids[i, :L]).all(), (i, ids[i], bids[i])
        assert (ids[i, L:] == IDS.pad).all() and (bids[i, L:] == IDS.pad).all(), (i, ids[i])
        assert L == max_new + 1 or ids[i, L - 1] == IDS.eos
        if trace:
            if not same_bits(run["logits"][i, :L - 1], blg[i, :L - 1]):
                unequal.append((i, "logits"))
            if not same_bits(run["hidden"][i, :L - 1], bhid[i, :L - 1]):
                unequal.append((i, "hidden"))
            assert bool((run["logits"][i, L - 1:] == SENTINEL).all()) and bool((run["hidden"][i, L - 1:] == SENTINEL).all()), i
    assert unequal == [], f"traces differ in bits from the batch path: {unequal}"


def mixed_run(golden_dir, slots):
    """the traced mixed-length run at `slots`, shared; at 8 slots it is a replayed graph"""
    if slots not in _RUNS:
        _RUNS[slots] = stream_run(decoder(golden_dir, "eos_b3_s6"), mixed_memories(), NEW_MIX, slots, trace=True, side_stream=slots == 8)
    return _RUNS[slots]


# ---------------------------------------------------------------------------------------------------------------- 1: the batch path, exactly
@pytest.mark.parametrize("slots", [1, 3, 8])
def test_stream_equals_the_batch_path(golden_dir, slots):
    yard = batch_groups(golden_dir, "eos_b3_s6", mixed_memories(), NEW_MIX, slots, "mixed")
    print(f"\n[table stream, {slots} slots] batch-path lengths: {yard[1].tolist()}")
    assert_spread(yard[1], slots)
    run = mixed_run(golden_dir, slots)
    check_equals_batch(run, yard, NEW_MIX)
    for side in (False, True):           # the product entry, launched directly and as a replayed graph: the same bytes without traces
        plain = stream_run(decoder(golden_dir, "eos_b3_s6"), mixed_memories(), NEW_MIX, slots, side_stream=side)
        assert plain["ids"].tobytes() == run["ids"].tobytes() and plain["lens"].tobytes() == run["lens"].tobytes() and plain["stats"] == run["stats"]


# ---------------------------------------------------------------------------------------------------------------- 2: the reference fixture
@pytest.mark.parametrize("slots", [1, 2, 3])
def test_stream_gives_the_reference_ids_lengths_and_padding(golden_dir, slots):
    """eos_b3_s6: three tables of three distinct lengths; with one slot a shorter table decodes behind a longer one in the same cache rows"""
    mem, g = R.dec_fixture(golden_dir, "eos_b3_s6")
    run = stream_run(decoder(golden_dir, "eos_b3_s6"), mem, 100, slots)
    refs = [[int(v) for v in g["ids"][b] if v >= 0] for b in range(3)]
    assert len({len(r) for r in refs}) == 3
    assert any(len(refs[b]) > len(refs[b + 1]) for b in range(2)), "no shorter table behind a longer one: the stale-cache case is not covered"
    for b, ref in enumerate(refs):
        n = int(run["lens"][b])
        assert n == len(ref) and run["ids"][b, :n].tolist() == ref and ref[-1] == IDS.eos
        assert bool((run["ids"][b, n:] == IDS.pad).all())
    assert run["stats"]["admitted"] == 3 and run["stats"]["live_slot_steps"] == sum(len(r) - 1 for r in refs)


# ---------------------------------------------------------------------------------------------------------------- 3: the bbox counter
def test_bbox_counter_starts_at_zero_for_an_admitted_table(golden_dir):
    """bbox variant: every table runs to the cap of 7 tokens, so the counter stands at 2 when a table ends; the next table in the slot must
    count from 0 (a counter carried over would move its `]</td>` from column 5 to column 3)"""
    mem = mixed_memories(3)
    alone = batch_groups(golden_dir, "bbox_s6", mem, 7, 1, "bbox3")
    assert alone[1].tolist() == [8, 8, 8], alone[1]
    for row in alone[0]:
        assert [int(t == IDS.bbox_close) for t in row[1:]] == [0, 0, 0, 0, 1, 0, 0], row
        assert all(IDS.bbox_first <= t <= IDS.bbox_last for k, t in enumerate(row[1:]) if k != 4), row
    run = stream_run(decoder(golden_dir, "bbox_s6"), mem, 7, 1, trace=True)
    check_equals_batch(run, alone, 7)


# ---------------------------------------------------------------------------------------------------------------- 4: schedule and counters
@pytest.mark.parametrize("slots", [3, 8])
def test_schedule_and_counters_are_the_simulated_ones(golden_dir, slots):
    run = mixed_run(golden_dir, slots)
    lens, stats = run["lens"], run["stats"]
    assert_spread(lens, slots)
    want = SR.simulate(lens, slots)
    sched, steps = run["sched"], stats["steps"]
    print(f"\n[table stream, {slots} slots] {steps} step launches, {len(want)} scheduled; chunks of {slots} take {SR.chunk_steps(lens, slots)}")
    assert len(want) <= steps <= len(want) + 7
    assert (sched[: len(want)] == want).all()
    assert (sched[len(want): steps, :, 0] == -1).all() and (sched[len(want): steps, :, 1] == 0).all()      # the host's run-ahead: every slot idle
    assert (sched[steps:] == -9).all()
    assert stats["slots"] == slots and stats["admitted"] == N_MIX and stats["live_slot_steps"] == int((lens - 1).sum())


# ---------------------------------------------------------------------------------------------------------------- 5: edges
@pytest.mark.parametrize("N,slots,max_new", [(3, 8, 40), (8, 8, 40), (9, 8, 40), (5, 2, 1), (5, 2, 2), (5, 2, 3)])
def test_edges(golden_dir, N, slots, max_new):
    """Idle slots from the start; exactly full; one waiting; fewer steps than the host looks at the state for.  Every table equals that
    table alone (rd_table_decode at B = 1)."""
    eng = decoder(golden_dir, "eos_b3_s6")
    mem = mixed_memories(N)
    if max_new == NEW_MIX:
        alone = batch_groups(golden_dir, "eos_b3_s6", mixed_memories(), NEW_MIX, 1, "mixed")        # shared with the one-slot case above
    else:
        alone = batch_groups(golden_dir, "eos_b3_s6", mem, max_new, 1, "edges")
    alone = tuple(a[:N] for a in alone)
    run = stream_run(eng, mem, max_new, slots, trace=True)
    check_equals_batch(run, alone, max_new)
    want = SR.simulate(run["lens"], slots)
    assert (run["sched"][: len(want)] == want).all()
    assert len(want) <= run["stats"]["steps"] <= len(want) + 7
    assert run["stats"]["live_slot_steps"] == int((run["lens"] - 1).sum()) and run["stats"]["admitted"] == N
    again = stream_run(eng, mem, max_new, slots)
    assert again["ids"].tobytes() == run["ids"].tobytes() and again["lens"].tobytes() == run["lens"].tobytes() and again["stats"] == run["stats"]


# ---------------------------------------------------------------------------------------------------------------- 6: refusals
def test_refusals_name_the_limit_and_leave_the_outputs_alone(golden_dir):
    from rapiddoc_amd.engine import TABLE_STREAM_MAX_TOKENS, EngineError
    eng = decoder(golden_dir, "eos_b3_s6")
    mem = mixed_memories(3)
    assert "RD_TABLE_STREAM_MAX_SLOTS" in stream_run(eng, mem, 8, 0, expect_rc=1)["msg"]
    assert "RD_TABLE_STREAM_MAX_SLOTS" in stream_run(eng, mem, 8, 9, expect_rc=1)["msg"]
    assert "N must be at least 1" in stream_run(eng, mem, 8, 4, expect_rc=1, n_claimed=0)["msg"]
    assert "S <= 1024" in stream_run(eng, None, 8, 4, expect_rc=1, mem_dev=torch.zeros((1, 1025, D), device="cuda"))["msg"]
    assert "max_new_tokens <= 1024" in stream_run(eng, mem, 0, 4, expect_rc=1)["msg"]
    assert "max_new_tokens <= 1024" in stream_run(eng, mem, 1025, 4, expect_rc=1)["msg"]
    N = TABLE_STREAM_MAX_TOKENS // 1024 + 1
    big = torch.empty((N, 1024, D), dtype=torch.float32, device="cuda")
    assert "RD_TABLE_STREAM_MAX_TOKENS" in stream_run(eng, None, 8, 4, expect_rc=1, mem_dev=big)["msg"]
    del big
    ok = stream_run(eng, mem, 8, 4)                               # and the handle still works
    assert (ok["ids"][:, 0] == IDS.prefix).all()
    with pytest.raises(EngineError, match="RD_TABLE_STREAM_MAX_SLOTS"):
        eng.table_decode_stream(torch.from_numpy(mem).cuda(), IDS, 8, slots=9)
    with pytest.raises(EngineError, match="N must be at least 1"):
        eng.table_decode_stream(torch.zeros((0, 6, D), device="cuda"), IDS, 8)
    with pytest.raises(EngineError, match="1 .. 8 tables"):       # the batch entry keeps its limit
        eng.table_decode(torch.zeros((9, 6, D)), IDS, 4)
    ids, lens, stats = eng.table_decode_stream(torch.from_numpy(mem), IDS, 8, slots=2)
    assert ids.cpu().numpy().tobytes() == stream_run(eng, mem, 8, 2)["ids"].tobytes() and stats["admitted"] == 3 and lens.dtype == torch.int32


# ---------------------------------------------------------------------------------------------------------------- 7: the class
def _class448_stream(golden_dir):
    """the class of test_gpu_unitable_decoder._class448 (the EOS variant the mint tuned for the 448 x 448 input) with batching="stream" """
    from rapiddoc_amd import weights as W
    exp = json.loads((golden_dir / "summary_unitable.json").read_text())["decoder"]["class448"]
    if "cls448" not in _ENG:
        st = dict(R.dec_state(golden_dir))
        b = st["generator.bias"].copy()
        b[IDS.eos] += np.float32(exp["bias_add"])
        st["generator.bias"] = b
        _ENG["cls448"] = TU.Mi355UniTableStructure(R.state(golden_dir), st, IDS, TU.stand_in_tokens(), max_new_tokens=64, resize="pil", batching="stream",
                                                   slots=3)
    return _ENG["cls448"], W.synth_normal_image(int(exp["x_seed"]), 1, 448, 448), exp


def test_class_stream_returns_the_chunk_contexts_in_order(golden_dir):
    from rapiddoc_amd import weights as W
    cls, x448, exp = _class448_stream(golden_dir)
    x = torch.from_numpy(np.concatenate([W.synth_normal_image(40 + i, 1, 32, 48) for i in range(11)])).cuda()
    got = cls.decode_ids(x)
    assert len(cls.last_stream_stats) == 1 and cls.last_stream_stats[0]["admitted"] == 11 and cls.last_stream_stats[0]["slots"] == 3
    try:
        cls.batching = "chunk"
        want = cls.decode_ids(x)
    finally:
        cls.batching = "stream"
    assert len(got) == 11 and got == want
    assert all(c[0] == IDS.prefix and (c[-1] == IDS.eos or len(c) == 65) for c in got)
    xd = torch.from_numpy(x448).cuda()
    assert cls.decode_ids(xd) == [exp["ids"]]
    struct, boxes = cls.forward_tensor(xd, [tuple(exp["ori_hw"])])
    assert struct == [(exp["wrapped"], 1.0)] and boxes[0].tolist() == exp["boxes"]


# ---------------------------------------------------------------------------------------------------------------- 8: the pooled route
def test_predict_many_equals_the_predict_loop(golden_dir, monkeypatch):
    """Five small tables; the engine runs on every one that has OCR rows, then the ids are replaced by recorded ids whose structure holds
    cells (synthetic weights never decode a `<tr> ... </tr>` pair), as test_gpu_table_path does.  Table 1 has no OCR rows, the matcher
    raises on table 3: both come back None, the others string for string."""
    from rapiddoc_amd import table_match as TM, weights as W
    cls, _x, _exp = _class448_stream(golden_dir)
    inj = json.loads((golden_dir / "table_path_match.json").read_text())["engine_inject"]
    oh, ow = inj["ori_hw"]
    sizes = [(120, 300), (90, 200), (150, 260), (100, 240), (64, 330)]
    items = []
    for k, (h, w) in enumerate(sizes):
        quads, texts, scores = copy.deepcopy(inj["ocr_result"])
        quads = [[[px * w / ow, py * h / oh] for px, py in q] for q in quads]
        texts = [f"{t} #{k}" for t in texts]
        if k == 3:
            texts[0] = "RAISE"
        ocr = [] if k == 1 else [quads, texts, scores]
        items.append((np.ascontiguousarray(W.synth_table_crop(20 + k, h, w)[:, :, ::-1]), ocr, [], [], True, False, True))
    real_match, engine_ids = TM.match_tables, []

    def match_tables(pred_structures, cell_bboxes, dt_boxes, rec_res, **kw):
        if any(t == "RAISE" for res in rec_res for t, _s in res):
            raise RuntimeError("the matcher of table 3")
        return real_match(pred_structures, cell_bboxes, dt_boxes, rec_res, **kw)
    monkeypatch.setattr(TM, "match_tables", match_tables)
    real_decode = cls.decode_ids

    def decode_ids(x):
        engine_ids.append(real_decode(x))
        return [list(inj["ids"]) for _ in range(x.shape[0])]
    monkeypatch.setattr(cls, "decode_ids", decode_ids, raising=False)
    model = TU.Mi355RapidTable(cls)
    want = [model.predict(*copy.deepcopy(it)) for it in items]
    calls_loop = len(engine_ids)
    got = model.predict_many(copy.deepcopy(items))
    assert calls_loop == 4 and len(engine_ids) == 5 and len(engine_ids[4]) == 4, "one structure call over the four tables that have OCR rows"
    print(f"\n[predict_many] the pooled call decodes the per-table calls' ids: {engine_ids[4] == [c[0] for c in engine_ids[:4]]}")
    assert got == want
    assert got[1] is None and got[3] is None and all(isinstance(got[k], str) and f"#{k}" in got[k] for k in (0, 2, 4))
    assert len({got[0], got[2], got[4]}) == 3
