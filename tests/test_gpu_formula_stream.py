"""GPU: the formula decode through refilled slots (rd_formula_decode_stream, csrc/formula_decoder.hip) against the batch path, fp64 and the
host restatement of its schedule.

Weights: `formula_long_case` with the EOS row of the lm head times a further 3.0, so that the sequences of the `encoder_states` pool end at
very different lengths (the fp32 oracle, S = 144, 24 sequences, 40 new tokens: 6 33 40 1 2 16 4 1 4 11 40 1 1 3 3 16 15 36 9 9 2 1 3 23).
Every length a test relies on is read off the GPU's own ids, and every test that needs the spread asserts it first."""
import ctypes as C

import numpy as np
import pytest
import torch

import dec_reference as R
import stream_reference as SR

pytestmark = pytest.mark.gpu

V = 50000
ID_GUARD, LEN_GUARD = -5, -7
RUNS = {}


@pytest.fixture(scope="module")
def decoder(golden_dir):
    from rapiddoc_amd.engine import RdEngine
    from test_oracle_golden import formula_long_case
    st, _enc, _g = formula_long_case(golden_dir)
    st["head.decoder.lm_head.weight"][2] *= np.float32(3.0)
    return RdEngine("ppformulanet_head").load_weights(st), st


def pool(N, S):
    from test_gpu_dec_step import encoder_states
    return encoder_states(N, S)


def stream_run(eng, enc, max_new, slots, trace=False, expect_rc=0, n_claimed=None, enc_dev=None):
    """One call with guard rows around both outputs.  Without `trace` it is the product entry, with it the developer entry and all three
    traces.  Returns a dict; on a refusal (`expect_rc` != 0) the outputs are checked to be untouched and the message is returned."""
    e = torch.from_numpy(enc).cuda() if enc_dev is None else enc_dev
    N = e.shape[0] if n_claimed is None else n_claimed
    S = e.shape[1]
    rows = max(N, 1)
    ids = torch.full((rows + 2, max_new + 1), ID_GUARD, dtype=torch.int64, device="cuda")
    lens = torch.full((rows + 2,), LEN_GUARD, dtype=torch.int32, device="cuda")
    from rapiddoc_amd.engine import FormulaStreamStats
    st = FormulaStreamStats()
    lib, stream = R.lib(), torch.cuda.current_stream().cuda_stream
    lg = hid = sched = None
    if trace:
        sched_steps = N * max_new + 8
        lg = torch.full((N, max_new, V), R.SENTINEL, device="cuda")
        hid = torch.full((N, max_new, R.D), R.SENTINEL, device="cuda")
        sched = torch.full((sched_steps, slots, 2), -9, dtype=torch.int32, device="cuda")
        rc = lib.rd_debug_formula_decode_stream(eng._h, e.data_ptr(), N, S, max_new, slots, ids[1:].data_ptr(), lens[1:].data_ptr(), C.byref(st),
                                                stream, lg.data_ptr(), hid.data_ptr(), sched.data_ptr(), sched_steps)
    else:
        rc = lib.rd_formula_decode_stream(eng._h, e.data_ptr(), N, S, max_new, slots, ids[1:].data_ptr(), lens[1:].data_ptr(), C.byref(st), stream)
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


def shared_run(decoder, slots):
    """the traced N = 24, S = 144, 40-token run at `slots`; the one at 8 slots is shared by four tests"""
    key = (24, 144, 40, slots)
    if key in RUNS:
        return RUNS[key]
    run = stream_run(decoder[0], pool(24, 144), 40, slots, trace=True)
    if slots == 8:
        RUNS[key] = run
    return run


def batch_decode(eng, enc, max_new, trace):
    """rd_debug_formula_decode on one batch: (ids [B][n_cols] numpy, logits [max_new][B][V] on the device or None)"""
    B, S, _ = enc.shape
    e = torch.from_numpy(np.ascontiguousarray(enc)).cuda()
    ids = torch.full((B, max_new + 1), ID_GUARD, dtype=torch.int64, device="cuda")
    lg = torch.full((max_new, B, V), R.SENTINEL, device="cuda") if trace else None
    n = C.c_int32(0)
    rc = R.lib().rd_debug_formula_decode(eng._h, e.data_ptr(), B, S, max_new, ids.data_ptr(), C.byref(n), torch.cuda.current_stream().cuda_stream,
                                         R.ptr(lg), None)
    assert rc == 0, eng._l.rd_last_error(eng._h).decode()
    torch.cuda.synchronize()
    return ids[:, :n.value].cpu().numpy(), lg


def assert_spread(lens, max_new):
    """the conditions under which the length-dependent assertions mean something"""
    tokens = np.asarray(lens) - 1
    assert len(set(tokens.tolist())) >= 6 and tokens.min() <= 2 and tokens.max() == max_new, tokens


def slot_of(lens, slots):
    """formula -> the slot it decodes in (a pure function of the lengths: stream_reference.simulate)"""
    sched = SR.simulate(lens, slots)
    return {int(f): s for t in range(len(sched)) for s in range(slots) for f in [sched[t, s, 0]] if f >= 0}


def check_equals_batch(decoder, enc, max_new, slots, run, trace):
    """Row i of the stream = row i of rd_formula_decode at B = slots over consecutive groups of `slots` formulas (the last group filled up
    with copies of formula 0), up to lens[i], PAD behind it; lens = first EOS + 1 or max_new + 1; with traces the logits of every live
    (formula, position) are bit-equal.

    Up to 16 slots that holds for every formula.  From 17 slots on rd_formula_decode itself gives one formula different bits in different
    ROWS of a batch (measured: docs/notebook/formula_stream.md s3 - the batch path's own linears at M = 17 .. 32, nothing the stream adds), so
    there bit equality is asked of the formulas whose slot is their row of the comparison batch, and the others take the bound of
    test_gpu_dec_step.test_image_in_a_batch_of_16_equals_the_image_alone - 4 x the fp32 yardstick's error against fp64 + 2^-22 max|ref| - on
    the common prefix of the two id rows, with equal ids there."""
    eng, st = decoder
    N = enc.shape[0]
    ids, lens = run["ids"], run["lens"]
    assert ids.shape == (N, max_new + 1) and lens.shape == (N,)
    assert (ids[:, 0] == 0).all() and ((ids >= 0) & (ids < V)).all()
    for i in range(N):
        L = int(lens[i])
        eos = np.nonzero(ids[i, 1:] == R.EOS)[0]
        assert L == (int(eos[0]) + 2 if len(eos) else max_new + 1) and (ids[i, L:] == R.PAD).all(), (i, L, ids[i])
    slot = slot_of(lens, slots)
    unequal, bounded = [], []
    for g0 in range(0, N, slots):
        rows = list(range(g0, min(N, g0 + slots)))
        rows += [0] * (slots - len(rows))
        bids, blg = batch_decode(eng, enc[rows], max_new, trace)
        blens = SR.lens_of(bids, max_new)
        for r, i in enumerate(rows[: min(N, g0 + slots) - g0]):
            L = int(blens[r])
            if slots <= 16 or slot[i] == r:
                assert int(lens[i]) == L, (i, int(lens[i]), L)
                assert (ids[i, :L] == bids[r, :L]).all(), (i, ids[i, :L], bids[r, :L])
                if trace and not R.same_bits(run["logits"][i, :L - 1], blg[:L - 1, r]):
                    unequal.append(i)
                continue
            n = min(L, int(lens[i]))
            diff = np.nonzero(ids[i, :n] != bids[r, :n])[0]
            steps = int(diff[0]) if len(diff) else n - 1                # steps whose input prefix is the same
            assert steps >= 1
            if not len(diff):
                assert int(lens[i]) == L
            if trace:
                with torch.no_grad():
                    _h64, lg64 = R.step_reference(st, enc[i: i + 1], ids[i: i + 1, :steps + 1])
                    _h32, lg32 = R.step_reference(st, enc[i: i + 1], ids[i: i + 1, :steps + 1], torch.float32)
                bound = 4.0 * float((lg32.double() - lg64).abs().max()) + 2.0 ** -22 * float(lg64.abs().max())
                d = float((run["logits"][i, :steps].double() - blg[:steps, r].double()).abs().max())
                bounded.append((i, slot[i], r, steps, d, bound))
                assert d <= bound, (i, d, bound)
        del blg
    for i, s, r, steps, d, bound in bounded:
        print(f"{slots} slots: formula {i} in slot {s}, row {r} of the batch: {steps} steps, max logit difference {d:.3e} (bound {bound:.3e})")
    assert unequal == [], f"logits differ in bits from the batch path for formulas {unequal}"
    if trace:      # positions no formula reached stay unwritten
        for i in range(N):
            assert bool((run["logits"][i, int(lens[i]) - 1:] == R.SENTINEL).all()) and bool((run["hidden"][i, int(lens[i]) - 1:] == R.SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------- 1: the batch path, exactly
@pytest.mark.parametrize("slots", [1, 8, 9, 17])
def test_stream_equals_the_batch_path(decoder, slots):
    """One slot (a 1-token formula decodes behind a 40-token one in the same cache: stale rows), then one count per dec_gemv band."""
    run = shared_run(decoder, slots)
    assert_spread(run["lens"], 40)
    if slots == 1:
        tokens = run["lens"] - 1
        assert any(tokens[i] == 40 and tokens[i + 1] <= 2 for i in range(23)), tokens
    check_equals_batch(decoder, pool(24, 144), 40, slots, run, trace=True)
    # the product entry: the same bytes without traces
    plain = stream_run(decoder[0], pool(24, 144), 40, slots)
    assert plain["ids"].tobytes() == run["ids"].tobytes() and plain["lens"].tobytes() == run["lens"].tobytes() and plain["stats"] == run["stats"]


# ---------------------------------------------------------------------------------------------------------------- 2: fp64
def test_stream_against_fp64(decoder):
    """The stream's own ids fed to the teacher-forced fp64 reference: hidden rows and logits of every live (formula, position) within
    4 x err(fp32 yardstick) + 2^-22 max|ref|, the chosen token at most twice that below the fp64 maximum (test_gpu_dec_step.check_case)."""
    eng, st = decoder
    run = shared_run(decoder, 8)
    ids, lens = run["ids"], run["lens"]
    assert_spread(lens, 40)
    live = torch.from_numpy(np.arange(40)[None, :] < (lens[:, None] - 1))
    with torch.no_grad():
        hid64, lg64 = R.step_reference(st, pool(24, 144), ids)
        hid32, lg32 = R.step_reference(st, pool(24, 144), ids, torch.float32)
    tag = f"stream 8 slots, {int(live.sum())} live rows"
    R.bound_ratio(run["hidden"].cpu()[live], hid64[live], hid32[live], tag + " hidden")
    yerr = float((lg32[live].double() - lg64[live]).abs().max())
    bound = 4.0 * yerr + 2.0 ** -22 * float(lg64[live].abs().max())
    R.bound_ratio(run["logits"].cpu()[live], lg64[live], lg32[live], tag + " logits")
    chosen = torch.gather(lg64, 2, torch.from_numpy(ids[:, 1:, None]))[..., 0]
    gap = (lg64.max(dim=2).values - chosen)[live]
    print(f"{tag}: chosen token below the fp64 maximum by at most {float(gap.max()):.3e} (2 x bound {2 * bound:.3e})")
    assert float(gap.max()) <= 2 * bound, (float(gap.max()), bound)


# ---------------------------------------------------------------------------------------------------------------- 3: refill works
def test_refill_keeps_the_slots_busy(decoder):
    run = shared_run(decoder, 8)
    lens, stats = run["lens"], run["stats"]
    assert_spread(lens, 40)
    total = int((lens - 1).sum())
    bound = SR.refill_bound(lens, 8, look_ahead=7)
    chunked = SR.chunk_steps(lens, 8)
    print(f"8 slots: {stats['steps']} step launches for {total} tokens (bound {bound}); chunks of 8 would take {chunked} steps")
    assert stats["slots"] == 8 and stats["admitted"] == 24
    assert stats["live_slot_steps"] == total
    assert chunked > bound, "the input does not discriminate"
    assert stats["steps"] <= bound


# ---------------------------------------------------------------------------------------------------------------- 4: the schedule
def test_schedule_is_the_simulated_one(decoder):
    """The lowest finished slot takes the lowest waiting formula at the end of the step in which it finished."""
    run = shared_run(decoder, 8)
    assert_spread(run["lens"], 40)
    want = SR.simulate(run["lens"], 8)
    sched, steps = run["sched"], run["stats"]["steps"]
    assert len(want) <= steps <= len(want) + 7
    assert (sched[: len(want)] == want).all()
    assert (sched[len(want): steps, :, 0] == -1).all() and (sched[len(want): steps, :, 1] == 0).all()      # the host's run-ahead: every slot idle
    assert (sched[steps:] == -9).all()


# ---------------------------------------------------------------------------------------------------------------- 5: edges
@pytest.mark.parametrize("N,slots,max_new", [(3, 8, 40), (8, 8, 40), (9, 8, 40), (24, 16, 40), (5, 2, 1), (5, 2, 2), (5, 2, 3)])
def test_edges(decoder, N, slots, max_new):
    """S = 5.  Idle slots from the start; exactly full; one waiting; several slots refilled in one step and a queue that runs dry while
    slots are live; fewer steps than the batch loop captures a graph for."""
    eng = decoder[0]
    enc = pool(N, 5)
    run = stream_run(eng, enc, max_new, slots, trace=True)
    lens = run["lens"]
    if (N, slots) == (24, 16):
        assert_spread(lens, 40)
        assert int((lens[:16] == 2).sum()) >= 2, lens          # formulas of the first wave that end at their first token: refilled together
        want = SR.simulate(lens, slots)
        assert (want[1, :, 0] >= 16).sum() >= 2
        dry = next(t for t in range(len(want)) if want[t, :, 0].max() == N - 1)
        assert (want[dry + 1:, :, 0] >= 0).any(), "nothing is live after the queue ran dry"
    check_equals_batch(decoder, enc, max_new, slots, run, trace=True)
    want = SR.simulate(lens, slots)
    assert (run["sched"][: len(want)] == want).all()
    assert run["stats"]["live_slot_steps"] == int((lens - 1).sum()) and run["stats"]["admitted"] == N
    again = stream_run(eng, enc, max_new, slots)
    assert again["ids"].tobytes() == run["ids"].tobytes() and again["lens"].tobytes() == run["lens"].tobytes()
    third = stream_run(eng, enc, max_new, slots)
    assert third["ids"].tobytes() == again["ids"].tobytes() and third["lens"].tobytes() == again["lens"].tobytes() and third["stats"] == again["stats"]


# ---------------------------------------------------------------------------------------------------------------- 6: refusals
def test_refusals_leave_the_outputs_alone(decoder):
    from rapiddoc_amd.engine import FORMULA_STREAM_MAX_TOKENS
    eng = decoder[0]
    enc = pool(3, 5)
    assert "slots" in stream_run(eng, enc, 8, 0, expect_rc=1)["msg"]
    assert "slots" in stream_run(eng, enc, 8, 33, expect_rc=1)["msg"]
    assert "at least 1" in stream_run(eng, enc, 8, 4, expect_rc=1, n_claimed=0)["msg"]
    N = FORMULA_STREAM_MAX_TOKENS // 144 + 1
    big = torch.empty((N, 144, 2048), dtype=torch.float32, device="cuda")
    assert "RD_FORMULA_STREAM_MAX_TOKENS" in stream_run(eng, None, 8, 4, expect_rc=1, enc_dev=big)["msg"]
    del big
    ok = stream_run(eng, enc, 8, 4)                               # and the handle still works
    assert (ok["ids"][:, 0] == 0).all()
    from rapiddoc_amd.engine import EngineError
    with pytest.raises(EngineError, match="slots"):
        eng.formula_decode_stream(torch.from_numpy(enc).cuda(), 8, slots=0)


# ---------------------------------------------------------------------------------------------------------------- 7: FormulaRecognizer
def test_recognizer_stream_returns_the_chunk_strings(golden_dir, monkeypatch):
    """Five crops of different sizes and one the pre-process finds empty (a stand-in: the 1 x 1 crop), stream against chunk."""
    from rapiddoc_amd import formula_host as FH, weights as W
    st = W.synth_state_dict(W.load_manifest(golden_dir / "manifest_ppformulanet_plus_m_m8.json"), 0)
    rec = FH.FormulaRecognizer(st, max_new_tokens=6, token_decoder=lambda toks: "<" + " ".join(str(t) for t in toks) + ">", batching="stream", slots=2)
    host_preprocess = FH.preprocess
    monkeypatch.setattr(FH, "preprocess", lambda ims: [None if im.shape[:2] == (1, 1) else host_preprocess([im])[0] for im in ims])
    rng = np.random.default_rng(3)
    sizes = [(60, 200), (90, 90), (40, 300), (1, 1), (120, 70), (33, 57)]
    imgs = []
    for h, w in sizes:
        im = np.full((h, w, 3), 255, np.uint8)
        if h > 1:
            im[h // 4: h - h // 4, w // 6: w - w // 6] = rng.integers(0, 120, (h - h // 4 - h // 4, w - w // 6 - w // 6, 3))
        imgs.append(im)
    got = rec.batch_predict(imgs, batch_size=2)
    assert len(rec.last_stream_stats) == 1 and rec.last_stream_stats[0]["admitted"] == 5 and rec.last_stream_stats[0]["slots"] == 2
    rec.batching = "chunk"
    want = rec.batch_predict(imgs, batch_size=2)
    assert len(got) == 6 and all(isinstance(s, str) for s in got)
    assert got == want
    assert got[3] == "" and rec.last_routes[3] == "empty" and all(got[i].startswith("<") for i in (0, 1, 2, 4, 5))
