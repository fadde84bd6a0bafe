"""CPU: the references of the UniTable decoder's kernel tests (tests/td_reference.py) against independent statements of the same operations:
the fp64 single-query attention against the masked softmax of `unitable_reference.decoder_forward`, the score spreads the attention cases
are built for, the batch select and state reference against `table_unitable.loop_reference` over the recorded trajectories of the
fixtures, the stream one (with the admission rule) against `stream_reference.simulate`."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stream_reference as SR
import td_reference as R
import unitable_reference as U
from rapiddoc_amd import table_unitable as TU

IDS = TU.STAND_IN_IDS


def test_attention_is_the_last_row_of_the_decoder_forwards_masked_softmax(golden_dir):
    """One block of decoder_forward on n tokens: its self-attention output at row n - 1 is single_query_attention of row n - 1's q over the k,
    v of rows 0 .. n - 1; the cross form is the same over the projected memory.  Checked through the block's hidden row: the reference
    attention put in the masked softmax's place gives the same row."""
    st = U.dec_state(golden_dir)
    w = lambda n: torch.from_numpy(np.asarray(st[n])).double()
    lin = lambda x, p: x @ w(p + ".weight").T + w(p + ".bias")
    rng = np.random.default_rng(2)
    n, S = 9, 5
    toks = [IDS.prefix] + [int(t) for t in rng.choice(U.WHITE, n - 1)]
    mem = rng.standard_normal((S, R.D)).astype(np.float32)
    with torch.no_grad():
        hid, _ = U.decoder_forward(st, mem, toks)
        x = w("token_embed.embedding.weight")[torch.tensor(toks)] + w("pos_embed.embedding.weight")[:n]
        p = "layers.0."
        q, k, v = lin(F.layer_norm(x, (R.D,), w(p + "norm1.weight"), w(p + "norm1.bias"), 1e-5), p + "self_attn.wqkv").split(R.D, dim=-1)
        a = torch.cat([R.single_query_attention(q[t:t + 1], k[None, :t + 1], v[None, :t + 1]) for t in range(n)])      # row t sees rows 0 .. t
        x = x + lin(a, p + "self_attn.wo")
        q = lin(F.layer_norm(x, (R.D,), w(p + "norm2.weight"), w(p + "norm2.bias"), 1e-5), p + "multihead_attn.query")
        m = torch.from_numpy(mem).double()
        k, v = lin(m, p + "multihead_attn.key"), lin(m, p + "multihead_attn.value")
        a = R.single_query_attention(q, k[None].expand(n, S, R.D), v[None].expand(n, S, R.D))
        x = x + lin(a, p + "multihead_attn.out")
        x = x + lin(F.gelu(lin(F.layer_norm(x, (R.D,), w(p + "norm3.weight"), w(p + "norm3.bias"), 1e-5), p + "linear1")), p + "linear2")
    assert float((x - hid[:, 0]).abs().max()) < 1e-11 * max(1.0, float(hid[:, 0].abs().max()))


def test_linear_reference_is_the_decoder_forwards_linear():
    g = torch.Generator().manual_seed(4)
    x, w, b, r = (torch.randn(s, generator=g) for s in ((3, 256), (5, 256), (5,), (3, 5)))
    ref = F.gelu(x.double() @ w.double().T + b.double()) + r.double()
    assert float((R.linear_reference(x, w, b, R.ACT_GELU, r) - ref).abs().max()) < 1e-14
    assert R.linear_reference(x, w, dtype=torch.float32).dtype == torch.float32
    assert float((R.linear_reference(x, w) - x.double() @ w.double().T).abs().max()) < 1e-14


@pytest.mark.parametrize("a2", [0.2, 3, 10])
def test_score_spread_of_the_attention_cases(a2):
    """scores (q / 8) . k of standard deviation a2, measured over 3 x 12 x 257 scores, within 15 %; this step's key is spread like the cache"""
    c = R.attention_case(3, 256, True, a2, 11)
    s = R.scores_of(c["q"], torch.cat([c["kc"], c["kcur"][:, None]], 1))
    assert abs(float(s.std()) / a2 - 1) < 0.15, float(s.std())
    assert abs(float(c["kcur"].std()) / R.qk_sigma(a2) - 1) < 0.15
    c = R.attention_case(3, 256, False, a2, 12)
    assert c["kcur"] is None and abs(float(R.scores_of(c["q"], c["kc"]).std()) / a2 - 1) < 0.15


@pytest.mark.parametrize("self_attn", [True, False])
def test_rising_case_has_its_maximum_at_the_last_key(self_attn):
    T = 300
    c = R.attention_case(2, T, self_attn, None, 3, rising=True)
    k = torch.cat([c["kc"], c["kcur"][:, None]], 1) if self_attn else c["kc"]
    s = R.scores_of(c["q"], k)
    tiles = s[..., :288].reshape(2, R.HEADS, 9, 32).max(-1).values
    assert bool((tiles[..., 1:] > tiles[..., :-1] + 1.0).all())         # climbs (by about `rise` = 3) from one 32 keys to the next
    assert bool((s.argmax(-1) >= k.shape[1] - 8).all())


def test_select_argmax_rule():
    rng = np.random.default_rng(0)
    z = rng.standard_normal((8, R.VOCAB)).astype(np.float32)
    z[0, 700] = 50.0                       # outside the whitelist: never wins
    z[1, 40] = np.nan
    z[2, :] = np.nan
    z[3, U.WHITE] = -np.inf                # -1e9 beats -inf: id 0
    z[4, U.WHITE] = -np.inf
    z[4, 300] = -5.0
    z[5, 20] = np.inf
    z[5, 19] = np.nan
    z[6, 12] = z[6, 13] = 9.0
    z[7, 1] = z[7, 509] = 9.0
    got = R.select_argmax(z)
    ref0 = U.whitelist_argmax(z[:1])[0]
    assert ref0 != 700 and got[0] == ref0 == U.WHITE[np.argmax(z[0, U.WHITE])]
    assert got[1] != 40 and got[1] == U.WHITE[np.nanargmax(z[1, U.WHITE])]
    assert got[2:].tolist() == [0, 0, 300, 20, 12, 1]
    assert bool(((got >= 0) & (got < R.VOCAB)).all())


def _recorded(golden_dir):
    """(logits [steps][960], ids the reference's loop produced) per table of the free-loop fixtures, and a synthetic trajectory rich in
    bbox tokens that ends by EOS"""
    out = []
    for tag in ("bbox_s6", "eos_b3_s6", "free_s6"):
        _, g = U.dec_fixture(golden_dir, tag)
        for b in range(g["ids"].shape[0]):
            out.append((tag, g["logits"][:, b], [int(v) for v in g["ids"][b] if v >= 0]))
    rng = np.random.default_rng(5)
    z = rng.standard_normal((40, R.VOCAB)).astype(np.float32)
    z[:, IDS.bbox_first:IDS.bbox_last + 1] += 1.5
    z[:, 12:20] += 2.5
    z[33, IDS.eos] = 30.0
    out.append(("synthetic", z, None))
    return out


def test_batch_select_reference_follows_the_loop_reference_over_recorded_trajectories(golden_dir):
    for tag, z, ref_ids in _recorded(golden_dir):
        steps = len(z)
        ctx = TU.loop_reference(lambda c: U.whitelist_argmax(z[len(c) - 1][None])[0], IDS, max_steps=steps)
        if ref_ids is not None:
            assert ctx == ref_ids, tag                                   # the fixture's loop is this loop
        ids = np.full(steps + 1, IDS.pad, np.int64)
        ids[0] = IDS.prefix
        fin, box, tok = np.zeros(1, np.int32), np.zeros(1, np.int32), IDS.prefix
        for t in range(steps):
            r = R.select_reference(z[t][None], t, IDS, fin, box, steps + 1)
            fin, box = r["finished"], r["boxcount"]
            ids[t + 1] = r["written"][0]
            if len(ctx) > t + 1:                                         # while the table is live: the loop's token, fed on
                assert r["written"][0] == ctx[t + 1] and r["tok"][0] == ctx[t + 1], (tag, t)
            else:                                                        # behind its EOS: pad written, eos fed, the latch holds
                assert r["written"][0] == IDS.pad and r["tok"][0] == IDS.eos and fin[0] == 1, (tag, t)
        assert ids[:len(ctx)].tolist() == ctx and bool((ids[len(ctx):] == IDS.pad).all()), tag
        if tag == "synthetic":
            assert ctx[-1] == IDS.eos and IDS.bbox_close in ctx and len(ctx) == 35


def test_batch_select_reference_forced_mode_and_the_last_step():
    rng = np.random.default_rng(1)
    z = rng.standard_normal((2, R.VOCAB)).astype(np.float32)
    z[:, IDS.eos] = 40.0
    forced = np.array([[11, 5000, 13], [11, -7, 15]], np.int32)
    r = R.select_reference(z, 0, IDS, [0, 0], [0, 0], 4, forced=forced)
    assert r["written"].tolist() == [IDS.eos] * 2 and r["finished"].tolist() == [0, 0] and r["tok"].tolist() == [959, 0]      # latch off, clamped
    r = R.select_reference(z, 2, IDS, [0, 1], [0, 0], 4, forced=forced)
    assert r["tok"].tolist() == [IDS.eos] * 2 and r["written"].tolist() == [IDS.eos, IDS.pad]                                 # past the list
    r = R.select_reference(z, 1023, IDS, [0, 0], [0, 0], 1025)
    assert r["written"] is not None and not r["embed"]
    assert R.select_reference(z, 5, IDS, [0, 0], [0, 0], 6)["written"] is None


@pytest.mark.parametrize("slots", [1, 2, 3, 8])
def test_stream_select_reference_with_the_admission_rule_gives_the_simulated_schedule(golden_dir, slots):
    """N tables, each with a recorded logits trajectory of its own, through `slots` slots: the select reference per step plus the admission
    rule (finished slots take the waiting tables in slot order) visit exactly the (table, position) pairs `stream_reference.simulate` gives
    for the lengths of `loop_reference`, and write that loop's ids."""
    max_new = 24                                                         # the shortest recorded trajectory (bbox_s6, which never stops)
    traj = [z[:max_new] for _, z, _ in _recorded(golden_dir)]
    traj = traj + [traj[0][::-1], traj[-1][::-1]]                        # (two whose every row is finite)
    N = len(traj)
    ctxs = [TU.loop_reference(lambda c, z=z: U.whitelist_argmax(z[len(c) - 1][None])[0], IDS, max_steps=max_new) for z in traj]
    lens = [len(c) for c in ctxs]
    assert len(set(lens)) >= 3 and max(lens) == max_new + 1
    sched = SR.simulate(lens, slots)
    src = np.array([s if s < N else -1 for s in range(slots)], np.int32)
    pos, box, nxt = np.zeros(slots, np.int32), np.zeros(slots, np.int32), min(N, slots)
    ids = np.full((N, max_new + 1), IDS.pad, np.int64)
    ids[:, 0] = IDS.prefix
    got_lens = {}
    for step in range(len(sched)):
        assert np.array_equal(np.stack([src, pos], 1), sched[step]), step
        z = np.stack([traj[src[s]][pos[s]] if src[s] >= 0 else np.full(R.VOCAB, np.nan, np.float32) for s in range(slots)])
        r = R.stream_select_reference(z, IDS, max_new, src, pos, box)
        for (tab, col), v in r["writes"].items():
            ids[tab, col] = v
        got_lens.update(r["lens"])
        pos, box = r["pos"], r["box"]
        assert all((r["tok"][s] >= 0) == (src[s] >= 0 and not r["done"][s]) for s in range(slots))
        for s in range(slots):                                           # td_stream_admit_kernel's rule
            if src[s] >= 0 and r["done"][s]:
                pos[s], box[s] = 0, 0
                src[s], nxt = (nxt, nxt + 1) if nxt < N else (-1, nxt)
    assert bool((src < 0).all()) and got_lens == dict(enumerate(lens))
    for i, c in enumerate(ctxs):
        assert ids[i, :len(c)].tolist() == c and bool((ids[i, len(c):] == IDS.pad).all())


def test_step_reference_stacks_the_decoder_forward(golden_dir):
    st = U.dec_state(golden_dir)
    rng = np.random.default_rng(7)
    mem = rng.standard_normal((2, 3, R.D)).astype(np.float32)
    toks = R.forced_tokens(3, 2, 4, IDS)
    assert (toks[:, 0] == IDS.prefix).all() and not (toks == IDS.eos).any() and not np.array_equal(toks[0], toks[1])
    hid, lg = R.step_reference(st, mem, toks)
    assert hid.shape == (2, 4, 4, R.D) and lg.shape == (2, 4, R.VOCAB) and lg.dtype == torch.float64
    h1, l1 = U.decoder_forward(st, mem[1], [int(t) for t in toks[1]])
    assert torch.equal(hid[1], h1) and torch.equal(lg[1], l1)
    gap = R.whitelist_gap(lg[0].numpy())
    z = np.sort(lg[0].numpy()[:, U.WHITE], axis=1)
    assert gap.shape == (4,) and np.array_equal(gap, z[:, -1] - z[:, -2]) and (gap >= 0).all()
