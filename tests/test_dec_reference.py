"""CPU: the references of the formula decoder's kernel tests (tests/dec_reference.py) against independent statements of the same operations:
the fp64 single-query attention against torch's scaled_dot_product_attention, the fp64 step reference against
oracle.formula.decoder_logits on a prefix, the score spreads the attention cases are built for, the select reference against np.argmax on
the planted rows."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dec_reference as R
from oracle import nets as O
from rapiddoc_amd import weights as W


def test_single_query_attention_equals_sdpa():
    g = torch.Generator().manual_seed(1)
    B, T = 3, 37
    q = torch.randn((B, R.D), generator=g, dtype=torch.float64)
    k = torch.randn((B, T, R.D), generator=g, dtype=torch.float64)
    v = torch.randn((B, T, R.D), generator=g, dtype=torch.float64)
    ours = R.single_query_attention(q, k, v)
    heads = lambda t: t.reshape(B, -1, R.HEADS, R.HD).transpose(1, 2)
    ref = F.scaled_dot_product_attention(heads(q[:, None]), heads(k), heads(v), scale=1.0).transpose(1, 2).reshape(B, R.D)
    assert float((ours - ref).abs().max()) < 1e-13


def test_fused_reference_is_projection_then_attention():
    c = R.fused_case(2, 9, True, 3, 5)
    out, kn, vn = R.fused_attention_reference(c["x"], c["ln_g"], c["ln_b"], c["w"], c["bias"], c["kc"], c["vc"], True)
    h = F.layer_norm(c["x"].double(), (R.D,), c["ln_g"].double(), c["ln_b"].double(), 1e-5)
    qkv = h @ c["w"].double().T + c["bias"].double()
    assert float((kn - qkv[:, R.D:2 * R.D]).abs().max()) < 1e-13 and float((vn - qkv[:, 2 * R.D:]).abs().max()) < 1e-13
    k = torch.cat([c["kc"].double(), qkv[:, None, R.D:2 * R.D]], 1)
    v = torch.cat([c["vc"].double(), qkv[:, None, 2 * R.D:]], 1)
    assert float((out - R.single_query_attention(qkv[:, :R.D], k, v)).abs().max()) < 1e-13
    c = R.fused_case(2, 9, False, 3, 6)
    out, kn, vn = R.fused_attention_reference(c["x"], c["ln_g"], c["ln_b"], c["w"], c["bias"], c["kc"], c["vc"], False)
    assert kn is None and vn is None and out.shape == (2, R.D)


@pytest.mark.parametrize("a2", [0.2, 3, 10])
def test_score_spread_of_the_attention_cases(a2):
    """The cases are built for scores of standard deviation a2 (q, k per entry as `random_qkv` of test_gpu_attention scales them; the fused
    cases through the rows of W_q / W_k): measured over 3 x 16 x 256 scores, within 15 %."""
    B, T = 3, 256
    c = R.unfused_case(B, T, True, a2, 11)
    s = R.scores_of(c["q"], torch.cat([c["kc"], c["kcur"][:, None]], 1))
    assert abs(float(s.std()) / a2 - 1) < 0.15, float(s.std())
    for self_attn in (True, False):
        c = R.fused_case(B, T, self_attn, a2, 12)
        proj = R.linear_reference(c["x"], c["w"], c["bias"], ln=(c["ln_g"], c["ln_b"]))
        k = torch.cat([c["kc"].double(), proj[:, None, R.D:2 * R.D]], 1) if self_attn else c["kc"]
        s = R.scores_of(proj[:, :R.D], k)
        assert abs(float(s.std()) / a2 - 1) < 0.15, (self_attn, float(s.std()))
        if self_attn:                      # the projected current key is spread like the cached ones
            assert abs(float(proj[:, R.D:2 * R.D].std()) / R.qk_sigma(a2) - 1) < 0.15


@pytest.mark.parametrize("fused", [False, True])
def test_rising_case_has_its_maximum_at_the_last_key(fused):
    T = 300
    if fused:
        c = R.fused_case(2, T, True, None, 3, rising=True)
        proj = R.linear_reference(c["x"], c["w"], c["bias"], ln=(c["ln_g"], c["ln_b"]))
        q, k = proj[:, :R.D], torch.cat([c["kc"].double(), proj[:, None, R.D:2 * R.D]], 1)
    else:
        c = R.unfused_case(2, T, True, None, 3, rising=True)
        q, k = c["q"], torch.cat([c["kc"], c["kcur"][:, None]], 1)
    s = R.scores_of(q, k)                                               # [B][HEADS][T + 1]
    tiles = s[..., :288].reshape(2, R.HEADS, 9, 32).max(-1).values      # the best score of every 32 keys
    assert bool((tiles[..., 1:] > tiles[..., :-1] + 1.0).all())         # climbs (by about `rise` = 3) from one tile to the next
    assert bool((s.argmax(-1) >= T - 8).all())


def test_select_reference_on_planted_rows():
    rng = np.random.default_rng(0)
    for V in (4, 4100, 65540):
        pairs = R.tie_pairs(V)
        assert len(pairs) >= 2 and all(a < b < V for a, b in pairs)
        z = R.plant_ties(rng.standard_normal((2 * len(pairs), V)).astype(np.float32), pairs)
        tok, unf, n = R.select_reference(z, 5, np.ones(len(z), np.int32), len(z))
        assert (tok == np.argmax(z, axis=1)).all()
        for r in range(len(z)):                                         # the planted pair holds the maximum and the lower column is named
            a, b = pairs[r % len(pairs)]
            assert z[r, a] == z[r, b] == z[r].max() and tok[r] == a
    assert len(R.tie_pairs(65540)) == 9
    # NaN is the greatest value, all -inf names column 0, forced EOS, PAD for finished rows, one decrement per fresh EOS
    z = rng.standard_normal((5, 8)).astype(np.float32)
    z[0, 6] = np.nan
    z[1, :] = -np.inf
    z[2, :] = np.nan
    z[3, R.EOS] = 99.0
    z[4, R.EOS] = 99.0
    tok, unf, n = R.select_reference(z, 5, np.array([1, 1, 1, 1, 0], np.int32), 4)
    assert tok.tolist() == [6, 0, 0, R.EOS, R.PAD] and unf.tolist() == [1, 1, 1, 0, 0] and n == 3
    tok, unf, n = R.select_reference(z, R.FORCED_EOS_LEN - 2, np.array([1, 1, 1, 1, 0], np.int32), 4)
    assert tok.tolist() == [R.EOS] * 4 + [R.PAD] and n == 0
    tok, _, _ = R.select_reference(z, R.FORCED_EOS_LEN - 3, np.array([1, 1, 1, 1, 0], np.int32), 4)
    assert tok.tolist() == [6, 0, 0, R.EOS, R.PAD]


def test_step_reference_equals_the_oracle_on_a_prefix(golden_dir):
    """Row t of the teacher-forced fp64 reference == oracle.formula.decoder_logits on the prefix ids[:, :t + 1] (fp32 oracle: to fp32
    round-off), and in fp32 the two are the same computation."""
    from oracle import formula as OF
    st = W.synth_state_dict(W.load_manifest(golden_dir / "manifest_ppformulanet_head_dec_a.json"), 0)
    tst = O.as_torch_state(st)
    rng = np.random.default_rng(3)
    V = st["head.decoder.lm_head.weight"].shape[0]
    B, S, L = 2, 5, 6
    enc = torch.from_numpy((rng.standard_normal((B, S, st["head.enc_to_dec_proj.weight"].shape[1])) * 3.0).astype(np.float32))
    ids = torch.from_numpy(rng.integers(3, V, (B, L + 1)))
    ids[:, 0] = 0
    hid64, lg64 = R.step_reference(st, enc, ids)
    hid32, lg32 = R.step_reference(st, enc, ids, torch.float32)
    assert hid64.shape == (B, L, R.D) and lg64.shape == (B, L, V) and lg64.dtype == torch.float64
    with torch.no_grad():
        enc_proj = OF._lin(tst, "head.enc_to_dec_proj", enc)
        for t in (0, 3, L - 1):
            ref = OF.decoder_logits(tst, enc_proj, ids[:, :t + 1])
            scale = float(ref.abs().max())
            assert float((lg64[:, t] - ref.double()).abs().max()) < 1e-4 * max(scale, 1.0)
            assert float((lg32[:, t] - ref).abs().max()) < 1e-4 * max(scale, 1.0)
        full = OF.teacher_forced_logits(tst, enc, ids)
    assert float((lg32 - full).abs().max()) < 1e-4 * max(float(full.abs().max()), 1.0)
