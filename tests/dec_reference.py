"""References and input builders shared by the formula decoder's kernel tests (tests/test_gpu_dec_*.py; the helpers
themselves are tested on the CPU in tests/test_dec_reference.py).

Every reference takes a `dtype`: float64 is the reference proper, float32 the YARDSTICK - the same operation in plain torch fp32 on the CPU.
Bound (one for all cases): the kernel's max-abs error against fp64 may be at most 4 x the yardstick's + 2^-22 max|ref|.  The factor is the
convention of tests/test_gpu_attention.py / test_gpu_layernorm.py (it covers `__expf`'s extra rounding of its argument and the kernels'
re-association of sums); nothing in it comes from the code under test.  The measured ratios are in docs/notebook/formula_decode_kernels.md."""
import numpy as np
import torch
import torch.nn.functional as F

SENTINEL = -777.25
D, HEADS, HD, FFN = 512, 16, 32, 2048
EOS, PAD = 2, 1
FORCED_EOS_LEN = 1537
ACT_NONE, ACT_GELU = 0, 2

def lib():
    from rapiddoc_amd import _lib
    return _lib.load()


def ptr(t):
    return t.data_ptr() if t is not None else None


# ------------------------------------------------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------------------------------------------------
def bound_ratio(got, ref64, yard32, tag):
    """Asserts max|got - ref64| <= 4 max|yard32 - ref64| + 2^-22 max|ref64|; prints the figures first; returns error / bound."""
    got, ref64, yard32 = (torch.as_tensor(a) for a in (got, ref64, yard32))
    assert got.shape == ref64.shape == yard32.shape, (tag, got.shape, ref64.shape, yard32.shape)
    assert bool(torch.isfinite(got).all()), tag
    err = float((got.double() - ref64).abs().max())
    yerr = float((yard32.double() - ref64).abs().max())
    bound = 4.0 * yerr + 2.0 ** -22 * float(ref64.abs().max())
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{tag}: err {err:.3e} fp32 yardstick {yerr:.3e} bound {bound:.3e} ratio {ratio:.3f}")
    assert err <= bound, (tag, err, yerr, bound)
    return ratio


def same_bits(a, b):
    """Bit equality of two fp32 tensors (NaN payloads included)."""
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


# ------------------------------------------------------------------------------------------------------------------------------------------
# linear (dec_gemv_kernel): y = act(LN?(x) w^T + bias) + res
# ------------------------------------------------------------------------------------------------------------------------------------------
def linear_reference(x, w, bias=None, ln=None, act=ACT_NONE, res=None, dtype=torch.float64):
    c = lambda t: None if t is None else t.to(dtype)
    h = c(x)
    if ln is not None:
        h = F.layer_norm(h, (h.shape[-1],), c(ln[0]), c(ln[1]), 1e-5)
    y = F.linear(h, c(w), c(bias))
    if act == ACT_GELU:
        y = F.gelu(y)
    return y if res is None else y + c(res)


# ------------------------------------------------------------------------------------------------------------------------------------------
# single-query attention (dec_attention_kernel / dec_attn_fused*_kernel)
# ------------------------------------------------------------------------------------------------------------------------------------------
def single_query_attention(q, k, v, dtype=torch.float64):
    """softmax(q k^T) v per (sequence, head): q [B][HEADS HD] (already scaled), k / v [B][T][HEADS HD] -> [B][HEADS HD]."""
    B, T = k.shape[0], k.shape[1]
    qh = q.to(dtype).reshape(B, HEADS, 1, HD)
    kh = k.to(dtype).reshape(B, T, HEADS, HD).permute(0, 2, 1, 3)
    vh = v.to(dtype).reshape(B, T, HEADS, HD).permute(0, 2, 1, 3)
    p = torch.softmax(qh @ kh.transpose(-1, -2), dim=-1)
    return (p @ vh).reshape(B, HEADS * HD)


def fused_attention_reference(x, ln_g, ln_b, w, bias, kc, vc, self_attn, dtype=torch.float64):
    """The fused launch: h = LN(x); SELF: q | k | v = h w^T + bias (w [3 D][D]), the new k, v join the cached kc / vc [B][T][D] as the last
    key; cross: q = h w^T + bias (w [D][D]) over the cached keys alone.  Returns (out [B][D], new k or None, new v or None)."""
    proj = linear_reference(x, w, bias, ln=(ln_g, ln_b), dtype=dtype)
    if not self_attn:
        return single_query_attention(proj, kc.to(dtype), vc.to(dtype), dtype), None, None
    q, kn, vn = proj[:, :D], proj[:, D:2 * D], proj[:, 2 * D:]
    k = torch.cat([kc.to(dtype), kn[:, None]], 1)
    v = torch.cat([vc.to(dtype), vn[:, None]], 1)
    return single_query_attention(q, k, v, dtype), kn, vn


def scores_of(q, k):
    """fp64 scores [B][HEADS][T] of a single query (for the spread checks)."""
    B, T = k.shape[0], k.shape[1]
    return (q.double().reshape(B, HEADS, 1, HD) @ k.double().reshape(B, T, HEADS, HD).permute(0, 2, 3, 1))[:, :, 0]


def qk_sigma(a2):
    """Per-entry deviation of q and k at which the (pre-scaled) scores q . k over HD dims have standard deviation a2 - what `random_qkv` of
    tests/test_gpu_attention.py does with scale = hd^-1/2."""
    return float(a2) ** 0.5 / HD ** 0.25


def unfused_case(B, T, self_attn, a2, seed, rising=False, rise=3.0):
    """Operands of dec_attention_kernel.  T = cached keys.  Returns dict(q [B][D], kc, vc [B][T][D], kcur, vcur [B][D] or None)."""
    g = torch.Generator().manual_seed(seed)
    s = qk_sigma(a2 if not rising else 1.0)
    q = torch.randn((B, D), generator=g) * s
    kc = torch.randn((B, T, D), generator=g) * s
    vc = torch.randn((B, T, D), generator=g)
    kcur = torch.randn((B, D), generator=g) * s if self_attn else None
    vcur = torch.randn((B, D), generator=g) if self_attn else None
    if rising:
        u, gain = _rising_dirs(g, T + 1, rise)
        q = 0.1 * q + gain * u.reshape(1, D)
        ramp = (torch.arange(T + 1) + 1.0) / (T + 1)
        kc = 0.1 * kc + ramp[None, :T, None] * gain * u.reshape(1, 1, D)
        if self_attn:
            kcur = 0.1 * kcur + gain * u.reshape(1, D)
    return dict(q=q, kc=kc, vc=vc, kcur=kcur, vcur=vcur)


def _rising_dirs(g, keys, rise):
    """A unit direction per head and the gain at which the best score climbs by `rise` per 32 keys (as `rising_qkv` of test_gpu_attention)."""
    u = torch.randn((HEADS, HD), generator=g)
    u = u / u.norm(dim=1, keepdim=True)
    return u, (rise * max(keys, 32) / 32.0) ** 0.5


def fused_case(B, T, self_attn, a2, seed, rising=False, rise=3.0):
    """Operands of the fused launches.  The rows of W_q (and W_k) are scaled so that the projected q (k) entries have deviation qk_sigma(a2),
    like the cached keys: the scores have deviation a2.  Rising: the q bias carries gain u, the cached keys ramp along u."""
    g = torch.Generator().manual_seed(seed)
    s = qk_sigma(a2 if not rising else 1.0)
    x = torch.randn((B, D), generator=g) * 2.0 + 0.5
    ln_g = 1.0 + 0.1 * torch.randn(D, generator=g)
    ln_b = 0.1 * torch.randn(D, generator=g)
    rows = 3 * D if self_attn else D
    w = torch.randn((rows, D), generator=g) / D ** 0.5           # LN(x) has unit entries: projections of unit deviation
    bias = 0.1 * torch.randn(rows, generator=g)
    w[:D] *= s
    bias[:D] *= s
    if self_attn:
        w[D:2 * D] *= s
        bias[D:2 * D] *= s
    kc = torch.randn((B, T, D), generator=g) * s
    vc = torch.randn((B, T, D), generator=g)
    if rising:
        u, gain = _rising_dirs(g, T + 1, rise)
        w[:D] *= 0.1
        bias[:D] = gain * u.reshape(D)
        ramp = (torch.arange(T + 1) + 1.0) / (T + 1)
        kc = 0.1 * kc + ramp[None, :T, None] * gain * u.reshape(1, 1, D)
        if self_attn:
            w[D:2 * D] *= 0.1
            bias[D:2 * D] = gain * u.reshape(D)
    return dict(x=x, ln_g=ln_g, ln_b=ln_b, w=w.contiguous(), bias=bias, kc=kc, vc=vc)


# ------------------------------------------------------------------------------------------------------------------------------------------
# select (dec_select_kernel) and the next step's embedding
# ------------------------------------------------------------------------------------------------------------------------------------------
def select_reference(logits, step, unfinished, n_unfinished):
    """What one select launch at `step` leaves: (token [B] int64, unfinished [B], n_unfinished).  argmax as numpy / torch define it (a NaN
    is the greatest value, the lowest index among equals wins), EOS forced at the length limit, PAD for finished sequences."""
    z = np.asarray(logits)
    tok = np.argmax(z, axis=1).astype(np.int64)
    if step + 1 == FORCED_EOS_LEN - 1:
        tok[:] = EOS
    unf = np.asarray(unfinished).copy()
    tok = np.where(unf != 0, tok, PAD)
    ended = (unf != 0) & (tok == EOS)
    unf[ended] = 0
    return tok, unf, int(n_unfinished) - int(ended.sum())


def tie_pairs(V):
    """Column pairs (lo, hi) for planted ties, those that exist at this V: inside a quad, across quads, across the 16-byte path's first
    wrap (4095, 4096), the same thread's next load (c, c + 4096), the ends, and between wavefront 15 and wavefront 0 in both orders, for
    the 16-byte path (thread = (c / 4) % 1024) and the scalar one (thread = c % 1024)."""
    cand = [(1, 2), (3, 4), (4095, 4096), (37, 37 + 4096), (0, V - 1), (4 * 1000, 4 * 1024 + 4), (8, 4 * 1000), (970, 1030), (5, 1000)]
    return [(a, b) for a, b in cand if 0 <= a < b < V]


def plant_ties(logits, pairs):
    """Row r of a copy of `logits` gets the pair r % len(pairs) raised to the same value above the row's maximum."""
    z = np.array(logits, copy=True)
    for r in range(z.shape[0]):
        a, b = pairs[r % len(pairs)]
        z[r, a] = z[r, b] = np.float32(z[r].max() + 1.0)
    return z


def embed_reference(emb, pos, g, b, tok, position, dtype=torch.float64):
    """LN(emb[tok] + pos[position]) - emb already carries sqrt(d_model), as the library stores it."""
    v = emb.to(dtype)[torch.as_tensor(tok)] + pos.to(dtype)[position]
    return F.layer_norm(v, (v.shape[-1],), g.to(dtype), b.to(dtype), 1e-5)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the whole step
# ------------------------------------------------------------------------------------------------------------------------------------------
def step_reference(state, enc, ids, dtype=torch.float64):
    """Teacher-forced decoder fed `ids` [B][L] (start token included): (hidden [B][L-1][512] in front of the final LayerNorm, logits
    [B][L-1][V]); row t is what step t of the decode loop computes.  oracle.formula.decoder_logits' layer stack in `dtype`."""
    from oracle import formula as OF
    st = {k: torch.as_tensor(v).to(dtype) for k, v in state.items() if k.startswith("head.")}
    enc_proj = OF._lin(st, "head.enc_to_dec_proj", torch.as_tensor(enc).to(dtype))
    idp = torch.as_tensor(ids)[:, :-1]
    L = idp.shape[1]
    DEC = OF.DEC
    x = st[DEC + "embed_tokens.weight"][idp] * (D ** 0.5) + st[DEC + "embed_positions.weight"][torch.arange(L) + 2]
    x = OF._ln(st, DEC + "layernorm_embedding", x)
    l = 0
    while f"{DEC}layers.{l}.fc1.weight" in st:
        p = f"{DEC}layers.{l}"
        h = OF._ln(st, p + ".self_attn_layer_norm", x)
        x = x + OF._attn(st, p + ".self_attn", h, h, True)
        h = OF._ln(st, p + ".encoder_attn_layer_norm", x)
        x = x + OF._attn(st, p + ".encoder_attn", h, enc_proj, False)
        h = OF._ln(st, p + ".final_layer_norm", x)
        x = x + OF._lin(st, p + ".fc2", F.gelu(OF._lin(st, p + ".fc1", h)))
        l += 1
    logits = F.linear(OF._ln(st, DEC + "layer_norm", x), st["head.decoder.lm_head.weight"])
    return x, logits
