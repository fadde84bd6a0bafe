"""References and input builders shared by the UniTable decoder's kernel tests (tests/test_gpu_td_*.py; the helpers themselves are tested on
the CPU in tests/test_td_reference.py).  The pattern, the helpers and the bound are the formula decoder's (tests/dec_reference.py).

Every reference takes a `dtype`: float64 is the reference proper, float32 the YARDSTICK - the same operation in plain torch fp32 on the CPU.
Bound (one for all cases): the kernel's max-abs error against fp64 may be at most 4 x the yardstick's + 2^-22 max|ref| (`bound_ratio`).
Nothing in it comes from the code under test.  The measured ratios are in docs/notebook/table_decode_kernels.md."""
import numpy as np
import torch
import torch.nn.functional as F

import unitable_reference as U
from dec_reference import SENTINEL, bound_ratio, lib, ptr, same_bits      # noqa: F401  (the tests take them from here)

D, HEADS, HD, FFN, VOCAB, MAXPOS, MAXB = 768, 12, 64, 3072, 960, 1024, 8
ACT_NONE, ACT_GELU = 0, 2
Q_SCALE = 0.125


# ------------------------------------------------------------------------------------------------------------------------------------------
# linear (td_gemv_kernel): y = act(x w^T + bias) + res
# ------------------------------------------------------------------------------------------------------------------------------------------
def linear_reference(x, w, bias=None, act=ACT_NONE, res=None, dtype=torch.float64):
    c = lambda t: None if t is None else t.to(dtype)
    y = F.linear(c(x), c(w), c(bias))
    if act == ACT_GELU:
        y = F.gelu(y)
    return y if res is None else y + c(res)


# ------------------------------------------------------------------------------------------------------------------------------------------
# single-query attention (td_attn_kernel / td_stream_attn_kernel)
# ------------------------------------------------------------------------------------------------------------------------------------------
def single_query_attention(q, k, v, dtype=torch.float64):
    """softmax((q / 8) k^T) v per (table, head): q [B][768] (NOT yet scaled), k / v [B][T][768] -> [B][768]."""
    B, T = k.shape[0], k.shape[1]
    qh = (q.to(dtype) * Q_SCALE).reshape(B, HEADS, 1, HD)
    kh = k.to(dtype).reshape(B, T, HEADS, HD).permute(0, 2, 1, 3)
    vh = v.to(dtype).reshape(B, T, HEADS, HD).permute(0, 2, 1, 3)
    p = torch.softmax(qh @ kh.transpose(-1, -2), dim=-1)
    return (p @ vh).reshape(B, HEADS * HD)


def scores_of(q, k):
    """fp64 scores [B][HEADS][T] of a single query, the 1 / 8 included (for the spread checks)."""
    B, T = k.shape[0], k.shape[1]
    return ((q.double() * Q_SCALE).reshape(B, HEADS, 1, HD) @ k.double().reshape(B, T, HEADS, HD).permute(0, 2, 3, 1))[:, :, 0]


def qk_sigma(a2):
    """Per-entry deviation of q / 8 and of k at which the scores (q / 8) . k over 64 dims have standard deviation a2."""
    return float(a2) ** 0.5 / HD ** 0.25


def attention_case(B, T, self_attn, a2, seed, rising=False, rise=3.0):
    """Operands of one attention launch, T = cached keys (the self form has T + 1 keys: this step's row is the last).  Score deviation a2
    (0.2 flat, 3 moderate, 10 few-hot), or `rising`: the best score climbs by `rise` per 32 keys, so the last key leads and the early
    keys' probabilities are tiny (modelled on dec_reference.unfused_case).  Returns dict(q [B][768], kc, vc [B][T][768], kcur, vcur
    [B][768] or None)."""
    g = torch.Generator().manual_seed(seed)
    s = qk_sigma(a2 if not rising else 1.0)
    q = torch.randn((B, D), generator=g) * s
    kc = torch.randn((B, T, D), generator=g) * s
    vc = torch.randn((B, T, D), generator=g)
    kcur = torch.randn((B, D), generator=g) * s if self_attn else None
    vcur = torch.randn((B, D), generator=g) if self_attn else None
    if rising:
        keys = T + (1 if self_attn else 0)
        u = torch.randn((HEADS, HD), generator=g)
        u = u / u.norm(dim=1, keepdim=True)
        gain = (rise * max(keys, 32) / 32.0) ** 0.5
        q = 0.1 * q + gain * u.reshape(1, D)
        ramp = (torch.arange(keys) + 1.0) / keys
        kc = 0.1 * kc + ramp[None, :T, None] * gain * u.reshape(1, 1, D)
        if self_attn:
            kcur = 0.1 * kcur + gain * u.reshape(1, D)
    return dict(q=q / Q_SCALE, kc=kc, vc=vc, kcur=kcur, vcur=vcur)      # the kernel multiplies q by 1 / 8 (exact in fp32)


def attention_reference(case, dtype=torch.float64):
    """[B][768] of a case of `attention_case`: the cached keys, and behind them this step's row in the self form."""
    k, v = case["kc"], case["vc"]
    if case["kcur"] is not None:
        k, v = torch.cat([k, case["kcur"][:, None]], 1), torch.cat([v, case["vcur"][:, None]], 1)
    return single_query_attention(case["q"], k, v, dtype)


# ------------------------------------------------------------------------------------------------------------------------------------------
# select (td_select_kernel / td_stream_select_kernel), the state words and the next step's input row
# ------------------------------------------------------------------------------------------------------------------------------------------
def select_argmax(logits):
    """The kernels' documented rule on [n][960]: a NaN counts as -inf, then `whitelist_argmax` - ids outside {1, 12 .. 509} sit at -1e9, the
    lowest id wins among equals.  (So a row whose whitelisted logits are all NaN or -inf names id 0.)"""
    z = np.array(logits, dtype=np.float64, copy=True)
    z[np.isnan(z)] = -np.inf
    return U.whitelist_argmax(z)


def _bbox_rule(chosen, count, ids):
    """(emitted, new count): only a bbox token raises the counter, the fifth in a row is replaced by `bbox_close` and clears it"""
    if ids.bbox_first <= chosen <= ids.bbox_last:
        count += 1
        if count > 4:
            return ids.bbox_close, 0
    return chosen, count


def select_reference(logits, step, ids, finished, boxcount, ids_ld, forced=None):
    """What one td_select_kernel launch at `step` leaves.  logits [B][960]; finished, boxcount [B]; forced None or int [B][forced_ld] (the
    EOS latch is then off and forced[b][step + 1] is fed, `eos` past the list).  Returns dict(chosen, emitted, written = the value of
    ids[b][step + 1] or None when that column does not exist, finished, boxcount, tok = the token fed to the next step, clamped to the
    vocabulary, embed = whether the next step's input row emb[tok] + pos[step + 1] is written)."""
    chosen = select_argmax(logits)
    B = len(chosen)
    fin, box = np.array(finished, dtype=np.int32, copy=True), np.array(boxcount, dtype=np.int32, copy=True)
    emitted, written, tok = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    for b in range(B):
        e, box[b] = _bbox_rule(int(chosen[b]), int(box[b]), ids)
        was_done = fin[b] != 0
        emitted[b], written[b] = e, (ids.pad if was_done else e)
        if forced is None and not was_done and e == ids.eos:
            fin[b] = 1
        nt = ids.eos if (was_done or e == ids.eos) else e
        if forced is not None:
            f = np.asarray(forced)
            nt = int(f[b, step + 1]) if step + 1 < f.shape[1] else ids.eos
        tok[b] = min(max(nt, 0), VOCAB - 1)
    return dict(chosen=chosen, emitted=emitted, written=written if step + 1 < ids_ld else None, finished=fin, boxcount=box, tok=tok,
                embed=step + 1 < MAXPOS)


def stream_select_reference(logits, ids, max_new, src, pos, box):
    """What one td_stream_select_kernel launch leaves for slots (src, pos, box) [M], logits [M][960].  Returns dict(writes = {(table,
    column): id}, lens = {table: columns}, pos, box, done [M] after the launch (done is only ever SET here), tok [M] = the token whose row
    emb[tok] + pos[new pos] becomes the slot's next input, or -1 where no row is written (idle, or the table ended))."""
    M = len(src)
    chosen = select_argmax(logits)
    pos2, box2 = np.array(pos, dtype=np.int32, copy=True), np.array(box, dtype=np.int32, copy=True)
    done, tok = np.zeros(M, np.int32), np.full(M, -1, np.int64)
    writes, lens = {}, {}
    for s in range(M):
        if src[s] < 0:
            continue
        t = int(pos[s])
        e, box2[s] = _bbox_rule(int(chosen[s]), int(box[s]), ids)
        writes[(int(src[s]), t + 1)] = e
        if e == ids.eos or t + 1 >= max_new:
            lens[int(src[s])] = t + 2
            done[s] = 1
        else:
            pos2[s] = t + 1
            tok[s] = min(max(e, 0), VOCAB - 1)
    return dict(writes=writes, lens=lens, pos=pos2, box=box2, done=done, tok=tok)


def embed_row(emb, pos, tok, position):
    """emb[tok] + pos[position] in torch fp32: one rounding, so the kernels' rows equal it bit for bit"""
    return emb[torch.as_tensor(tok)] + pos[position]


# ------------------------------------------------------------------------------------------------------------------------------------------
# the whole step
# ------------------------------------------------------------------------------------------------------------------------------------------
def step_reference(state, memory, tokens, dtype=torch.float64):
    """Teacher-forced decoder of B tables: memory [B][S][768], tokens [B][n] -> (hidden [B][n][4][768], logits [B][n][960]) by
    unitable_reference.decoder_forward per table."""
    hid, lg = [], []
    with torch.no_grad():
        for b in range(len(tokens)):
            h, l = U.decoder_forward(state, np.ascontiguousarray(memory[b]), [int(t) for t in tokens[b]], dtype)
            hid.append(h)
            lg.append(l)
    return torch.stack(hid), torch.stack(lg)


def forced_tokens(seed, B, n, ids):
    """int32 [B][n]: the prefix, then whitelisted ids other than EOS, a different list per table"""
    rng = np.random.default_rng(seed)
    pool = U.WHITE[U.WHITE != ids.eos]
    t = rng.choice(pool, size=(B, n)).astype(np.int32)
    t[:, 0] = ids.prefix
    return t


def whitelist_gap(logits64):
    """[n] fp64: the best whitelisted logit minus the second best"""
    z = np.sort(np.asarray(logits64)[:, U.WHITE], axis=1)
    return z[:, -1] - z[:, -2]
