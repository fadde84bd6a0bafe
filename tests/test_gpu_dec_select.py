"""GPU: the decode step's token selection (`dec_select_kernel` of csrc/formula_decoder.hip, with and without the next step's embedding riding in
it) alone, through the developer entry `rd_debug_dec_select`: the argmax against np.argmax on the 16-byte path (V a multiple of 4, <= 65536)
and the scalar one, planted ties (the lower column wins), rows that are not finite (a NaN is the greatest value, a row of -inf names column
0: the token is always inside the vocabulary), the step's state (forced EOS at the length limit, PAD for finished sequences, one decrement per
fresh EOS, the arrival ticket, the step counter), and the embedding row of the next step against fp64 and, bit for bit, against
`dec_embed_ln_kernel`.

Reference, yardstick and bound: tests/dec_reference.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import dec_reference as R

pytestmark = pytest.mark.gpu

IDS_FILL = 7777
VS = [4, 4096, 4100, 50000, 50001, 65536, 65540]
BS = [1, 7, 33]


def select(z, step, unfinished=None, n_unfinished=None, ids_ld=None, embed=None, max_new=None):
    """One launch.  z [B][V] numpy fp32.  Returns (token column [B], unfinished after, state (step, n_unfinished, arrived), ids untouched
    elsewhere, x [B + 1][512] or None)."""
    B, V = z.shape
    ids_ld = ids_ld or step + 3
    unf = np.ones(B, np.int32) if unfinished is None else np.asarray(unfinished, np.int32)
    n_unf = int(unf.sum()) if n_unfinished is None else n_unfinished
    zd = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    ids = torch.full((B + 1, ids_ld), IDS_FILL, dtype=torch.int64, device="cuda")          # one guard row
    unfd = torch.from_numpy(np.concatenate([unf, [IDS_FILL]]).astype(np.int32)).cuda()      # one guard entry
    state = (C.c_int32 * 3)(-1, -1, -1)
    x = None
    e = [None] * 4
    if embed is not None:
        e = [t.cuda() for t in embed]
        x = torch.full((B + 1, R.D), R.SENTINEL, device="cuda")
    rc = R.lib().rd_debug_dec_select(0, zd.data_ptr(), V, B, step, ids.data_ptr(), ids_ld, unfd.data_ptr(), n_unf,
                                     max_new if max_new is not None else ids_ld - 1, R.ptr(e[0]), R.ptr(e[1]), R.ptr(e[2]), R.ptr(e[3]), R.ptr(x), state)
    assert rc == 0, rc
    idc = ids.cpu().numpy()
    tok = idc[:B, step + 1].copy()
    idc[:B, step + 1] = IDS_FILL
    unfc = unfd.cpu().numpy()
    assert unfc[B] == IDS_FILL
    return tok, unfc[:B], tuple(state), bool((idc == IDS_FILL).all()), (x.cpu() if x is not None else None)


def check(z, step=5, unfinished=None, tag=""):
    B, V = z.shape
    unf = np.ones(B, np.int32) if unfinished is None else np.asarray(unfinished, np.int32)
    tok, unf_after, state, untouched, _ = select(z, step, unf)
    want_tok, want_unf, want_n = R.select_reference(z, step, unf, int(unf.sum()))
    assert ((tok >= 0) & (tok < V)).all(), (tag, tok)
    assert (tok == want_tok).all(), (tag, np.nonzero(tok != want_tok)[0][:5], tok[:8], want_tok[:8])
    assert (unf_after == want_unf).all(), tag
    assert state == (step + 1, want_n, 0), (tag, state)                 # step advanced once, one decrement per fresh EOS, ticket back at 0
    assert untouched, tag                                               # only column step + 1 of rows 0 .. B - 1 was written
    return tok


def logits(B, V, seed):
    return np.random.default_rng(seed).standard_normal((B, V)).astype(np.float32)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("V", VS)
def test_argmax_equals_numpy(V, B):
    check(logits(B, V, V + B), tag=f"V{V} B{B}")


@pytest.mark.parametrize("V", VS)
def test_planted_ties_name_the_lower_column(V):
    pairs = R.tie_pairs(V)
    z = R.plant_ties(logits(2 * len(pairs) + 1, V, V), pairs)
    tok = check(z, tag=f"ties V{V}")
    for r in range(len(z)):
        assert tok[r] == pairs[r % len(pairs)][0]
    flat = np.zeros((3, V), np.float32)                                 # every column ties: column 0
    assert (check(flat, tag=f"flat V{V}") == 0).all()


@pytest.mark.parametrize("V", VS)
def test_rows_that_are_not_finite_stay_inside_the_vocabulary(V):
    """numpy / torch argmax: a NaN is the greatest value (the first one wins), +inf beats every finite value, a row of -inf names column 0."""
    z = logits(10, V, 7 * V)
    last, mid = V - 1, V // 2
    z[0, mid] = np.nan                                                  # one NaN among finite values
    z[1, :] = np.nan                                                    # all NaN: the first
    z[2, :] = -np.inf                                                   # all -inf: 0
    z[3, :] = -np.inf
    z[3, last] = -1e30                                                  # one finite value among -inf
    z[4, last] = np.inf
    z[4, 0] = -np.inf
    z[5, mid] = np.inf
    z[5, last] = np.inf                                                 # two +inf: the lower
    z[6, last] = np.nan
    z[6, 0] = np.inf                                                    # NaN beats +inf
    z[7, mid:] = np.nan                                                 # a run of NaN: its first
    z[8, :] = -np.inf
    z[8, mid] = np.inf
    z[9, :] = np.inf                                                    # all +inf: 0
    tok = check(z, tag=f"non-finite V{V}")
    assert tok.tolist() == [mid, 0, 0, last, last, mid, last, mid, mid, 0]


def test_forced_eos_at_the_length_limit_only():
    z = logits(3, 4100, 1)
    z[:, 77] = 50.0
    assert (check(z, step=R.FORCED_EOS_LEN - 2, tag="step 1535") == R.EOS).all()       # 1536 tokens in: only EOS survives
    assert (check(z, step=R.FORCED_EOS_LEN - 3, tag="step 1534") == 77).all()
    tok, unf, state, untouched, _ = select(z, R.FORCED_EOS_LEN - 2)
    assert state == (R.FORCED_EOS_LEN - 1, 0, 0) and (unf == 0).all() and untouched


def test_finished_sequences_get_pad_and_eos_is_counted_once():
    B = 7
    z = logits(B, 50000, 2)
    z[1, R.EOS] = 60.0                                                  # fresh EOS
    z[4, R.EOS] = 60.0                                                  # EOS again on a sequence that already ended: PAD, no decrement
    z[5, R.PAD] = 60.0                                                  # a live sequence may choose the pad id: not an end
    unf = np.array([1, 1, 0, 1, 0, 1, 1], np.int32)
    tok = check(z, step=9, unfinished=unf, tag="state")
    assert tok[1] == R.EOS and tok[2] == R.PAD and tok[4] == R.PAD and tok[5] == R.PAD
    tok, unf_after, state, _, _ = select(z, 9, unf)
    assert unf_after.tolist() == [1, 0, 0, 1, 0, 1, 1] and state == (10, 4, 0)


def _embed_tables(V, positions, seed):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn((V, R.D), generator=g) * (R.D ** 0.5) * 0.05      # the library stores emb * sqrt(d_model)
    pos = torch.randn((positions, R.D), generator=g)
    return emb, pos, 1.0 + 0.1 * torch.randn(R.D, generator=g), 0.1 * torch.randn(R.D, generator=g)


@pytest.mark.parametrize("B", BS)
def test_next_embedding_rides_in_the_select_launch(B):
    V, step = 4100, 6
    tables = _embed_tables(V, step + 4, 5)
    z = logits(B, V, 11 + B)
    unf = np.ones(B, np.int32)
    unf[B // 2] = 0                                                     # its row embeds PAD
    tok, _, state, untouched, x = select(z, step, unf, ids_ld=step + 3, embed=tables, max_new=step + 2)
    want_tok, _, _ = R.select_reference(z, step, unf, int(unf.sum()))
    assert (tok == want_tok).all() and untouched and state[0] == step + 1
    assert bool((x[B:] == R.SENTINEL).all())                            # nothing past row B - 1
    ref = R.embed_reference(*tables, tok, step + 3)
    R.bound_ratio(x[:B], ref, R.embed_reference(*tables, tok, step + 3, dtype=torch.float32), f"next embedding B{B}")
    # the same row from dec_embed_ln_kernel at step + 1 on the ids the select launch wrote: bit for bit
    ids = torch.full((B, step + 3), IDS_FILL, dtype=torch.int64)
    ids[:, step + 1] = torch.from_numpy(tok)
    idd = ids.cuda()
    e = [t.cuda() for t in tables]
    x2 = torch.full((B + 1, R.D), R.SENTINEL, device="cuda")
    state = (C.c_int32 * 3)(-1, -1, -1)
    rc = R.lib().rd_debug_dec_select(1, None, V, B, step + 1, idd.data_ptr(), step + 3, None, B, step + 2, e[0].data_ptr(), e[1].data_ptr(),
                                     e[2].data_ptr(), e[3].data_ptr(), x2.data_ptr(), state)
    assert rc == 0 and tuple(state) == (step + 1, B, 0)                 # the embedding launch leaves the state alone
    assert R.same_bits(x2.cpu(), x)
    assert bool(torch.equal(idd.cpu(), ids))


def test_no_embedding_after_the_last_step():
    V, step, B = 4096, 6, 3
    tables = _embed_tables(V, step + 4, 6)
    z = logits(B, V, 3)
    tok, _, state, untouched, x = select(z, step, ids_ld=step + 2, embed=tables, max_new=step + 1)      # t + 1 >= max_new: the loop ends here
    assert (tok == np.argmax(z, axis=1)).all() and state == (step + 1, B, 0) and untouched
    assert bool((x == R.SENTINEL).all())
