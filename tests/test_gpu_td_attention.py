"""GPU: `td_attn_kernel` and its per-slot copy `td_stream_attn_kernel` (csrc/table_decoder.hip) alone against fp64, through the developer
entry `rd_debug_td_attention` (the launch function of decode() / decode_stream()).  Self and cross forms at the lengths where the kernel's
loops change shape: one key, the four waves of the P V loop (3, 4, 5), one wavefront (63 .. 65), the 256-stride score loop's second, third and
fourth trip (255 .. 257, 511 .. 513) and the full LDS score array (1023, 1024).  Flat / moderate / few-hot scores and a maximum that rises
along the keys.  Cache rows the launch must not read are NaN, as are the guard columns of every leading dimension; the self form appends this
step's k, v as row `pos` and changes no other byte.  The stream form equals the batch form bit for bit at every slot's own length, reads the
cross block of the slot's TABLE, and leaves an idle slot's row and cache alone.

Reference, yardstick and bound: tests/td_reference.py.  The measured ratios are in docs/notebook/table_decode_kernels.md."""
import pytest
import torch

import td_reference as R

pytestmark = pytest.mark.gpu

SELF_KEYS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024]          # T + 1: the cached rows and this step's
CROSS_S = [1, 3, 4, 5, 255, 256, 257, 784, 1023, 1024]
B8_KEYS = [1, 257, 1024]                # B = 8 at a few lengths only (time)
SPREADS = [0.2, 3, 10]
GUARD_ROWS = 2                          # rows behind the last one a sequence may touch; out rows in front of and behind the B written
LDKV, LDO, LDQ = R.D + 64, R.D + 32, 3 * R.D + 64        # every leading dimension carries guard columns
NAN = float("nan")


def cache_buffers(seqs_k, seqs_v, rows):
    """Device k, v [1 + n + 1][rows][LDKV]: sequence i's valid rows in block 1 + i, NaN everywhere else - the rows at and behind its length,
    the guard columns, a guard sequence in front and one behind."""
    n = len(seqs_k)
    k, v = torch.full((n + 2, rows, LDKV), NAN), torch.full((n + 2, rows, LDKV), NAN)
    for i, (a, b) in enumerate(zip(seqs_k, seqs_v)):
        if a is not None and len(a):
            k[1 + i, :len(a), :R.D] = a
            v[1 + i, :len(a), :R.D] = b
    return k.cuda(), v.cuda()


def query_rows(q, kcur=None, vcur=None):
    """The product's packing q | k | v per row (cross: q alone) in rows of LDQ; what is not given is NaN"""
    t = torch.full((q.shape[0], LDQ), NAN)
    t[:, :R.D] = q
    if kcur is not None:
        t[:, R.D:2 * R.D], t[:, 2 * R.D:3 * R.D] = kcur, vcur
    return t.cuda()


def launch(stream_form, self_attn, B, T, kd, vd, qd, src=None, pos=None, first_block=1):
    """One launch on blocks first_block .. of the cache buffers.  Returns out [B][LDO] on the CPU; the rows around it must be unchanged."""
    out = torch.full((GUARD_ROWS + B + GUARD_ROWS, LDO), R.SENTINEL, device="cuda")
    flat = qd.reshape(-1)
    kcur, vcur = (flat[R.D:], flat[2 * R.D:]) if self_attn else (None, None)
    i32 = lambda a: None if a is None else torch.tensor(a, dtype=torch.int32)
    srct, post = i32(src), i32(pos)
    rc = R.lib().rd_debug_td_attention(stream_form, int(self_attn), B, T, kd[first_block:].data_ptr(), vd[first_block:].data_ptr(), LDKV,
                                       kd.shape[1] * LDKV, qd.data_ptr(), LDQ, R.ptr(kcur), R.ptr(vcur), LDQ if self_attn else 0,
                                       out[GUARD_ROWS:].data_ptr(), LDO, R.ptr(srct), R.ptr(post))
    assert rc == 0, rc
    oc = out.cpu()
    assert bool((oc[:GUARD_ROWS] == R.SENTINEL).all() and (oc[GUARD_ROWS + B:] == R.SENTINEL).all()), "out rows around the B written ones changed"
    return oc[GUARD_ROWS:GUARD_ROWS + B]


def written_rows_then_nothing_else(before, after, appended, tag):
    """appended = [(block, row, k [768], v [768])]: those rows hold this step's k, v bit for bit, every other byte of both caches is unchanged"""
    for buf, (b0, a0) in enumerate(zip(before, after)):
        a = a0.clone()
        for blk, row, k, v in appended:
            assert R.same_bits(a[blk, row, :R.D].cpu(), (k, v)[buf]), (tag, "appended row", blk, row)
            a[blk, row, :R.D] = b0[blk, row, :R.D]
        assert R.same_bits(a, b0), (tag, "cache bytes outside the appended rows changed")


def live_columns(out, tag):
    assert bool((out[:, R.D:] == R.SENTINEL).all()), (tag, "guard columns of out changed")
    return out[:, :R.D]


def check(self_attn, B, T, a2=None, rising=False, seed=0):
    """Batch form; T = cached keys"""
    case = R.attention_case(B, T, self_attn, a2, seed + 7 * T + B, rising=rising)
    tag = f"td_attn {'self' if self_attn else 'cross'} B{B} keys{T + int(self_attn)} " + ("rising" if rising else f"a2={a2}")
    kd, vd = cache_buffers(list(case["kc"]), list(case["vc"]), T + int(self_attn) + GUARD_ROWS)
    before = (kd.clone(), vd.clone())
    out = live_columns(launch(0, self_attn, B, T, kd, vd, query_rows(case["q"], case["kcur"], case["vcur"])), tag)
    appended = [(1 + b, T, case["kcur"][b], case["vcur"][b]) for b in range(B)] if self_attn else []
    written_rows_then_nothing_else(before, (kd, vd), appended, tag)
    return R.bound_ratio(out, R.attention_reference(case), R.attention_reference(case, torch.float32), tag)


@pytest.mark.parametrize("keys", SELF_KEYS)
def test_self_attention(keys):
    for B in [1, 3] + ([8] if keys in B8_KEYS else []):
        for a2 in SPREADS:
            check(True, B, keys - 1, a2)


@pytest.mark.parametrize("S", CROSS_S)
def test_cross_attention(S):
    for B in [1, 3] + ([8] if S in B8_KEYS else []):
        for a2 in SPREADS:
            check(False, B, S, a2)


@pytest.mark.parametrize("self_attn", [True, False])
def test_rising_maximum(self_attn):
    """The best score climbs by about 3 per 32 keys: the early keys' probabilities are tiny, the last key (self: this step's own) leads."""
    check(self_attn, 3, 300, rising=True)
    check(self_attn, 1, R.MAXPOS - int(self_attn), rising=True)


@pytest.mark.parametrize("a2", SPREADS)
def test_stream_self_form_equals_the_batch_form_at_every_slots_own_length(a2):
    """One launch of 8 slots at positions on both sides of 256 and at the last cache row, two of them idle"""
    src = [5, 2, 9, 0, -1, 7, 3, -1]
    pos = [0, 3, 255, 256, 0, 257, 1023, 0]
    cases = [R.attention_case(1, p, True, a2, 50 + s) if t >= 0 else None for s, (t, p) in enumerate(zip(src, pos))]
    kd, vd = cache_buffers([c["kc"][0] if c else None for c in cases], [c["vc"][0] if c else None for c in cases], R.MAXPOS + GUARD_ROWS)
    before = (kd.clone(), vd.clone())
    pick = lambda name: torch.cat([c[name] if c else torch.full((1, R.D), NAN) for c in cases])
    qd = query_rows(pick("q"), pick("kcur"), pick("vcur"))
    out = launch(1, True, 8, 0, kd, vd, qd, src, pos)
    live = [s for s in range(8) if src[s] >= 0]
    tag = f"td_stream_attn self a2={a2}"
    for s in range(8):
        if src[s] < 0:
            assert bool((out[s] == R.SENTINEL).all()), (tag, "an idle slot's out row was written", s)
    written_rows_then_nothing_else(before, (kd, vd), [(1 + s, pos[s], cases[s]["kcur"][0], cases[s]["vcur"][0]) for s in live], tag)
    for s in live:
        k1, v1 = before[0].clone(), before[1].clone()
        one = launch(0, True, 1, pos[s], k1, v1, qd[s:s + 1], first_block=1 + s)
        assert R.same_bits(out[s:s + 1], one), (tag, "slot differs from the batch kernel at its length", s)
        assert R.same_bits(k1[1 + s], kd[1 + s]) and R.same_bits(v1[1 + s], vd[1 + s]), (tag, "the slot's cache differs from the batch kernel's", s)
    got = live_columns(out[live], tag)
    ref = torch.cat([R.attention_reference(cases[s]) for s in live])
    yard = torch.cat([R.attention_reference(cases[s], torch.float32) for s in live])
    R.bound_ratio(got, ref, yard, tag + " positions " + str([pos[s] for s in live]))


def test_stream_cross_form_reads_the_block_of_the_slots_table():
    """11 tables, S = 257, 8 slots that hold tables far from their slot numbers (slot 0 holds table 10) and one idle slot"""
    N, S = 11, 257
    src = [10, 7, 0, 9, -1, 5, 1, 8]
    case = R.attention_case(N, S, False, 3, 77)
    kd, vd = cache_buffers(list(case["kc"]), list(case["vc"]), S + GUARD_ROWS)
    before = (kd.clone(), vd.clone())
    q = case["q"][:8].clone()
    q[4] = NAN
    qd = query_rows(q)
    out = launch(1, False, 8, S, kd, vd, qd, src, [0, 3, 255, 256, 0, 257, 1023, 0])
    tag = "td_stream_attn cross N11 S257"
    written_rows_then_nothing_else(before, (kd, vd), [], tag)
    assert bool((out[4] == R.SENTINEL).all()), (tag, "the idle slot's out row was written")
    live = [s for s in range(8) if src[s] >= 0]
    for s in live:
        one = launch(0, False, 1, S, kd, vd, qd[s:s + 1], first_block=1 + src[s])
        assert R.same_bits(out[s:s + 1], one), (tag, "slot differs from the batch kernel on its table's block", s)
    tables = [src[s] for s in live]
    args = (case["q"][live], case["kc"][tables], case["vc"][tables])
    R.bound_ratio(live_columns(out[live], tag), R.single_query_attention(*args), R.single_query_attention(*args, torch.float32), tag)


def test_arguments_no_launch_can_take():
    f = R.lib().rd_debug_td_attention
    kv = torch.zeros((8, 4, R.D), device="cuda")
    q = torch.zeros((8, 3 * R.D), device="cuda")
    out = torch.full((8, R.D), R.SENTINEL, device="cuda")
    k, qp, o = kv.data_ptr(), q.data_ptr(), out.data_ptr()
    kc, vc = qp + 4 * R.D, qp + 8 * R.D
    st = 4 * R.D
    src, pos = torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
    sp, pp = src.data_ptr(), pos.data_ptr()
    ok_self = lambda: f(0, 1, 1, 3, k, k, R.D, st, qp, 3 * R.D, kc, vc, 3 * R.D, o, R.D, None, None)
    assert f(0, 1, 0, 3, k, k, R.D, st, qp, 3 * R.D, kc, vc, 3 * R.D, o, R.D, None, None) == -1          # B = 0
    assert f(0, 1, 9, 3, k, k, R.D, st, qp, 3 * R.D, kc, vc, 3 * R.D, o, R.D, None, None) == -1          # B = 9
    assert f(0, 1, 1, -1, k, k, R.D, st, qp, 3 * R.D, kc, vc, 3 * R.D, o, R.D, None, None) == -1         # self: no cached row -1
    assert f(0, 1, 1, 1024, k, k, R.D, 1025 * R.D, qp, 3 * R.D, kc, vc, 3 * R.D, o, R.D, None, None) == -1      # self: 1025 keys
    assert f(0, 0, 1, 0, k, k, R.D, st, qp, 3 * R.D, None, None, 0, o, R.D, None, None) == -1            # cross over no keys
    assert f(0, 0, 1, 1025, k, k, R.D, 1025 * R.D, qp, 3 * R.D, None, None, 0, o, R.D, None, None) == -1        # cross: 1025 keys
    assert f(0, 1, 1, 4, k, k, R.D, st, qp, 3 * R.D, kc, vc, 3 * R.D, o, R.D, None, None) == -1          # self: the cache has no row 4
    assert f(0, 0, 1, 5, k, k, R.D, st, qp, 3 * R.D, None, None, 0, o, R.D, None, None) == -1            # cross: fewer cache rows than keys
    assert f(0, 1, 1, 3, k, k, R.D - 4, st, qp, 3 * R.D, kc, vc, 3 * R.D, o, R.D, None, None) == -1      # ldkv
    assert f(0, 1, 1, 3, k, k, R.D, st, qp, R.D - 1, kc, vc, 3 * R.D, o, R.D, None, None) == -1          # ldq
    assert f(0, 1, 1, 3, k, k, R.D, st, qp, 3 * R.D, kc, vc, R.D - 4, o, R.D, None, None) == -1          # ldcur
    assert f(0, 1, 1, 3, k, k, R.D, st, qp, 3 * R.D, kc, vc, 3 * R.D, o, R.D - 1, None, None) == -1      # ldo
    assert f(0, 1, 1, 3, k, k, R.D, st, qp, 3 * R.D, None, vc, 3 * R.D, o, R.D, None, None) == -1        # self without this step's k
    assert f(0, 1, 1, 3, None, k, R.D, st, qp, 3 * R.D, kc, vc, 3 * R.D, o, R.D, None, None) == -1
    assert f(1, 1, 1, 0, k, k, R.D, st, qp, 3 * R.D, kc, vc, 3 * R.D, o, R.D, None, None) == -1          # stream form without the slots' state
    pos[0] = 4
    assert f(1, 1, 1, 0, k, k, R.D, st, qp, 3 * R.D, kc, vc, 3 * R.D, o, R.D, sp, pp) == -1              # stream: the slot's cache has no row 4
    pos[0] = 1024
    assert f(1, 1, 1, 0, k, k, R.D, 1025 * R.D, qp, 3 * R.D, kc, vc, 3 * R.D, o, R.D, sp, pp) == -1      # stream: position 1024
    pos[0], src[0] = 0, -2
    assert f(1, 1, 1, 0, k, k, R.D, st, qp, 3 * R.D, kc, vc, 3 * R.D, o, R.D, sp, pp) == -1              # no such table
    assert bool((out == R.SENTINEL).all() and (kv == 0).all())
    assert ok_self() == 0 and bool((out[0] == 0).all() and (out[1:] == R.SENTINEL).all())
