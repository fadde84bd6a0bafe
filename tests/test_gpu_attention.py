"""GPU: the recogniser tail's self-attention kernels alone (csrc/kernels_attention_h3.hip on the split-fp16 matrix cores, the VALU
`attention_kernel` of csrc/kernels_misc.hip) against fp64, through the developer entry `rd_debug_attention`: the product head size 15, the
ragged `seg` form, the lengths at which the code takes another path (key tiles of 32, the matrix-core kernel's longest line, the keys the VALU
kernel holds in LDS - all read from the library, `rd_debug_attention_limits`), flat / moderate / few-hot scores, a running maximum that
rises in every key tile, one launch that holds lines of both kernels, and the range flag of the fp16 conversion.

Reference: softmax(q scale @ k^T) @ v per (line, head) in fp64 on the same fp32 inputs.  Bound: the same formula evaluated by torch in plain
fp32 is the yardstick - the kernel's max-abs error against fp64 may be at most 4 x the yardstick's (the margin covers `__expf`'s extra
rounding of its argument and the online re-association) plus 2^-22 max|v| (one split-fp16 rounding of the output).  The measured ratios are
in docs/notebook/rec_tail_kernels.md."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
HEADS, HD = 8, 15


def attention_reference(qkv, lines, heads, hd, scale, dtype=torch.float64):
    """softmax(q scale @ k^T) @ v of every (line, head).  qkv [tokens][3 heads hd] (q | k | v, head-major), lines = (first token, tokens)
    pairs; returns [tokens][heads hd] in `dtype`, rows that no line owns are NaN."""
    c = heads * hd
    out = torch.full((qkv.shape[0], c), float("nan"), dtype=dtype)
    for first, n in lines:
        if n <= 0:
            continue
        r = qkv[first:first + n].to(dtype).reshape(n, 3, heads, hd).permute(1, 2, 0, 3)      # [3][heads][n][hd]
        p = torch.softmax((r[0] * torch.tensor(scale, dtype=dtype)) @ r[1].transpose(-1, -2), dim=-1)
        out[first:first + n] = (p @ r[2]).permute(1, 0, 2).reshape(n, c)
    return out


def place_lines(lengths, order=None, gap_after=None, gap=0, guard=0):
    """Token rows of a ragged launch.  Lines are laid down in `order` (default: as given, one after the other - where `ragged_tables` of
    rapiddoc_amd/engine.py puts them), `gap` unowned rows follow line `gap_after`, `guard` rows follow the last line.
    Returns (seg int32 [n][2] = (first token, tokens) in LINE order, total rows)."""
    lengths = [int(v) for v in lengths]
    seg = np.zeros((len(lengths), 2), dtype=np.int32)
    at = 0
    for i in (range(len(lengths)) if order is None else order):
        seg[i] = (at, lengths[i])
        at += lengths[i]
        if gap_after is not None and i == gap_after:
            at += gap
    return seg, at + guard


def random_qkv(tokens, heads, hd, a2, seed):
    """q, k ~ N(0, a2) per entry: with scale = hd^-1/2 the scaled scores have standard deviation a2.  v ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((tokens, 3, heads * hd), generator=g)
    x[:, :2] *= float(a2) ** 0.5
    return x.reshape(tokens, 3 * heads * hd).contiguous()


def rising_qkv(B, T, heads, hd, scale, seed, rise=3.0):
    """k_j = u (j + 1) / T g + noise, q_i = +-u g + noise for a unit vector u per head, with scale g^2 = rise T / 32: the best score of a
    '+' query (even i) climbs by `rise` from one tile of 32 keys to the next, so alpha = exp(-rise) in every tile; a '-' query (odd i) has
    its maximum in the first tile and its later probabilities fall through the fp16 subnormals to zero."""
    g = torch.Generator().manual_seed(seed)
    gain = (rise * max(T, 32) / 32.0 / scale) ** 0.5
    u = torch.randn((heads, hd), generator=g)
    u = u / u.norm(dim=1, keepdim=True)
    x = torch.randn((B, T, 3, heads, hd), generator=g)
    x[:, :, :2] *= 0.1
    sign = torch.where(torch.arange(T) % 2 == 0, 1.0, -1.0)
    x[:, :, 0] += sign[None, :, None, None] * gain * u
    x[:, :, 1] += ((torch.arange(T) + 1.0) / T)[None, :, None, None] * gain * u
    return x.reshape(B * T, 3 * heads * hd).contiguous()


def _lib():
    from rapiddoc_amd import _lib
    return _lib.load()


def limits(hd):
    """(longest line of the matrix-core kernel, keys the VALU kernel holds in LDS) at this head size, from the library."""
    a, b = C.c_int(-1), C.c_int(-1)
    assert _lib().rd_debug_attention_limits(hd, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def resolve(t, hd):
    """A length given as a number or as ('max_t' | 'lds', multiplier, offset)."""
    if isinstance(t, int):
        return t
    max_t, lds = limits(hd)
    return {"max_t": max_t, "lds": lds}[t[0]] * t[1] + t[2]


def launch(qkv, rows, B, T, heads, hd, scale, route, seg=None):
    """One launch into a sentinel-filled output of `rows` rows; returns (output on the CPU, range flag)."""
    q = qkv.cuda()
    o = torch.full((rows, heads * hd), SENTINEL, device="cuda")
    s = torch.from_numpy(seg).cuda() if seg is not None else None
    flag = C.c_int(-1)
    rc = _lib().rd_debug_attention(B, T, heads, hd, scale, q.data_ptr(), o.data_ptr(), s.data_ptr() if s is not None else None, route,
                                   C.byref(flag))
    assert rc == 0, rc
    return o.cpu(), flag.value


def check_bound(o, qkv, lines, heads, hd, scale, tag):
    """max-abs error of the owned rows against fp64 <= 4 x that of plain fp32 + 2^-22 max|v|.  Returns the ratio error / bound."""
    ref = attention_reference(qkv, lines, heads, hd, scale)
    yard = attention_reference(qkv, lines, heads, hd, scale, torch.float32)
    own = ~torch.isnan(ref[:, 0])
    assert bool(torch.isfinite(o[own]).all()), tag
    err = float((o[own].double() - ref[own]).abs().max())
    yerr = float((yard[own].double() - ref[own]).abs().max())
    vmax = float(qkv[:, 2 * heads * hd:].abs().max())
    bound = 4.0 * yerr + 2.0 ** -22 * vmax
    print(f"attention {tag}: err {err:.3e} fp32 yardstick {yerr:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert err <= bound, (tag, err, yerr, bound)
    return err / bound


def dense_lines(B, T):
    return [(b * T, T) for b in range(B)]


def run_dense(T, heads, hd, route, a2=None, rising=False, B=2, seed=0):
    T = resolve(T, hd)
    scale = hd ** -0.5
    qkv = rising_qkv(B, T, heads, hd, scale, seed + T) if rising else random_qkv(B * T, heads, hd, a2, seed + T)
    o, flag = launch(qkv, B * T + 3, B, T, heads, hd, scale, route)
    assert flag == 0
    assert bool((o[B * T:] == SENTINEL).all())                       # nothing past the last token
    return check_bound(o[:B * T], qkv, dense_lines(B, T), heads, hd, scale, f"route{route} hd{hd} T{T} " + ("rising" if rising else f"a2={a2}"))


ROUTE0_T = [1, 2, 31, 32, 33, 64, 65, 127, ("max_t", 1, -1), ("max_t", 1, 0)]


def _tid(t):
    return str(t) if isinstance(t, int) else "%s%s%+d" % (t[0], "" if t[1] == 1 else "x%d" % t[1], t[2])


@pytest.mark.parametrize("a2", [0.2, 3, 10])
@pytest.mark.parametrize("T", ROUTE0_T, ids=_tid)
def test_dense_engine_route_hd15(T, a2):
    run_dense(T, HEADS, HD, 0, a2=a2)


@pytest.mark.parametrize("T", [65, ("max_t", 1, 0)], ids=_tid)
def test_dense_engine_route_rising_maximum(T):
    """The running maximum moves up in every key tile (alpha << 1 each time) for even queries; odd ones underflow their late probabilities."""
    run_dense(T, HEADS, HD, 0, rising=True)


@pytest.mark.parametrize("a2", [0.2, 3, 10])
@pytest.mark.parametrize("T", [33, ("max_t", 1, 0)], ids=_tid)
def test_dense_engine_route_hd16(T, a2):
    run_dense(T, 2, 16, 0, a2=a2, B=3)


@pytest.mark.parametrize("a2", [0.2, 3, 10])
@pytest.mark.parametrize("T", [33, ("max_t", 1, 1), ("lds", 1, 0), ("lds", 1, 1), ("lds", 2, 1)], ids=_tid)
def test_dense_valu_route_hd15(T, a2):
    """The VALU kernel: one round of queries, beyond the matrix-core kernel's lines, the last length whose keys fit in LDS, and the
    key-tiled form with a one-key and a full-plus-one-key last tile."""
    run_dense(T, HEADS, HD, 1, a2=a2, B=1 if resolve(T, HD) > 1000 else 2)


def test_dense_valu_route_rising_maximum_tiled():
    run_dense(("lds", 1, 1), HEADS, HD, 1, rising=True, B=1)


@pytest.mark.parametrize("a2", [0.2, 10])
@pytest.mark.parametrize("T", [("lds", 1, 0), ("lds", 1, 1)], ids=_tid)
def test_dense_valu_route_hd32(T, a2):
    run_dense(T, 2, 32, 1, a2=a2, B=2)


def test_unknown_head_size_or_route_is_refused():
    q = torch.zeros((4, 3 * 2 * 24), device="cuda")
    o = torch.zeros((4, 2 * 24), device="cuda")
    lib = _lib()
    assert lib.rd_debug_attention(1, 4, 2, 24, 1.0, q.data_ptr(), o.data_ptr(), None, 0, None) == -1
    assert lib.rd_debug_attention(1, 4, 2, 15, 1.0, q.data_ptr(), o.data_ptr(), None, 3, None) == -1
    assert lib.rd_debug_attention(1, 4, 2, 32, 1.0, q.data_ptr(), o.data_ptr(), None, 2, None) == -1       # no matrix-core kernel at 32
    assert lib.rd_debug_attention_limits(24, None, None) == -1
    assert limits(32)[0] == 0 and limits(32)[1] < limits(15)[1]


# ----------------------------------------------------------------------------------------------------------------------------------------
# one ragged launch that holds lines of both kernels
# ----------------------------------------------------------------------------------------------------------------------------------------
def _ragged_case():
    max_t, lds = limits(HD)
    lengths = [33, 1, max_t, max_t + 1, 0, 5, lds + 1, 32]
    order = [5, 2, 7, 4, 0, 6, 1, 3]                              # where the lines sit in the token buffer
    seg, rows = place_lines(lengths, order=order, gap_after=0, gap=7, guard=3)
    qkv = random_qkv(rows, HEADS, HD, 3, 4242)
    return lengths, seg, rows, qkv, max_t, lds


def _owned(seg, rows):
    own = torch.zeros(rows, dtype=torch.bool)
    for first, n in seg.tolist():
        own[first:first + n] = True
    return own


def test_ragged_launch_of_both_kernels():
    lengths, seg, rows, qkv, max_t, lds = _ragged_case()
    scale = HD ** -0.5
    own = _owned(seg, rows)
    assert int((~own).sum()) == 7 + 3 and int(own.sum()) == sum(lengths)
    o, flag = launch(qkv, rows, len(lengths), max(lengths), HEADS, HD, scale, 0, seg)
    assert flag == 0
    assert bool((o[~own] == SENTINEL).all())                      # unowned rows, guard rows (and the empty line owns nothing)
    for i, (first, n) in enumerate(seg.tolist()):                 # every line against fp64 on its own
        if n:
            check_bound(o, qkv, [(first, n)], HEADS, HD, scale, f"ragged line {i} ({n} tokens)")
    for first, n in seg.tolist():                                 # a line's bits do not depend on its neighbours in the launch
        if n:
            alone, _ = launch(qkv[first:first + n].contiguous(), n, 1, n, HEADS, HD, scale, 0)
            assert torch.equal(alone, o[first:first + n]), n
    loose, flag = launch(qkv, rows, len(lengths), 2 * lds + 1, HEADS, HD, scale, 0, seg)      # T as a loose upper bound
    assert flag == 0 and torch.equal(loose, o)


def test_ragged_launch_matrix_core_kernel_only():
    lengths, seg, rows, qkv, max_t, lds = _ragged_case()
    scale = HD ** -0.5
    o0, _ = launch(qkv, rows, len(lengths), max(lengths), HEADS, HD, scale, 0, seg)
    o2, flag = launch(qkv, rows, len(lengths), max(lengths), HEADS, HD, scale, 2, seg)
    assert flag == 0
    for first, n in seg.tolist():
        if n > max_t:
            assert bool((o2[first:first + n] == SENTINEL).all()), n           # the VALU kernel's lines are left alone
        else:
            assert torch.equal(o2[first:first + n], o0[first:first + n]), n
    assert bool((o2[~_owned(seg, rows)] == SENTINEL).all())


def test_ragged_launch_valu_kernel_for_every_line():
    lengths, seg, rows, qkv, max_t, lds = _ragged_case()
    scale = HD ** -0.5
    o, flag = launch(qkv, rows, len(lengths), max(lengths), HEADS, HD, scale, 1, seg)
    assert flag == 0 and bool((o[~_owned(seg, rows)] == SENTINEL).all())
    check_bound(o, qkv, [tuple(r) for r in seg.tolist()], HEADS, HD, scale, "ragged, VALU for every line")


# ----------------------------------------------------------------------------------------------------------------------------------------
# range: a K, V or scaled Q value that the fp16 split cannot hold
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["none", "k", "v", "q"])
def test_range_flag_of_the_matrix_core_kernel(which):
    B, T = 2, 65
    scale = HD ** -0.5
    c = HEADS * HD
    qkv = random_qkv(B * T, HEADS, HD, 1, 99)
    tok, col = T + 40, 3 * HD + 7                                  # line 1, head 3, dim 7
    if which == "k":
        qkv[tok, c + col] = 7.0e4
    elif which == "v":
        qkv[tok, 2 * c + col] = -7.0e4
    elif which == "q":
        qkv[tok, col] = 1.1 * 65504.0 / scale                     # what the kernel converts is q scale
    for route in (0, 2):
        _o, flag = launch(qkv, B * T, B, T, HEADS, HD, scale, route)
        assert flag == (0 if which == "none" else 1), (which, route, flag)
    o, flag = launch(qkv, B * T, B, T, HEADS, HD, scale, 1)      # the fp32 route on the same inputs: finite and within the bound
    assert flag == 0
    check_bound(o, qkv, dense_lines(B, T), HEADS, HD, scale, f"VALU route, out-of-range {which}")


def test_range_flag_only_for_lines_the_matrix_core_kernel_serves():
    """A large value in a line beyond the matrix-core kernel's limit is never converted to fp16: no flag, fp32 result."""
    max_t, _lds = limits(HD)
    lengths = [max_t + 1, 40]
    seg, rows = place_lines(lengths)
    scale = HD ** -0.5
    qkv = random_qkv(rows, HEADS, HD, 1, 7)
    qkv[5, 2 * HEADS * HD + 3] = 7.0e4                            # a V value of line 0 (VALU)
    o, flag = launch(qkv, rows, 2, max(lengths), HEADS, HD, scale, 0, seg)
    assert flag == 0
    check_bound(o, qkv, [tuple(r) for r in seg.tolist()], HEADS, HD, scale, "large V in a VALU line")
    qkv[max_t + 1 + 5, 2 * HEADS * HD + 3] = 7.0e4                # ... and of line 1 (matrix cores)
    _o, flag = launch(qkv, rows, 2, max(lengths), HEADS, HD, scale, 0, seg)
    assert flag == 1
