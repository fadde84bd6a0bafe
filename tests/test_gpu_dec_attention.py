"""GPU: the decode step's five single-query attention kernels (`dec_attention_kernel`, `dec_attn_fused_kernel<SELF | cross>`,
`dec_attn_fused2_kernel<SELF | cross>` of csrc/formula_decoder.hip) alone against fp64, through the developer entry `rd_debug_dec_attention`
(the launch functions of the decode step itself).  Lengths at which the kernels' loops change shape: the strides of the score loop (128 /
256 threads), the edges of the four-rows-in-flight loops of the output (`j + 48 < T` by 64, `j + 96 < T` by 128), the forced-EOS limit; cross lengths
around one key group and 144.  Flat / moderate / few-hot scores and a maximum that rises along the keys.  Cache rows the step must not read
are NaN; the SELF launches append this step's k, v as row `step` and touch nothing else; fused2 equals fused bit for bit.

Reference, yardstick and bound: tests/dec_reference.py.  The measured ratios are in docs/notebook/formula_decode_kernels.md."""
import pytest
import torch

import dec_reference as R

pytestmark = pytest.mark.gpu

# 47, 48, 111: the edge of the unfused kernel's four-rows-in-flight loop (`j + 48 < T` by 64 meets `j + 48 == T` at T = 48 .. 63, 112 .. 127;
# T = step + 1); 95, 96: the same edge of the fused kernels (`j + 96 < T` by 128)
SELF_STEPS = [0, 1, 31, 32, 47, 48, 95, 96, 97, 111, 127, 128, 129, 255, 256, 257, 300, 1535]
CROSS_S = [1, 3, 4, 5, 143, 144, 145]
BS = [1, 3]
SPREADS = [0.2, 3, 10]
GUARD_ROWS = 2          # cache rows behind row `step` (SELF) / behind the last key (cross), and one guard sequence behind the last
LDO = R.D + 32          # out rows carry 32 guard columns


def _cache(kc, vc, B, T, self_attn):
    """Device caches around the T valid rows of kc / vc [B][T][D].  SELF: [B + 1][T + 1 + GUARD_ROWS][D] each (the product's layout), rows >= T
    NaN.  cross: k | v interleaved [B + 1][T + GUARD_ROWS][2 D] (the product's ckv layout), rows >= T NaN.  Returns (k view, v view, ldkv,
    seq_stride, backing tensors)."""
    nan = float("nan")
    if self_attn:
        rows = T + 1 + GUARD_ROWS
        k = torch.full((B + 1, rows, R.D), nan)
        v = torch.full((B + 1, rows, R.D), nan)
        k[:B, :T] = kc
        v[:B, :T] = vc
        kd, vd = k.cuda(), v.cuda()
        return kd, vd, R.D, rows * R.D, (kd, vd)
    rows = T + GUARD_ROWS
    kv = torch.full((B + 1, rows, 2 * R.D), nan)
    kv[:B, :T, :R.D] = kc
    kv[:B, :T, R.D:] = vc
    kvd = kv.cuda()
    return kvd, kvd.reshape(-1)[R.D:], 2 * R.D, rows * 2 * R.D, (kvd,)


def launch(route, self_attn, B, T, case):
    """One launch.  Returns (out [B][D] on the CPU, new cache row k, v [B][D] or None, everything else untouched)."""
    kd, vd, ldkv, stride, backing = _cache(case["kc"], case["vc"], B, T, self_attn)
    before = [t.clone() for t in backing]
    out = torch.full((B + 2, LDO), R.SENTINEL, device="cuda")
    dev = {k: (v.cuda() if v is not None else None) for k, v in case.items() if k not in ("kc", "vc")}
    if route == 0:
        if self_attn:                                   # the product's packing: q | k | v rows of 3 D
            qkv = torch.cat([dev["q"], dev["kcur"], dev["vcur"]], 1).contiguous()
            q, kcur, vcur, ldq, ldcur = qkv, qkv.reshape(-1)[R.D:], qkv.reshape(-1)[2 * R.D:], 3 * R.D, 3 * R.D
        else:
            q, kcur, vcur, ldq, ldcur = dev["q"], None, None, R.D, 0
        rc = R.lib().rd_debug_dec_attention(0, int(self_attn), B, T, kd.data_ptr(), vd.data_ptr(), ldkv, stride, None, None, None, None, None,
                                            q.data_ptr(), ldq, R.ptr(kcur), R.ptr(vcur), ldcur, out.data_ptr(), LDO)
    else:
        rc = R.lib().rd_debug_dec_attention(route, int(self_attn), B, T, kd.data_ptr(), vd.data_ptr(), ldkv, stride, dev["x"].data_ptr(),
                                            dev["ln_g"].data_ptr(), dev["ln_b"].data_ptr(), dev["w"].data_ptr(), dev["bias"].data_ptr(),
                                            None, 0, None, None, 0, out.data_ptr(), LDO)
    assert rc == 0, rc
    oc = out.cpu()
    untouched = bool((oc[B:] == R.SENTINEL).all() and (oc[:B, R.D:] == R.SENTINEL).all())
    kn = vn = None
    after = [t.clone() for t in backing]
    if self_attn:
        kn, vn = after[0][:B, T].cpu(), after[1][:B, T].cpu()
        for a, b in zip(after, before):
            a[:B, T] = b[:B, T]                         # everything but row `step` of the B sequences must be unchanged, bit for bit
    untouched = untouched and all(R.same_bits(a.cpu(), b.cpu()) for a, b in zip(after, before))
    return oc[:B, :R.D], kn, vn, untouched


def check(route, self_attn, B, T, a2=None, rising=False, seed=0):
    make = R.unfused_case if route == 0 else R.fused_case
    case = make(B, T, self_attn, a2, seed + 7 * T + B, rising=rising)
    tag = f"route{route} {'self' if self_attn else 'cross'} B{B} T{T} " + ("rising" if rising else f"a2={a2}")
    out, kn, vn, untouched = launch(route, self_attn, B, T, case)
    assert untouched, tag
    if route == 0:
        k = torch.cat([case["kc"], case["kcur"][:, None]], 1) if self_attn else case["kc"]
        v = torch.cat([case["vc"], case["vcur"][:, None]], 1) if self_attn else case["vc"]
        ref, yard = R.single_query_attention(case["q"], k, v), R.single_query_attention(case["q"], k, v, torch.float32)
        if self_attn:                                   # the appended row is this step's k, v
            assert R.same_bits(kn, case["kcur"]) and R.same_bits(vn, case["vcur"]), tag
    else:
        args = (case["x"], case["ln_g"], case["ln_b"], case["w"], case["bias"], case["kc"], case["vc"], self_attn)
        ref, kr, vr = R.fused_attention_reference(*args)
        yard, ky, vy = R.fused_attention_reference(*args, dtype=torch.float32)
        if self_attn:
            R.bound_ratio(kn, kr, ky, tag + " k row")
            R.bound_ratio(vn, vr, vy, tag + " v row")
        if route == 2:                                  # the round-6 kernel equals the round-4 one bit for bit
            out1, kn1, vn1, _ = launch(1, self_attn, B, T, case)
            assert R.same_bits(out, out1), tag
            if self_attn:
                assert R.same_bits(kn, kn1) and R.same_bits(vn, vn1), tag
    return R.bound_ratio(out, ref, yard, tag)


@pytest.mark.parametrize("route", [0, 1, 2])
@pytest.mark.parametrize("step", SELF_STEPS)
def test_self_attention(step, route):
    for B in BS:
        for a2 in SPREADS:
            check(route, True, B, step, a2)


@pytest.mark.parametrize("route", [0, 1, 2])
@pytest.mark.parametrize("S", CROSS_S)
def test_cross_attention(S, route):
    for B in BS:
        for a2 in SPREADS:
            check(route, False, B, S, a2)


@pytest.mark.parametrize("route", [0, 1, 2])
@pytest.mark.parametrize("self_attn", [True, False])
def test_rising_maximum(self_attn, route):
    """The best score climbs by about 3 per 32 keys: the early keys' probabilities are tiny, the last key (SELF: this step's own) leads."""
    check(route, self_attn, 3, 300, rising=True)
    check(route, self_attn, 1, 144 if not self_attn else 129, rising=True)


def test_arguments_no_launch_can_take():
    z = torch.zeros((4, 4 * R.D), device="cuda")
    f = R.lib().rd_debug_dec_attention
    p = z.data_ptr()
    assert f(3, 1, 1, 1, p, p, R.D, 4 * R.D, p, p, p, p, p, None, 0, None, None, 0, p, R.D) == -1            # no such route
    assert f(1, 0, 1, 0, p, p, R.D, 4 * R.D, p, p, p, p, p, None, 0, None, None, 0, p, R.D) == -1            # cross over no keys
    assert f(1, 1, 1, 1, p, p, R.D, 4 * R.D, None, p, p, p, p, None, 0, None, None, 0, p, R.D) == -1         # fused without x
    assert f(0, 1, 1, 1, p, p, R.D, 4 * R.D, None, None, None, None, None, p, R.D, None, None, 0, p, R.D) == -1      # SELF without this step's k
    assert f(1, 1, 1, 1, p, p, R.D, R.D, p, p, p, p, p, None, 0, None, None, 0, p, R.D) == -1                # SELF: the cache has no row `step`
    assert f(1, 0, 1, 3, p, p, R.D, 2 * R.D, p, p, p, p, p, None, 0, None, None, 0, p, R.D) == -1            # cross: fewer cache rows than keys
    assert bool((z == 0).all())
