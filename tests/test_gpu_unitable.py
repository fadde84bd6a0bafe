"""GPU: the UniTable table-structure encoder (`unitable_encoder`) and its new kernels (csrc/kernels_vit_attn.hip).

Attention alone, through the developer entry `rd_debug_vit_attention`, against fp64 on the same fp32 inputs: lengths below, at and across the
64-key tile and the 64-row workgroup (1, 6, 63, 64, 65, 130) and the product length 784; batches 1 and 3 at score deviation 3; flat and
few-hot scores (deviation 0.2 / 10) at B = 3 and T = 65 and 784 only - one length across a tile edge and the longest: the deviation changes
the values the softmax sees, not the path the kernel takes; a row whose maximum rises in every key tile; NaN guard rows around the packed q | k | v rows and around the
output (never read, never written); the last sequence of a batch of three equal to the same sequence alone, bit for bit.
Bound, the convention of tests/test_gpu_attention.py: max-abs error <= 4 x that of the same formula in plain torch fp32 on the CPU
+ 2^-22 max|ref|.

LayerNorm at C = 768 through `rd_debug_layernorm` against fp64.

The encoder against the four reference-minted fixtures in the `auto` and `fp32` precisions: every tap (patch embedding, layers 0 and 11,
memory) within 1e-3 max(1, max|ref|), the project's fixture bound; image 1 of the B = 2 fixture equal to that image alone, bit for bit;
repeated forwards (the hipGraph replay) equal to the first; shapes outside the kernel's limits declined with a message."""
import os

import numpy as np
import pytest
import torch

import unitable_reference as R

pytestmark = pytest.mark.gpu

HD = 64
def _lib():
    from rapiddoc_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- attention alone
def reference(qkv, heads, scale, dtype):
    """qkv [B,T,3 heads 64] -> softmax(q scale @ k^T) @ v as [B,T,heads 64] in `dtype`"""
    B, T, _ = qkv.shape
    r = qkv.to(dtype).reshape(B, T, 3, heads, HD).permute(2, 0, 3, 1, 4)
    p = torch.softmax((r[0] * torch.tensor(scale, dtype=dtype)) @ r[1].transpose(-1, -2), dim=-1)
    return (p @ r[2]).permute(0, 2, 1, 3).reshape(B, T, heads * HD)


def random_qkv(B, T, heads, dev, seed):
    """q, k ~ N(0, dev): with scale 1/8 the scaled scores have standard deviation `dev`; v ~ N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, T, 3, heads * HD), generator=g)
    x[:, :, :2] *= float(dev) ** 0.5
    return x.reshape(B, T, 3 * heads * HD).contiguous()


def rising_qkv(B, T, heads, scale, seed, rise=3.0):
    """k_j = u (j + 1) / T g + noise, q_i = +-u g + noise, u a unit vector per head and scale g^2 = rise T / 64: the best score of an even
    query climbs by `rise` from one tile of 64 keys to the next (alpha = exp(-rise) in every tile); an odd query has its maximum in the first
    tile and its later probabilities fall to zero"""
    g = torch.Generator().manual_seed(seed)
    gain = (rise * max(T, 64) / 64.0 / scale) ** 0.5
    u = torch.randn((heads, HD), generator=g)
    u = u / u.norm(dim=1, keepdim=True)
    x = torch.randn((B, T, 3, heads, HD), generator=g)
    x[:, :, :2] *= 0.1
    sign = torch.where(torch.arange(T) % 2 == 0, 1.0, -1.0)
    x[:, :, 0] += sign[None, :, None, None] * gain * u
    x[:, :, 1] += ((torch.arange(T) + 1.0) / T)[None, :, None, None] * gain * u
    return x.reshape(B, T, 3 * heads * HD).contiguous()


GUARD = 3       # NaN rows in front of and behind the packed rows and the output rows


def launch(qkv, heads, scale):
    """One launch between NaN guard rows; returns the output on the CPU after checking that the guards are still NaN"""
    B, T, c3 = qkv.shape
    qbuf = torch.full((B * T + 2 * GUARD, c3), float("nan"), device="cuda")
    qbuf[GUARD:GUARD + B * T] = qkv.reshape(B * T, c3).cuda()
    obuf = torch.full((B * T + 2 * GUARD, heads * HD), float("nan"), device="cuda")
    rc = _lib().rd_debug_vit_attention(B, T, heads, HD, scale, qbuf[GUARD].data_ptr(), obuf[GUARD].data_ptr())
    assert rc == 0, rc
    o = obuf.cpu()
    assert bool(torch.isnan(o[:GUARD]).all()) and bool(torch.isnan(o[GUARD + B * T:]).all()), "a guard row of the output was written"
    assert bool(torch.isnan(qbuf.cpu()[[0, -1]]).all())
    return o[GUARD:GUARD + B * T].reshape(B, T, heads * HD)


def check_bound(o, qkv, heads, scale, tag):
    ref = reference(qkv, heads, scale, torch.float64)
    yard = reference(qkv, heads, scale, torch.float32)
    assert bool(torch.isfinite(o).all()), tag          # a guard row that was read would show here
    err = float((o.double() - ref).abs().max())
    yerr = float((yard.double() - ref).abs().max())
    bound = 4.0 * yerr + 2.0 ** -22 * float(ref.abs().max())
    print(f"\nvit attention {tag}: err {err:.3e} fp32 yardstick {yerr:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert err <= bound, (tag, err, yerr, bound)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 6, 63, 64, 65, 130, 784])
def test_attention_alone_against_fp64(T, B):
    heads = 12 if T == 784 and B == 1 else 3
    qkv = random_qkv(B, T, heads, 3.0, 100 * T + B)
    check_bound(launch(qkv, heads, 0.125), qkv, heads, 0.125, f"T{T} B{B} heads{heads} dev3")


@pytest.mark.parametrize("dev", [0.2, 10.0])
@pytest.mark.parametrize("T", [65, 784])
def test_attention_flat_and_few_hot_scores(T, dev):
    qkv = random_qkv(3, T, 3, dev, 7 * T)
    check_bound(launch(qkv, 3, 0.125), qkv, 3, 0.125, f"T{T} B3 dev{dev}")


@pytest.mark.parametrize("T", [130, 784])
def test_attention_row_maximum_rising_along_the_keys(T):
    qkv = rising_qkv(2, T, 3, 0.125, T)
    check_bound(launch(qkv, 3, 0.125), qkv, 3, 0.125, f"T{T} rising")


@pytest.mark.parametrize("T", [65, 784])
def test_a_sequence_does_not_depend_on_its_batch(T):
    qkv = random_qkv(3, T, 3, 3.0, 11 + T)
    o3 = launch(qkv, 3, 0.125)
    o1 = launch(qkv[2:3].contiguous(), 3, 0.125)
    assert torch.equal(o3[2], o1[0])


def test_attention_entry_declines_what_the_kernel_does_not_serve():
    x = torch.zeros((8, 3 * 64), device="cuda")
    o = torch.zeros((8, 64), device="cuda")
    lib = _lib()
    assert lib.rd_debug_vit_attention(1, 8, 1, 32, 0.125, x.data_ptr(), o.data_ptr()) == -1       # head size
    assert lib.rd_debug_vit_attention(1, 1025, 1, 64, 0.125, x.data_ptr(), o.data_ptr()) == -1    # longer than the position table
    assert lib.rd_debug_vit_attention(1, 0, 1, 64, 0.125, x.data_ptr(), o.data_ptr()) == -1


def test_layernorm_at_768_against_fp64():
    g = torch.Generator().manual_seed(3)
    M, Cn, xld, yld = 7, 768, 776, 772
    x = torch.randn((M, xld), generator=g) * 3.0 + 1.5
    gm, bt = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g)
    xd, gd, bd = x.cuda(), gm.cuda(), bt.cuda()
    y = torch.full((M, yld), -777.25, device="cuda")
    assert _lib().rd_debug_layernorm(M, Cn, xd.data_ptr(), xld, y.data_ptr(), yld, gd.data_ptr(), bd.data_ptr(), 1e-5) == 0
    y = y.cpu()
    ref = torch.nn.functional.layer_norm(x[:, :Cn].double(), (Cn,), gm.double(), bt.double(), 1e-5)
    yard = torch.nn.functional.layer_norm(x[:, :Cn], (Cn,), gm, bt, 1e-5)
    err, yerr = float((y[:, :Cn].double() - ref).abs().max()), float((yard.double() - ref).abs().max())
    print(f"\nlayernorm768: err {err:.3e} fp32 yardstick {yerr:.3e}")
    assert err <= 4.0 * yerr + 2.0 ** -22 * float(ref.abs().max())
    assert bool((y[:, Cn:] == -777.25).all())          # the columns behind C stay untouched


# ---------------------------------------------------------------------------------------------------------------- the encoder
_ENG = {}


def _engine(golden_dir, precision):
    """One engine per precision for the module: RD_PRECISION is read when the handle is created"""
    if precision not in _ENG:
        from rapiddoc_amd.engine import RdEngine
        old = os.environ.get("RD_PRECISION")
        os.environ["RD_PRECISION"] = precision
        try:
            _ENG[precision] = RdEngine(R.KIND, guard="off").load_weights(R.state(golden_dir))
        finally:
            if old is None:
                os.environ.pop("RD_PRECISION", None)
            else:
                os.environ["RD_PRECISION"] = old
    return _ENG[precision]


@pytest.mark.parametrize("precision", ["auto", "fp32"])
@pytest.mark.parametrize("tag", R.TAGS)
def test_encoder_matches_the_reference_fixtures(golden_dir, tag, precision):
    eng = _engine(golden_dir, precision)
    x, g = R.fixture(golden_dir, tag)
    memory, taps = eng.table_encoder_forward(torch.from_numpy(x), want_taps=True)
    assert not eng.range_overflow()
    got = dict(zip(("patch", "layer0", "layer11"), taps), memory=memory)
    msgs = []
    for name in R.TAPS:
        ref = torch.from_numpy(g[name])
        err = float((R.sub(got[name].cpu(), g, name) - ref).abs().max())
        bound = R.FIXTURE_TOL * max(1.0, float(ref.abs().max()))
        msgs.append(f"{name} {err:.2e} / {bound:.2e}")
        assert err <= bound, (tag, precision, name, err, bound)
    print(f"\n[unitable encoder {tag} {precision}] max-abs errors: " + ", ".join(msgs))
    # the public entry (no taps: another plan) gives the same memory, bit for bit
    assert torch.equal(eng.table_encoder_forward(torch.from_numpy(x)), memory)


@pytest.mark.parametrize("precision", ["auto", "fp32"])
def test_an_image_does_not_depend_on_the_batch_it_rides_in(golden_dir, precision):
    eng = _engine(golden_dir, precision)
    x, _ = R.fixture(golden_dir, "b2_h48_w208")
    both = eng.table_encoder_forward(torch.from_numpy(x)).clone()
    alone = eng.table_encoder_forward(torch.from_numpy(x[1:2].copy()))
    assert torch.equal(both[1], alone[0])


def test_repeated_forwards_replay_and_agree(golden_dir):
    eng = _engine(golden_dir, "auto")
    x, _ = R.fixture(golden_dir, "b1_h64_w272")
    xd = torch.from_numpy(x).cuda()
    out = torch.empty((1, 68, 768), device="cuda")
    first = eng.table_encoder_forward(xd, out=out).clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()            # (the null stream cannot be captured: a stream of the caller's, as the page pipeline has)
    before = eng.plan_stats()["graph_replays"]
    with torch.cuda.stream(side):
        for _ in range(4):
            assert torch.equal(eng.table_encoder_forward(xd, out=out), first)
    side.synchronize()
    assert eng.plan_stats()["graph_replays"] > before


def test_shapes_outside_the_limits_are_declined_with_a_message(golden_dir):
    from rapiddoc_amd.engine import EngineError
    eng = _engine(golden_dir, "auto")
    with pytest.raises(EngineError, match="multiples of 16"):
        eng.table_encoder_forward(torch.zeros((1, 3, 40, 48)))
    with pytest.raises(EngineError, match="1024"):
        eng.table_encoder_forward(torch.zeros((1, 3, 528, 512)))          # 33 x 32 = 1056 patches
    # the library itself says so too (the wrapper's check aside)
    lib = eng._l
    xd, out = torch.zeros((1, 3, 528, 512), device="cuda"), torch.zeros((1, 1056, 768), device="cuda")
    assert lib.rd_table_encoder_forward(eng._h, xd.data_ptr(), 1, 528, 512, out.data_ptr(), None, 0, None) != 0
    assert b"1024" in lib.rd_last_error(eng._h)
    assert lib.rd_table_encoder_forward(eng._h, xd.data_ptr(), 1, 40, 48, out.data_ptr(), None, 0, None) != 0
    assert b"multiples of 16" in lib.rd_last_error(eng._h)
