"""GPU: the whole decode step of the formula decoder (csrc/formula_decoder.hip) on every batch route, against fp64.  The decode batch B selects
the kernels: 1 .. 8, 9 .. 16 (16 is `FormulaRecognizer.batch_predict`'s default batch), 17 .. 32 - three sets of `dec_gemv_kernel`
instantiations behind the fused attention launches - and > 32: the unfused attention with every linear on the GEMM path.  The developer entry
`rd_debug_formula_decode` is `rd_formula_decode` plus two traces written inside every step (graph replay included): the step's logits and
the hidden row in front of the final LayerNorm.

The GPU's own ids are fed to the teacher-forced fp64 reference (tests/dec_reference.py `step_reference`; yardstick: the same in fp32), so no
step is excluded: hidden rows and logits of every live step are within the bound, and the token the GPU chose is, in fp64, at most twice the
logits' bound below the row's fp64 maximum.  The measured ratios are in docs/notebook/formula_decode_kernels.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import dec_reference as R

pytestmark = pytest.mark.gpu

V = 50000
POOL = {}
RUNS = {}


@pytest.fixture(scope="module")
def decoder(golden_dir):
    from rapiddoc_amd.engine import RdEngine
    from test_oracle_golden import formula_long_case
    st, _enc, _g = formula_long_case(golden_dir)          # synthetic weights of manifest_ppformulanet_head_dec_long.json, its lm_head gains
    eng = RdEngine("ppformulanet_head").load_weights(st)
    return eng, st


def encoder_states(B, S):
    """Sequences 0 .. B - 1 of one pool per S, scaled like `formula_long_case`: image b is the same in every batch."""
    if S not in POOL:
        POOL[S] = (np.random.default_rng(1000 + S).standard_normal((33, S, 2048)) * 3.0).astype(np.float32)
    return POOL[S][:B]


def decode(eng, enc, max_new, trace):
    """(ids [B][n_cols] numpy, hidden [max_new][B][512], logits [max_new][B][V]) - the traces None without `trace`."""
    B, S, _ = enc.shape
    e = torch.from_numpy(enc).cuda()
    ids = torch.full((B, max_new + 1), -5, dtype=torch.int64, device="cuda")
    hid = torch.full((max_new, B, R.D), R.SENTINEL, device="cuda") if trace else None
    lg = torch.full((max_new, B, V), R.SENTINEL, device="cuda") if trace else None
    n = C.c_int32(0)
    rc = R.lib().rd_debug_formula_decode(eng._h, e.data_ptr(), B, S, max_new, ids.data_ptr(), C.byref(n), torch.cuda.current_stream().cuda_stream,
                                         R.ptr(lg), R.ptr(hid))
    assert rc == 0, eng._l.rd_last_error(eng._h).decode()
    torch.cuda.synchronize()
    return ids[:, :n.value].cpu().numpy(), (hid.cpu() if trace else None), (lg.cpu() if trace else None)


def traced_run(decoder, B, S, max_new):
    key = (B, S, max_new)
    if key in RUNS:
        return RUNS[key]
    run = decode(decoder[0], encoder_states(B, S), max_new, True)
    if key in ((1, 144, 36), (16, 144, 36)):                            # the two runs that two tests share
        RUNS[key] = run
    return run


def check_case(decoder, B, S, max_new):
    from test_oracle_golden import live_steps
    eng, st = decoder
    enc = encoder_states(B, S)
    ids, hid, lg = traced_run(decoder, B, S, max_new)
    n = ids.shape[1]
    steps = n - 1
    assert ids.shape[0] == B and 2 <= n <= max_new + 1 and (ids[:, 0] == 0).all() and ((ids >= 0) & (ids < V)).all()
    # the entry without traces is rd_formula_decode: same ids, same column count - and so is the product's own entry
    ids0, _, _ = decode(eng, enc, max_new, False)
    assert ids0.shape == ids.shape and (ids0 == ids).all()
    idp = eng.formula_decode(torch.from_numpy(enc).cuda(), max_new).cpu().numpy()
    assert idp.shape == ids.shape and (idp == ids).all()
    live = torch.from_numpy(live_steps(ids))                            # [B][steps]
    assert bool(live[:, 0].all())
    with torch.no_grad():
        hid64, lg64 = R.step_reference(st, enc, ids)
        hid32, lg32 = R.step_reference(st, enc, ids, torch.float32)
    tag = f"step B{B} S{S} {steps} steps ({int(live.sum())} live rows)"
    gh = hid[:steps].permute(1, 0, 2)                                   # [B][steps][512]
    gl = lg[:steps].permute(1, 0, 2)
    rh = R.bound_ratio(gh[live], hid64[live], hid32[live], tag + " hidden")
    yerr = float((lg32[live].double() - lg64[live]).abs().max())
    bound = 4.0 * yerr + 2.0 ** -22 * float(lg64[live].abs().max())
    rl = R.bound_ratio(gl[live], lg64[live], lg32[live], tag + " logits")
    # the token the GPU chose at every live step: in fp64 at most 2 x the bound below the row's maximum
    chosen = torch.gather(lg64, 2, torch.from_numpy(ids[:, 1:, None]))[..., 0]
    gap = (lg64.max(dim=2).values - chosen)[live]
    print(f"{tag}: chosen token below the fp64 maximum by at most {float(gap.max()):.3e} (2 x bound {2 * bound:.3e})")
    assert float(gap.max()) <= 2 * bound, (tag, float(gap.max()), bound)
    # steps the loop did not run stay unwritten (it looks for the end of all sequences every 8 steps, so it may run ahead to the next multiple)
    ran = min(max_new, (steps + 7) // 8 * 8)
    assert bool((hid[ran:] == R.SENTINEL).all()) and bool((lg[ran:] == R.SENTINEL).all())
    return rh, rl


@pytest.mark.parametrize("B", [1, 8, 9, 16, 17, 32])
def test_step_every_fused_batch_band(decoder, B):
    """S = 144, 36 steps: the self-attention's length passes 32 / 33 (one key group of the fused kernels' output loop)."""
    check_case(decoder, B, 144, 36)


def test_step_unfused_route_b33(decoder):
    check_case(decoder, 33, 5, 6)


def test_step_b16_three_encoder_tokens(decoder):
    check_case(decoder, 16, 3, 36)


def test_image_in_a_batch_of_16_equals_the_image_alone(decoder):
    """Image 0 decoded alone (B = 1: the M <= 8 kernels) and as row 0 of a batch of 16 (the M <= 16 kernels) differ by at most the bound
    (4 x the fp32 oracle's error against fp64 on the same ids + 2^-22 max|ref|) - on the steps up to the first differing token, if any.  The
    kernels are routed by B, so bit equality is not promised; whether it holds is printed (docs/notebook/formula_decode_kernels.md)."""
    eng, st = decoder
    ids1, hid1, lg1 = traced_run(decoder, 1, 144, 36)
    ids16, hid16, lg16 = traced_run(decoder, 16, 144, 36)
    n = min(ids1.shape[1], ids16.shape[1])
    diff = np.nonzero(ids1[0, :n] != ids16[0, :n])[0]
    steps = int(diff[0]) if len(diff) else n - 1                        # steps whose input prefix is the same
    assert steps >= 1
    pref = ids1[:, :steps + 1]
    with torch.no_grad():
        hid64, lg64 = R.step_reference(st, encoder_states(1, 144), pref)
        hid32, lg32 = R.step_reference(st, encoder_states(1, 144), pref, torch.float32)
    for name, a, b, r64, r32 in (("hidden", hid1, hid16, hid64, hid32), ("logits", lg1, lg16, lg64, lg32)):
        bound = 4.0 * float((r32.double() - r64).abs().max()) + 2.0 ** -22 * float(r64.abs().max())
        d = float((a[:steps, 0].double() - b[:steps, 0].double()).abs().max())
        print(f"image 0 alone vs in a batch of 16, {steps} steps, {name}: max difference {d:.3e} (bound {bound:.3e}), "
              f"bit-equal: {R.same_bits(a[:steps, 0], b[:steps, 0])}")
        assert d <= bound, (name, d, bound)
    print(f"ids equal over {n} columns: {len(diff) == 0}")
