"""GPU: the whole decode step of the UniTable decoder (csrc/table_decoder.hip) against fp64 at every row count and across the length edges.
`rd_debug_table_decode` with forced tokens runs the step's launch chain (graph replay included) and traces the hidden row after each of the
four blocks and the logits of every step; the reference is `unitable_reference.decoder_forward` on the same memory and tokens in fp64, the
yardstick the same in fp32 on the CPU, the bound tests/td_reference.py's (4 x the yardstick's error + 2^-22 max|ref|).

  rows   B = 1 .. 8 (a memory and a token list per table), S = 39, 70 steps
  long   B = 2, S = 3, 1024 steps: cache row and position row 1023, the last step's guards, self lengths 255 .. 257 and 511 .. 513 on the way
  wide   B = 1, S = 1024 (the LDS score array full in the cross form), 8 steps
  stream N = 5 tables through 2 slots of `rd_debug_table_decode_stream`, S = 39, EOS raised so that the lengths differ: every live (table,
         position) against fp64 on the ids the stream itself produced - a numeric anchor of its own, not only equality with the batch path

The token the step chose equals `whitelist_argmax` of the fp64 logits wherever the fp64 top-2 whitelist gap exceeds twice the logits' bound;
at most 5 % of a case's steps may be left out by that rule.  The seeds below keep the share there for the fp64 reference and the yardstick
alone (`excluded_share`, checked on the CPU; seeds and shares in docs/notebook/table_decode_kernels.md)."""
import ctypes as C

import numpy as np
import pytest
import torch

import td_reference as R
import unitable_reference as U
from rapiddoc_amd import table_unitable as TU
from rapiddoc_amd import weights as W

pytestmark = pytest.mark.gpu

IDS = TU.STAND_IN_IDS
CASES = {"rows": dict(B=8, S=39, steps=70, seed=1), "long": dict(B=2, S=3, steps=1024, seed=2), "wide": dict(B=1, S=1024, steps=8, seed=3)}
STREAM = dict(N=5, S=39, max_new=48, slots=2, seed=40, eos_bias=5.0)
MAX_EXCLUDED = 0.05
_REF, _ENG = {}, {}


def case_inputs(name):
    """(memory [B][S][768], forced tokens int32 [B][steps]): table b is the same whatever the row count"""
    c = CASES[name]
    return W.synth_memory(c["seed"], c["B"], c["S"]), R.forced_tokens(c["seed"], c["B"], c["steps"], IDS)


def reference(golden_dir, name):
    """(hidden64 [B][steps][4][768], logits64 [B][steps][960], hidden32, logits32) of a case, computed once and left unchanged"""
    if name not in _REF:
        torch.set_num_threads(8)
        mem, toks = case_inputs(name)
        st = U.dec_state(golden_dir)
        _REF[name] = R.step_reference(st, mem, toks) + R.step_reference(st, mem, toks, torch.float32)
    return _REF[name]


def logits_bound(lg64, lg32):
    return 4.0 * float((lg32.double() - lg64).abs().max()) + 2.0 ** -22 * float(lg64.abs().max())


def decided(lg64, lg32):
    """bool [B][steps]: the fp64 top-2 whitelist gap exceeds twice the logits' bound"""
    bound = logits_bound(lg64, lg32)
    return np.stack([R.whitelist_gap(z.numpy()) for z in lg64]) > 2.0 * bound


def excluded_share(golden_dir, name, B=None):
    """Share of a case's steps the chosen-token rule leaves out - a property of the reference and the yardstick alone"""
    _, lg64, _, lg32 = reference(golden_dir, name)
    B = lg64.shape[0] if B is None else B
    return 1.0 - float(decided(lg64[:B], lg32[:B]).mean())


def engine(golden_dir, eos_bias=0.0):
    if eos_bias not in _ENG:
        from rapiddoc_amd.engine import RdEngine
        _ENG[eos_bias] = RdEngine(U.DEC_KIND).load_weights(stream_state(golden_dir, eos_bias))
    return _ENG[eos_bias]


def stream_state(golden_dir, eos_bias):
    st = U.dec_state(golden_dir)
    if eos_bias:
        st = dict(st)
        b = st["generator.bias"].copy()
        b[IDS.eos] += np.float32(eos_bias)
        st["generator.bias"] = b
    return st


def compare(tag, hid, lg, hid64, lg64, hid32, lg32):
    """hid [..][4][768], lg [..][960] of the GPU against the references of the same shapes; returns the worst ratio"""
    worst = 0.0
    for l in range(4):
        worst = max(worst, R.bound_ratio(hid[..., l, :], hid64[..., l, :], hid32[..., l, :], f"{tag} hidden after block {l}"))
    return max(worst, R.bound_ratio(lg, lg64, lg32, f"{tag} logits"))


def check_case(golden_dir, name, B):
    c = CASES[name]
    mem, toks = case_inputs(name)
    hid64, lg64, hid32, lg32 = (t[:B] for t in reference(golden_dir, name))
    out = engine(golden_dir).table_decode_debug(torch.from_numpy(mem[:B].copy()), IDS, c["steps"], forced=torch.from_numpy(toks[:B].copy()))
    torch.cuda.synchronize()
    tag = f"td_step {name} B{B} S{c['S']} {c['steps']} steps"
    hid = out["hidden"].permute(2, 0, 1, 3).cpu()                        # [B][steps][4][768]
    lg = out["logits"].permute(1, 0, 2).cpu()                            # [B][steps][960]
    worst = compare(tag, hid, lg, hid64, lg64, hid32, lg32)
    ok = decided(lg64, lg32)
    share = 1.0 - float(ok.mean())
    want = np.stack([U.whitelist_argmax(z.numpy()) for z in lg64])
    chosen = out["chosen"].cpu().numpy().T                               # [B][steps]
    print(f"{tag}: chosen token compared at {int(ok.sum())} of {ok.size} steps (left out {share:.4f}), worst ratio {worst:.3f}")
    assert share <= MAX_EXCLUDED, (tag, share)
    assert np.array_equal(chosen[ok], want[ok]), (tag, np.argwhere(ok & (chosen != want))[:8])
    assert bool(((chosen >= 0) & (chosen < R.VOCAB)).all())
    return worst


@pytest.mark.parametrize("B", range(1, R.MAXB + 1))
def test_step_at_every_row_count(golden_dir, B):
    check_case(golden_dir, "rows", B)


def test_step_over_1024_positions(golden_dir):
    check_case(golden_dir, "long", 2)


def test_step_over_1024_memory_rows(golden_dir):
    check_case(golden_dir, "wide", 1)


def test_stream_path_against_fp64(golden_dir):
    from rapiddoc_amd.engine import TableStreamStats
    s = STREAM
    N, S, max_new = s["N"], s["S"], s["max_new"]
    st = stream_state(golden_dir, s["eos_bias"])
    eng = engine(golden_dir, s["eos_bias"])
    mem = W.synth_memory(s["seed"], N, S)
    m = torch.from_numpy(mem).cuda()
    ids = torch.full((N, max_new + 1), -5, dtype=torch.int64, device="cuda")
    lens = torch.full((N,), -5, dtype=torch.int32, device="cuda")
    lg = torch.full((N, max_new, R.VOCAB), R.SENTINEL, device="cuda")
    hid = torch.full((N, max_new, 4, R.D), R.SENTINEL, device="cuda")
    stats, cfg = TableStreamStats(), TU.cfg_struct(IDS)
    torch.cuda.synchronize()
    rc = R.lib().rd_debug_table_decode_stream(eng._h, m.data_ptr(), N, S, max_new, s["slots"], C.byref(cfg), ids.data_ptr(), lens.data_ptr(),
                                              C.byref(stats), torch.cuda.current_stream().cuda_stream, lg.data_ptr(), hid.data_ptr(), None, 0)
    torch.cuda.synchronize()
    assert rc == 0, eng._l.rd_last_error(eng._h).decode()
    ids, lens, lg, hid = ids.cpu().numpy(), lens.cpu().numpy(), lg.cpu(), hid.cpu()
    assert len(set(lens.tolist())) >= 3 and lens.min() >= 2 and lens.max() <= max_new + 1, lens      # the precondition: lengths differ
    assert stats.live_slot_steps == int((lens - 1).sum())
    worst = 0.0
    for i in range(N):
        n = int(lens[i]) - 1                                             # live positions of table i; fed: the prefix and all but its last token
        toks = ids[i:i + 1, :n]
        h64, l64 = R.step_reference(st, mem[i:i + 1], toks)
        h32, l32 = R.step_reference(st, mem[i:i + 1], toks, torch.float32)
        worst = max(worst, compare(f"td_step stream table {i} ({n} positions)", hid[i:i + 1, :n], lg[i:i + 1, :n], h64, l64, h32, l32))
        assert bool((lg[i, n:] == R.SENTINEL).all() and (hid[i, n:] == R.SENTINEL).all()), "a position no table reached was written"
        # the emitted token: in fp64 at most twice the logits' bound below the best whitelisted logit (bbox overflow aside)
        bound = logits_bound(l64, l32)
        z = l64[0].numpy()
        for t in range(n):
            e = int(ids[i, t + 1])
            if e != IDS.bbox_close:
                assert e in U.WHITE and z[t, U.WHITE].max() - z[t, e] <= 2.0 * bound, (i, t, e)
    print(f"td_step stream N{N} S{S} slots {s['slots']}: lens {lens.tolist()}, worst ratio {worst:.3f}")
