"""GPU: the decode step's weight-streaming linears (`dec_gemv_kernel` of csrc/formula_decoder.hip) alone against fp64, through the developer
entry `rd_debug_dec_gemv` - the decode step's own routing (`dec_gemv_route`), the product's instantiations.  Every batch band (M <= 8, <= 16,
<= 32), the layer shapes of the step (512 -> 512 / 1536 / 2048, 2048 -> 512), the wide loop (512 -> 50 000), the clamped columns of a
four- and a two-column group (N = 4099 / 50 001), LayerNorm in front (rows of mean 100 and unit deviation), GELU, residual; which
instantiation ran; nothing written outside [M][N]; the direct-X kernel when a wavefront takes a second column group (K = 2048, N = 4100).

Reference, yardstick and bound: tests/dec_reference.py.  The measured ratios are in docs/notebook/formula_decode_kernels.md."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import dec_reference as R

pytestmark = pytest.mark.gpu

GUARD = 3          # rows of sentinel in front of and behind y (y is dense, ld = N: a column overrun lands in the next row or in the guard)


DIRECT_X = os.environ.get("RD_DEC_GEMV_DX", "1")[:1] != "0"        # the library's A/B knob, read once per process: 0 stages X through LDS


def expected_route(M, K, N, ln):
    """MT * 10000 + CW * 1000 + KPL * 100 + DB * 10 + DX of the instantiation the step uses, 0 = the step falls back to the skinny GEMM."""
    if K == 2048:
        if ln or M > 16:
            return 0
        return (81801 if DIRECT_X else 81800) if M <= 8 else 161800
    wide = N > 4096
    if M <= 8:
        return 84210 if wide else (81200 if ln or not DIRECT_X else 81201)
    if M <= 16:
        return 162210 if wide else 161200
    return 321210 if wide else 321200


@functools.lru_cache(maxsize=2)
def weights(K, N):
    """(w, bias, ln_g, ln_b) on the CPU and on the GPU, shared by the cases of a shape."""
    g = torch.Generator().manual_seed(K * 131 + N)
    w = torch.randn((N, K), generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g)
    ln_g = 1.0 + 0.1 * torch.randn(K, generator=g)
    ln_b = 0.1 * torch.randn(K, generator=g)
    cpu = (w, bias, ln_g, ln_b)
    return cpu, tuple(t.cuda() for t in cpu)


def run(M, K, N, ln, act, res, bias=True, seed=0):
    """One launch into a sentinel-framed y.  Returns (route code, y [M][N] on the CPU, frame untouched, x, res)."""
    (w, b, lg, lb), (wd, bd, lgd, lbd) = weights(K, N)
    g = torch.Generator().manual_seed(seed + M)
    x = torch.randn((M, K), generator=g)
    if ln:
        x = x + 100.0                                   # rows of mean 100, unit deviation
    r = torch.randn((M, N), generator=g) if res else None
    y = torch.full(((M + 2 * GUARD) * N,), R.SENTINEL, device="cuda")
    xd = x.cuda()
    rd = r.cuda() if res else None
    yv = y[GUARD * N:]
    code = R.lib().rd_debug_dec_gemv(M, K, N, act, xd.data_ptr(), wd.data_ptr(), bd.data_ptr() if bias else None, lgd.data_ptr() if ln else None,
                                     lbd.data_ptr() if ln else None, R.ptr(rd), yv.data_ptr())
    yc = y.cpu()
    frame_ok = bool((yc[:GUARD * N] == R.SENTINEL).all() and (yc[(GUARD + M) * N:] == R.SENTINEL).all())
    return code, yc[GUARD * N:(GUARD + M) * N].reshape(M, N), frame_ok, x, r


def check(M, K, N, ln, act, res, bias=True):
    code, y, frame_ok, x, r = run(M, K, N, ln, act, res, bias)
    want = expected_route(M, K, N, ln)
    tag = f"gemv M{M} K{K} N{N} ln{int(ln)} act{act} res{int(res)} bias{int(bias)} route {code}"
    assert code == want, (tag, want)
    assert frame_ok, tag
    if code == 0:                                       # declined: nothing launched, nothing written
        assert bool((y == R.SENTINEL).all()), tag
        print(tag + ": declined")
        return None
    (w, b, lg, lb), _ = weights(K, N)
    args = (x, w, b if bias else None, (lg, lb) if ln else None, act, r)
    return R.bound_ratio(y, R.linear_reference(*args), R.linear_reference(*args, dtype=torch.float32), tag)


MS = [1, 3, 8, 9, 16, 17, 32]
# (LayerNorm in front, activation, residual): the step's own combinations first (so / co: residual; fc1: LN + GELU; q | k | v: LN), then the rest
FLAGS = [(False, R.ACT_NONE, True), (True, R.ACT_GELU, False), (True, R.ACT_NONE, False), (False, R.ACT_GELU, False), (True, R.ACT_GELU, True),
         (False, R.ACT_NONE, False)]


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("KN", [(512, 512), (512, 1536), (512, 2048), (2048, 512)], ids=lambda kn: "%dx%d" % kn)
def test_step_shapes(KN, M):
    K, N = KN
    for ln, act, res in FLAGS:
        check(M, K, N, ln, act, res)
    check(M, K, N, False, R.ACT_NONE, True, bias=False)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", [50000, 50001, 4099])
def test_wide_loop_and_column_tail(N, M):
    """N > 4096: the double-buffered loop over column groups (lm_head: LayerNorm in front, no bias in the product - both forms here); 4099 and
    50 001 leave one live column in the last group of four / two, the others are computed on a clamped column and must not be stored."""
    check(M, 512, N, True, R.ACT_NONE, False, bias=False)
    check(M, 512, N, False, R.ACT_GELU, True)


@pytest.mark.parametrize("M", [5, 8, 9, 16])
def test_direct_x_second_column_group(M):
    """K = 2048 with more column groups than wavefronts (N = 4100: 1024 workgroups x 4 wavefronts take 4096, wavefronts 0 .. 3 take a second
    one).  At M <= 8 the direct-X kernel holds four X rows at a time; the second group must start again at rows 0 .. 3."""
    assert check(M, 2048, 4100, False, R.ACT_NONE, True) is not None
    check(M, 2048, 4100, False, R.ACT_GELU, False)


def test_declined_shapes_launch_nothing():
    for M, K, N, ln in [(17, 2048, 512, False), (32, 2048, 512, False), (4, 2048, 512, True), (16, 2048, 512, True), (33, 512, 512, False),
                        (4, 1024, 512, False), (4, 256, 512, False), (0, 512, 512, False)]:
        (w, b, lg, lb), (wd, bd, lgd, lbd) = weights(2048, 512) if K == 2048 else weights(512, 512)
        rows = max(M, 1)
        x = torch.zeros((rows, max(K, 2048)), device="cuda")
        y = torch.full((rows + 2, 512), R.SENTINEL, device="cuda")
        code = R.lib().rd_debug_dec_gemv(M, K, N, 0, x.data_ptr(), wd.data_ptr(), bd.data_ptr(), lgd.data_ptr() if ln else None,
                                         lbd.data_ptr() if ln else None, None, y.data_ptr())
        assert code == 0 and bool((y == R.SENTINEL).all()), (M, K, N, ln, code)
    # arguments no launch can take
    assert R.lib().rd_debug_dec_gemv(4, 512, 512, 0, None, wd.data_ptr(), None, None, None, None, y.data_ptr()) == -1
    assert R.lib().rd_debug_dec_gemv(4, 512, 512, 0, x.data_ptr(), wd.data_ptr(), None, lgd.data_ptr(), None, None, y.data_ptr()) == -1


_STAGED_X_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import dec_reference as R
import test_gpu_dec_gemv as T
assert not T.DIRECT_X
for M in (1, 3, 8):
    for K, N in ((2048, 512), (512, 512), (512, 2048)):
        assert T.check(M, K, N, False, R.ACT_NONE, True) is not None
        T.check(M, K, N, False, R.ACT_GELU, False, bias=False)
T.check(5, 2048, 4100, False, R.ACT_NONE, True)
print("staged-x child done")
"""


def test_staged_x_instantiations_in_a_child_process():
    """`RD_DEC_GEMV_DX=0` (read once per process) routes the M <= 8 linears without LayerNorm to the instantiations that stage X through LDS:
    `<8,1,8,false,false>` (K = 2048) and `<8,1,2,false,false>` (K = 512).  A child process with the knob set runs them against fp64 under
    the same bound, the second-column-group shape included."""
    here = Path(__file__).resolve().parent
    env = dict(os.environ, RD_DEC_GEMV_DX="0")
    r = subprocess.run([sys.executable, "-c", _STAGED_X_CHILD, str(here.parent), str(here)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "staged-x child done" in r.stdout          # (the child's own `code == want` assertions pin the routes: DIRECT_X is false there)
