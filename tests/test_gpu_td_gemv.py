"""GPU: `td_gemv_kernel` of csrc/table_decoder.hip alone against fp64, through the developer entry `rd_debug_td_gemv` (the launch function
of the decode step itself).  Every row count B = 1 .. 8 of the unrolled `if (b < B)`, at the step's five layer shapes; one loop trip (K = 256)
and column counts that are no multiple of the four wavefronts of a block (the `n >= N` return no product shape takes); bias and residual
present and absent.  The rows of `x` behind row B - 1 are NaN and the rows of `y` around the B written ones carry a sentinel.  The header's
claim "a (row, column) sum has the same order whatever B is" is asserted: row b of a B = 8 launch equals, bit for bit, the B = 1 launch of
that row alone.

Reference, yardstick and bound: tests/td_reference.py.  The measured ratios are in docs/notebook/table_decode_kernels.md."""
import pytest
import torch

import td_reference as R

pytestmark = pytest.mark.gpu

# the step's linears, K -> N: wo / cq / co, wqkv, linear1 (GELU), linear2 (+ residual), generator
LAYER_SHAPES = [(768, 768, R.ACT_NONE, False), (768, 2304, R.ACT_NONE, False), (768, 3072, R.ACT_GELU, False), (3072, 768, R.ACT_NONE, True),
                (768, 960, R.ACT_NONE, False)]
GUARD = 2
_CASES = {}


def operands(K, N, act, res):
    """x [8][K], w [N][K], bias [N], res [8][N] (host and device) and the fp64 / fp32 references of all 8 rows with and without bias and
    residual, once per shape"""
    key = (K, N, act, res)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 + K + 7 * N + act)
        c = dict(x=torch.randn((R.MAXB, K), generator=g), w=torch.randn((N, K), generator=g) / K ** 0.5, bias=0.1 * torch.randn(N, generator=g),
                 res=torch.randn((R.MAXB, N), generator=g))
        c["dev"] = {k: v.cuda() for k, v in c.items()}
        c["ref"] = {}
        _CASES[key] = c
    return _CASES[key]


def reference(c, act, bias, res):
    if (bias, res) not in c["ref"]:
        args = (c["x"], c["w"], c["bias"] if bias else None, act, c["res"] if res else None)
        c["ref"][(bias, res)] = (R.linear_reference(*args), R.linear_reference(*args, dtype=torch.float32))
    return c["ref"][(bias, res)]


def launch(c, B, K, N, act, bias, res, rows=None):
    """One launch on rows `rows` (default 0 .. B - 1) of the case; the rows of x behind them are NaN.  Returns y [B][N] on the CPU."""
    d = c["dev"]
    rows = list(range(B)) if rows is None else rows
    x = torch.full((R.MAXB, K), float("nan"), device="cuda")
    x[:B] = d["x"][rows]
    r = d["res"][rows].contiguous() if res else None
    y = torch.full((GUARD + B + GUARD, N), R.SENTINEL, device="cuda")
    rc = R.lib().rd_debug_td_gemv(B, K, N, act, x.data_ptr(), d["w"].data_ptr(), d["bias"].data_ptr() if bias else None, R.ptr(r), y[GUARD:].data_ptr())
    assert rc == 0, rc
    yc = y.cpu()
    assert bool((yc[:GUARD] == R.SENTINEL).all() and (yc[GUARD + B:] == R.SENTINEL).all()), "rows around the B written ones changed"
    return yc[GUARD:GUARD + B]


def check(B, K, N, act, bias, res):
    c = operands(K, N, act, res)
    y = launch(c, B, K, N, act, bias, res)
    ref, yard = reference(c, act, bias, res)
    return R.bound_ratio(y, ref[:B], yard[:B], f"td_gemv B{B} {K}->{N} act{act} bias{int(bias)} res{int(res)}")


@pytest.mark.parametrize("B", range(1, R.MAXB + 1))
def test_layer_shapes_at_every_row_count(B):
    for K, N, act, res in LAYER_SHAPES:
        check(B, K, N, act, True, res)


@pytest.mark.parametrize("N", [1, 5, 961])
def test_one_loop_trip_and_columns_that_do_not_fill_a_block(N):
    for B in (1, 5, 8):
        check(B, 256, N, R.ACT_NONE, True, True)
        check(B, 768, N, R.ACT_GELU, True, False)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("res", [False, True])
def test_bias_and_residual_present_and_absent(bias, res):
    for B in (1, 3, 8):
        check(B, 768, 768, R.ACT_NONE, bias, res)
        check(B, 256, 5, R.ACT_GELU, bias, res)


@pytest.mark.parametrize("shape", LAYER_SHAPES, ids=lambda s: f"{s[0]}to{s[1]}")
def test_row_b_of_eight_equals_the_row_alone_bit_for_bit(shape):
    K, N, act, res = shape
    c = operands(K, N, act, res)
    y8 = launch(c, 8, K, N, act, True, res)
    for b in range(R.MAXB):
        y1 = launch(c, 1, K, N, act, True, res, rows=[b])
        assert R.same_bits(y8[b:b + 1], y1), (shape, b)
    y3 = launch(c, 3, K, N, act, True, res, rows=[6, 0, 3])           # and in another place of another row count
    assert R.same_bits(y3, y8[[6, 0, 3]]), shape


def test_arguments_no_launch_can_take():
    f = R.lib().rd_debug_td_gemv
    x = torch.zeros((R.MAXB, 768), device="cuda")
    w = torch.zeros((8, 768), device="cuda")
    y = torch.full((R.MAXB + 1, 8), R.SENTINEL, device="cuda")
    px, pw, py = x.data_ptr(), w.data_ptr(), y.data_ptr()
    assert f(0, 768, 8, 0, px, pw, None, None, py) == -1
    assert f(9, 768, 8, 0, px, pw, None, None, py) == -1
    assert f(1, 0, 8, 0, px, pw, None, None, py) == -1
    assert f(1, -256, 8, 0, px, pw, None, None, py) == -1
    assert f(1, 700, 8, 0, px, pw, None, None, py) == -1              # K % 256
    assert f(1, 768, 0, 0, px, pw, None, None, py) == -1
    assert f(1, 768, 8, 0, None, pw, None, None, py) == -1
    assert f(1, 768, 8, 0, px, None, None, None, py) == -1
    assert f(1, 768, 8, 0, px, pw, None, None, None) == -1
    assert bool((y == R.SENTINEL).all())
    assert f(8, 768, 8, 0, px, pw, None, None, py) == 0
    assert bool((y[:8] == 0).all() and (y[8:] == R.SENTINEL).all())
