"""GPU: `layernorm_kernel` (csrc/kernels_misc.hip, one wavefront per row, up to 8 elements per lane) alone against fp64 through the
developer entry `rd_debug_layernorm`: widths where lanes hold unequal element counts (the recogniser's C = 120: 56 lanes hold two, 8 hold
one), one element, the 512 limit, row counts around the 4 rows of a workgroup, row strides wider than the tensor, both eps of the product.

Reference: fp64 `layer_norm`.  Yardstick: torch's fp32 `layer_norm` on the same inputs; the kernel's max-abs error against fp64 may be at
most 4 x the yardstick's + 2^-22 max|ref|.  Measured ratios: docs/notebook/rec_tail_kernels.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
WIDTHS = [1, 15, 64, 120, 121, 256, 511, 512]


def _lib():
    from rapiddoc_amd import _lib
    return _lib.load()


def _launch(x, Cn, g, b, eps, yld):
    """x [M][xld] on the CPU; returns y [M + 2][yld] (sentinel-filled: 2 guard rows, yld - C guard columns) on the CPU."""
    M, xld = x.shape
    xd, gd, bd = x.cuda(), g.cuda(), b.cuda()
    y = torch.full((M + 2, yld), SENTINEL, device="cuda")
    assert _lib().rd_debug_layernorm(M, Cn, xd.data_ptr(), xld, y.data_ptr(), yld, gd.data_ptr(), bd.data_ptr(), eps) == 0
    return y.cpu()


def _check(x, Cn, g, b, eps, yld, tag):
    M = x.shape[0]
    y = _launch(x, Cn, g, b, eps, yld)
    assert bool((y[M:] == SENTINEL).all()) and bool((y[:, Cn:] == SENTINEL).all()), tag      # guard rows and columns untouched
    ref = torch.nn.functional.layer_norm(x[:, :Cn].double(), (Cn,), g.double(), b.double(), eps)
    yard = torch.nn.functional.layer_norm(x[:, :Cn].contiguous(), (Cn,), g, b, eps)
    err = float((y[:M, :Cn].double() - ref).abs().max())
    yerr = float((yard.double() - ref).abs().max())
    bound = 4.0 * yerr + 2.0 ** -22 * float(ref.abs().max())
    print(f"layernorm {tag}: err {err:.3e} fp32 yardstick {yerr:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert err <= bound, (tag, err, yerr, bound)


def _inputs(M, Cn, xld, seed, mean=0.0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((M, xld), generator=gen) + mean
    x[:, Cn:] = 1.0e6                                            # columns past C belong to a neighbour: never read into the statistics
    g = torch.rand(Cn, generator=gen) + 0.5
    b = torch.randn(Cn, generator=gen)
    return x, g, b


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("wide", [False, True], ids=["packed", "strided"])
@pytest.mark.parametrize("Cn", WIDTHS)
def test_matches_fp64_at_every_width(Cn, wide, eps):
    for M in (1, 3, 4, 5):
        xld, yld = (Cn + 8, Cn + 5) if wide else (Cn, Cn)
        x, g, b = _inputs(M, Cn, xld, 100 * Cn + M)
        _check(x, Cn, g, b, eps, yld, f"C{Cn} M{M} xld{xld} yld{yld} eps{eps:g}")


@pytest.mark.parametrize("Cn", [15, 120, 121, 512])
def test_many_rows(Cn):
    x, g, b = _inputs(1000, Cn, Cn + 4, Cn)
    _check(x, Cn, g, b, 1e-6, Cn + 1, f"C{Cn} M1000")


@pytest.mark.parametrize("Cn", [15, 120, 511])
def test_rows_with_mean_100_and_unit_deviation(Cn):
    """The two-pass form subtracts the mean before squaring: no cancellation at |mean| / std = 100."""
    x, g, b = _inputs(5, Cn, Cn, 7 + Cn, mean=100.0)
    _check(x, Cn, g, b, 1e-6, Cn, f"C{Cn} mean 100")


@pytest.mark.parametrize("Cn", [1, 64, 120, 512])
def test_constant_row_gives_the_bias_exactly(Cn):
    """A row of one repeated value that sums exactly (2.5 C is exact for C <= 512): mean = value, every deviation is 0, y = g 0 + b = b."""
    _x, g, b = _inputs(3, Cn, Cn, 3)
    x = torch.full((3, Cn), 2.5)
    x[1] = -0.375
    y = _launch(x, Cn, g, b, 1e-6, Cn)
    assert torch.equal(y[:3], b.expand(3, Cn))


def test_width_beyond_the_register_file_is_refused():
    x = torch.zeros((2, 513), device="cuda")
    y = torch.zeros((2, 513), device="cuda")
    g = torch.ones(513, device="cuda")
    lib = _lib()
    assert lib.rd_debug_layernorm(2, 513, x.data_ptr(), 513, y.data_ptr(), 513, g.data_ptr(), g.data_ptr(), 1e-6) == -1
    assert lib.rd_debug_layernorm(2, 512, x.data_ptr(), 513, y.data_ptr(), 513, g.data_ptr(), g.data_ptr(), 1e-6) == 0
