"""Shared by tests/test_gpu_dw_register.py, test_gpu_se_chain.py and test_gpu_glue_ops.py (the HBM-bound operators of csrc/kernels_misc.hip
through their developer entries): strided views inside sentinel-filled device buffers, and the two error rules of those files."""
import torch

SENTINEL = -777.25
U = 2.0 ** -24          # the unit round-off of fp32


def lib():
    from rapiddoc_amd import _lib
    return _lib.load()


class View:
    """`rows` x `c` floats at channel offset `off` of a device buffer [guard + rows + guard][ld]: a channel slot of a wider map with guard
    rows in front and behind.  Everything but the view holds SENTINEL; the view holds `data` ([rows][c] on the CPU), or NaN (an output)."""

    def __init__(self, rows, c, ld=None, off=0, data=None, guard=3):
        ld = c if ld is None else ld
        assert off + c <= ld
        self.rows, self.c, self.ld, self.off, self.guard = rows, c, ld, off, guard
        self.buf = torch.full((rows + 2 * guard, ld), SENTINEL, device="cuda")
        own = self.buf[guard:guard + rows, off:off + c]
        if data is None:
            own.fill_(float("nan"))
        else:
            own.copy_(data.reshape(rows, c).to(torch.float32))
        self.before = self.buf.clone()

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * (self.guard * self.ld + self.off)

    def owned(self):
        """the view's contents now, [rows][c] on the CPU"""
        return self.buf[self.guard:self.guard + self.rows, self.off:self.off + self.c].cpu()

    def assert_outside_untouched(self, tag, owned_rows=None):
        """everything outside the view (with owned_rows, a bool [rows]: outside those rows of it) is bit-identical to the sentinel"""
        b = self.buf.clone()
        own = b[self.guard:self.guard + self.rows, self.off:self.off + self.c]
        if owned_rows is None:
            own.fill_(SENTINEL)
        else:
            own[owned_rows.to(own.device)] = SENTINEL
        bad = b.view(torch.int32) != torch.full_like(b, SENTINEL).view(torch.int32)
        assert not bool(bad.any()), (tag, "stores outside the view at (row, column)", bad.nonzero()[:8].tolist())

    def assert_unchanged(self, tag):
        """an input: the whole buffer is bit-identical to what it held before the launch"""
        assert torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32)), (tag, "an input buffer was written")


def check_linear(got, ref, mag, terms, tag):
    """The bound of a linear kernel in fp32, any summation or FMA order: |got - ref| <= terms * 2^-24 * mag elementwise, mag = the sum of the
    absolute values of the terms of ref (fp64).  Returns the largest error / bound."""
    assert bool(torch.isfinite(got).all()), (tag, "not finite")
    err = (got.double() - ref).abs()
    bound = terms * U * mag
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{tag}: max err {float(err.max()):.3e} max bound {float(bound.max()):.3e} worst err/bound {ratio:.3f}")
    assert bool((err <= bound).all()), (tag, float(err.max()), ratio)
    return ratio


def check_yardstick(got, ref, yard, tag):
    """The rule of tests/test_gpu_attention.py for a nonlinear kernel: `yard` is the same formula in plain fp32 on the CPU; the kernel's max-abs
    error against fp64 may be at most 4 x the yardstick's plus 4 * 2^-24 * max|ref|.  Returns error / bound."""
    assert bool(torch.isfinite(got).all()), (tag, "not finite")
    err = float((got.double() - ref).abs().max())
    yerr = float((yard.double() - ref).abs().max())
    bound = 4.0 * yerr + 4.0 * U * float(ref.abs().max())
    print(f"{tag}: err {err:.3e} fp32 yardstick {yerr:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert err <= bound, (tag, err, yerr, bound)
    return err / bound
