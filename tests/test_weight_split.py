"""CPU: the host rules every prepare_*_weights function shares (csrc/rd_host.h), asked through the host-only developer entry
rd_debug_weight_split (no HIP call): the power-of-two exponent of the single-accumulator split (rd_pow2_exp), its (hi, lo) fp16 halves
(rd_split_scaled) and the halves of the three-product form (rd_split_2048), against a NumPy statement of the same rules - np.frexp for
the exponent, float64 products (exact for a power of two) rounded once to float32, np.float16 casts (round to nearest even) for the
halves.  Bits are compared, not values.  docs/notebook/launcher_host_helpers.md."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

N = 4096
CLAMP, NO_CLAMP = 100, 0


@pytest.fixture(scope="module")
def lib():
    """the library without the torch import of _lib.load(): nothing here touches the GPU"""
    from rapiddoc_amd import _lib, build as rd_build
    rd_build.build(verbose=False)       # (as tests/test_cabi.py: a no-op when the library is up to date)
    lib = C.CDLL(str(_lib.LIB_PATH))
    lib.rd_debug_weight_split.restype, lib.rd_debug_weight_split.argtypes = _lib.DEBUG_SYMBOLS["rd_debug_weight_split"]
    return lib


def _inputs():
    base = np.random.default_rng(20261019).normal(0.0, 0.05, N).astype(np.float32)
    big, tiny, inf = base.copy(), (base * np.float32(1e-30 / np.abs(base).max())).astype(np.float32), base.copy()
    big[1234] = 3e4
    inf[77] = np.inf
    # name -> (array, exponent with clamp 100, exponent without): 0.05 N(0, 1) over 4096 draws peaks in [2^-3, 2^-2); 2^14 <= 3e4 < 2^15;
    # 2^-100 <= 1e-30 < 2^-99
    return {"normal": (base, 16, 16), "zero": (np.zeros(N, np.float32), 0, 0), "one_large": (big, -1, -1), "tiny": (tiny, 100, 113),
            "one_inf": (inf, 0, 0)}


INPUTS = _inputs()


def _bits(a):
    return np.ascontiguousarray(a, np.float16).view(np.uint16)


def reference(w, clamp):
    """(exponent, scaled halves [n][2], h3 halves [n][2]) by the rule as the notebook states it"""
    mx = float(np.max(np.abs(w)))
    ex = 0
    if mx > 0 and np.isfinite(mx):
        ex = 14 - int(np.frexp(np.float32(mx))[1])          # mx = m 2^x, m in [0.5, 1)  ->  mx 2^(14 - x) in [2^13, 2^14)
        if clamp > 0:
            ex = max(-clamp, min(clamp, ex))
    with np.errstate(all="ignore"):
        vs = (w.astype(np.float64) * 2.0 ** ex).astype(np.float32)
        hi = vs.astype(np.float16)
        lo = (vs - hi.astype(np.float32)).astype(np.float16)
        hi3 = w.astype(np.float16)
        lo3 = ((w - hi3.astype(np.float32)) * np.float32(2048)).astype(np.float16)
    return ex, np.stack([_bits(hi), _bits(lo)], 1), np.stack([_bits(hi3), _bits(lo3)], 1)


def native(lib, w, clamp):
    scaled, h3 = np.full((w.size, 2), 0xA5A5, np.uint16), np.full((w.size, 2), 0xA5A5, np.uint16)
    ex = lib.rd_debug_weight_split(w.ctypes.data, w.size, clamp, scaled.ctypes.data, h3.ctypes.data)
    return ex, scaled, h3


@pytest.mark.parametrize("clamp", [CLAMP, NO_CLAMP], ids=["clamp100", "noclamp"])
@pytest.mark.parametrize("name", list(INPUTS))
def test_exponent_and_halves_are_the_numpy_rule_bit_for_bit(lib, name, clamp):
    w, ex_clamped, ex_free = INPUTS[name]
    assert w.dtype == np.float32 and w.size == N
    ex, scaled, h3 = native(lib, w, clamp)
    ref_ex, ref_scaled, ref_h3 = reference(w, clamp)
    assert ex == ref_ex == (ex_clamped if clamp else ex_free)
    assert np.array_equal(scaled, ref_scaled), np.flatnonzero((scaled != ref_scaled).any(1))[:8]
    assert np.array_equal(h3, ref_h3), np.flatnonzero((h3 != ref_h3).any(1))[:8]


def test_the_scaled_largest_weight_lands_in_2_13_to_2_14(lib):
    """what the exponent is for: hi of the largest |w| is in [2^13, 2^14) whenever the exponent is not clamped, all-zero or refused"""
    for name in ("normal", "one_large", "tiny"):
        w = INPUTS[name][0]
        _, scaled, _ = native(lib, w, NO_CLAMP)
        top = abs(float(scaled[np.argmax(np.abs(w)), 0:1].view(np.float16)[0]))
        assert 2.0 ** 13 <= top < 2.0 ** 14, (name, top)


def test_bad_arguments_are_refused(lib):
    w = INPUTS["normal"][0]
    out = np.zeros((N, 2), np.uint16)
    assert lib.rd_debug_weight_split(None, N, CLAMP, out.ctypes.data, out.ctypes.data) == -1000
    assert lib.rd_debug_weight_split(w.ctypes.data, 0, CLAMP, out.ctypes.data, out.ctypes.data) == -1000
    assert lib.rd_debug_weight_split(w.ctypes.data, N, CLAMP, None, out.ctypes.data) == -1000
    assert not out.any()
