"""CPU: the C-ABI library builds, loads and exports every symbol include/rapiddoc_mi355.h declares; the two ctypes tables of
rapiddoc_amd/_lib.py agree with the C prototypes; the product path fails loudly (no CPU fallback) when there is no GPU."""
import ctypes as C
import os
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from rapiddoc_amd import build as rd_build
    rd_build.build(verbose=False)
    from rapiddoc_amd import _lib
    return _lib.load()


def test_header_symbols_are_exported(lib):
    header = (ROOT / "include" / "rapiddoc_mi355.h").read_text()
    declared = set(re.findall(r"\b(rd_[a-z0-9_]+)\s*\(", header))
    declared -= {"rd_handle", "rd_crop_desc", "rd_text_box", "rd_layout_post_cfg"}
    assert len(declared) >= 14
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    from rapiddoc_amd import _lib
    assert declared == set(_lib.SYMBOLS), (declared ^ set(_lib.SYMBOLS))


def test_debug_symbols_are_the_entries_api_debug_defines(lib):
    """the developer counterpart of test_header_symbols_are_exported: csrc/api_debug.cpp against _lib.DEBUG_SYMBOLS, by name"""
    from rapiddoc_amd import _lib
    defined = set(_debug_prototypes())
    assert len(defined) >= 30
    for name in sorted(defined):
        assert hasattr(lib, name), f"{name} defined in api_debug.cpp but not exported"
    assert defined == set(_lib.DEBUG_SYMBOLS), (defined ^ set(_lib.DEBUG_SYMBOLS))


# ---------------------------------------------------------------------------------------------------------------- tables against prototypes
def _is_int(size):
    return lambda t: isinstance(t, type) and issubclass(t, C._SimpleCData) and t._type_ in "bBhHiIlLqQ" and C.sizeof(t) == size


# a C type without `const` -> does this ctypes type (or None) stand for it?  Pointers and arrays are taken before the table is asked
C_TYPES = {"void": lambda t: t is None, "int": _is_int(4), "int32_t": _is_int(4), "unsigned": _is_int(4), "int64_t": _is_int(8), "long long": _is_int(8),
           "long": lambda t: t is C.c_long, "size_t": lambda t: t is C.c_size_t, "float": lambda t: t is C.c_float, "double": lambda t: t is C.c_double}


def _agrees(ctype, t):
    if "*" in ctype or "[" in ctype:
        return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))
    return C_TYPES[" ".join(w for w in ctype.split() if w != "const")](t)


def _prototypes(text, pattern):
    """name -> (return type, [parameter types]) of every `type name(parameters)` that `pattern` finds in `text`; a parameter's type is
    what is left of it without its name, an array parameter keeps its brackets"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    out = {}
    for m in re.finditer(pattern, text, flags=re.M):
        params = [p.strip() for p in m.group(3).split(",")]
        params = [] if params in ([""], ["void"]) else [re.sub(r"\w+(\s*\[\w*\])?$", r"\1", p).strip() for p in params]
        assert m.group(2) not in out, m.group(2)
        out[m.group(2)] = (m.group(1).strip(), params)
    return out


def _header_prototypes():
    return _prototypes((ROOT / "include" / "rapiddoc_mi355.h").read_text(), r"^([A-Za-z_][\w \*]*?[\s\*])(rd_\w+)\s*\(([^)]*)\)\s*;")


def _debug_prototypes():
    """the definitions of csrc/api_debug.cpp, up to the closing parenthesis (a static helper is no entry)"""
    return _prototypes((ROOT / "rapiddoc_amd" / "csrc" / "api_debug.cpp").read_text(), r"^(?!static\b)([A-Za-z_][\w \*]*?[\s\*])(rd_debug_\w+)\s*\(([^)]*)\)\s*\{")


def _mismatches(table, prototypes):
    out = []
    for name, (res, args) in table.items():
        cres, cparams = prototypes[name]
        if len(args) != len(cparams):
            out.append(f"{name}: {len(args)} argtypes, the prototype has {len(cparams)} parameters")
            continue
        for i, (ctype, t) in enumerate([(cres, res)] + list(zip(cparams, args))):
            if not _agrees(ctype, t):
                out.append(f"{name}: {'the return value' if i == 0 else f'parameter {i}'} is `{ctype}`, the table has {getattr(t, '__name__', t)}")
    return out


def test_both_tables_agree_with_the_c_prototypes():
    """Number of parameters, and class and size of each parameter and of the return value: SYMBOLS against the public header,
    DEBUG_SYMBOLS against the definitions in csrc/api_debug.cpp"""
    from rapiddoc_amd import _lib
    header, debug = _header_prototypes(), _debug_prototypes()
    assert set(header) == set(_lib.SYMBOLS) and set(debug) == set(_lib.DEBUG_SYMBOLS)
    assert header["rd_preproc_resize_norm"][1][6] == "const float [3]" and header["rd_create"] == ("rd_handle*", ["int", "const char*"])
    assert debug["rd_debug_dec_attention"][1][7] == "long long" and len(debug["rd_debug_mbv3s_block"][1]) == 27      # definitions that span lines
    assert _mismatches(_lib.SYMBOLS, header) == []
    assert _mismatches(_lib.DEBUG_SYMBOLS, debug) == []


def test_the_prototype_comparison_reports_a_wrong_row():
    from rapiddoc_amd import _lib
    debug = _debug_prototypes()
    res, args = _lib.DEBUG_SYMBOLS["rd_debug_conv"]
    assert _mismatches({"rd_debug_conv": (res, args)}, debug) == []
    assert _mismatches({"rd_debug_conv": (res, args[1:])}, debug) == ["rd_debug_conv: 21 argtypes, the prototype has 22 parameters"]       # one c_int fewer
    assert _mismatches({"rd_debug_conv": (res, args[:14] + [C.c_float] + args[15:])}, debug) == ["rd_debug_conv: parameter 15 is `float*`, the table has c_float"]
    assert _mismatches({"rd_debug_conv": (C.c_int, args)}, debug) == ["rd_debug_conv: the return value is `float`, the table has c_int"]
    assert _mismatches({"rd_debug_derived_tensor": (C.c_int, _lib.DEBUG_SYMBOLS["rd_debug_derived_tensor"][1])}, debug)                     # a 4-byte `long`


def test_version_and_seq_len(lib):
    assert b"gfx950" in lib.rd_version()
    from rapiddoc_amd import ocr_host
    for w in (15, 16, 17, 96, 320, 321, 327, 1157, 2112):
        assert lib.rd_rec_seq_len(w) == ocr_host.rec_seq_len(w)
    assert lib.rd_rec_seq_len(320) == 40


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_gpu_fails_loudly(lib):
    h = lib.rd_create(0, b"ppocrv6_det")
    assert not h
    assert b"no HIP device" in lib.rd_create_error()
    from rapiddoc_amd.engine import EngineError, RdEngine
    with pytest.raises(EngineError):
        RdEngine("ppocrv6_det")


def test_crop_desc_layout_matches_header():
    from rapiddoc_amd.pipeline import CROP_DTYPE, CropDesc
    assert C.sizeof(CropDesc) == 60 == CROP_DTYPE.itemsize  # 15 x 4-byte fields, see rd_crop_desc


def test_product_package_never_imports_oracle():
    for py in (ROOT / "rapiddoc_amd").rglob("*.py"):
        src = py.read_text()
        assert "import oracle" not in src and "from oracle" not in src, py


def test_importing_the_package_defaults_the_hardware_queue_count_and_respects_an_explicit_one():
    """`import rapiddoc_amd` gives every HIP stream its own hardware queue unless the environment says otherwise (with
    the runtime's default of four, streams that share a queue serialise - 7-15 % of a step)."""
    import subprocess
    import sys
    root = str(Path(__file__).resolve().parents[1])
    code = "import os, sys; sys.path.insert(0, %r); import rapiddoc_amd; print(os.environ['GPU_MAX_HW_QUEUES'])" % root
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    assert subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True).stdout.strip() == "16"
    env["GPU_MAX_HW_QUEUES"] = "4"
    assert subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True).stdout.strip() == "4"
    # the override is a side effect on the embedding process: it is logged once (INFO, logger "rapiddoc_amd") and can be asked for
    code2 = ("import logging, os, sys; logging.basicConfig(level=logging.INFO, stream=sys.stdout, format='%%(name)s|%%(message)s'); "
             "sys.path.insert(0, %r); import rapiddoc_amd; print(rapiddoc_amd.HW_QUEUES_SET_BY_IMPORT)" % root)
    del env["GPU_MAX_HW_QUEUES"]
    out = subprocess.run([sys.executable, "-c", code2], env=env, capture_output=True, text=True).stdout
    assert out.count("rapiddoc_amd|rapiddoc_amd: GPU_MAX_HW_QUEUES was unset") == 1 and out.strip().endswith("True")
    env["GPU_MAX_HW_QUEUES"] = "8"
    out = subprocess.run([sys.executable, "-c", code2], env=env, capture_output=True, text=True).stdout
    assert "GPU_MAX_HW_QUEUES" not in out and out.strip().endswith("False")
