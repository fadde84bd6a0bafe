"""CPU: every engine kind of `engine.KINDS` is registered in the library's model table (csrc/models.cpp, `find_model`).  Engine's
constructor looks the kind up before it looks for a device, so on a machine without a GPU `rd_create` of a registered kind fails with the
device error, never with "unknown model kind"."""
import pytest

from rapiddoc_amd import engine

DECODER_KINDS = ("ppformulanet_head", "unitable_decoder")      # not Engines: rd_create takes them without the table
ENGINE_KINDS = tuple(k for k in engine.KINDS if k not in DECODER_KINDS)


@pytest.fixture(scope="module")
def lib():
    from rapiddoc_amd import _lib, build as rd_build
    rd_build.build(verbose=False)
    return _lib.load()


def test_there_are_twelve_engine_kinds():
    assert len(ENGINE_KINDS) == 12 and set(DECODER_KINDS) <= set(engine.KINDS)


@pytest.mark.parametrize("kind", ENGINE_KINDS)
def test_every_engine_kind_is_registered(lib, kind):
    h = lib.rd_create(0, kind.encode())
    if h:
        lib.rd_destroy(h)
    else:
        assert b"unknown model kind" not in lib.rd_create_error(), lib.rd_create_error()


def test_an_unknown_kind_is_named_as_unknown(lib):
    assert not lib.rd_create(0, b"bogus")
    assert b"unknown model kind 'bogus'" in lib.rd_create_error()
