"""CPU: `rd_ctc_rows_text` (the rows of the device CTC collapse -> strings and confidences, all lines in one library call) returns
exactly what `parse_ctc_rows` + `format_score` return row by row."""
import importlib.util
from pathlib import Path

import numpy as np

from rapiddoc_amd import ocr_host as H

ROOT = Path(__file__).resolve().parents[1]
_spec = importlib.util.spec_from_file_location("host_boundary", ROOT / "tools" / "host_boundary.py")
hb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(hb)


def assert_same(rows):
    want = H.parse_ctc_rows(rows)
    texts, conf, conf3 = H.parse_ctc_rows_native(rows)
    assert texts == [t for t, _s in want]
    assert all(type(c) is float for c in conf + conf3)
    assert np.array(conf).tobytes() == np.array([s for _t, s in want]).tobytes()
    assert np.array(conf3).tobytes() == np.array([H.format_score(s) for _t, s in want]).tobytes()
    return texts, conf, conf3


def test_texts_of_every_byte_length():
    """Empty lines, ASCII, and 2- / 3- / 4-byte characters: the dictionary the pipeline serves without a dictionary file is the CJK
    block from U+4E00 (3 bytes); Latin-1, Greek and Cyrillic letters (2 bytes) are what the multilingual PP-OCR dictionaries add."""
    chars = H.build_characters([chr(0x4E00 + i) + "\n" for i in range(300)] + list("éñßΩλяж") + ["a", "Z", "0", "~", "𠀀"])
    tab, max_len = H.char_table(chars)
    assert max_len == 5 and {int(v) for v in tab[1:, 0]} == {1, 2, 3, 4}          # ("blank" itself, 5 bytes, is never emitted)
    rng = np.random.default_rng(3)
    texts = ["", "a", "plain ASCII line 0123~", "é", "ñandú Ωλ яж", "一丁七", "𠀀a𠀀", ""]
    texts += ["".join(chars[int(c)] for c in rng.integers(1, len(chars), size=int(rng.integers(0, 50)))) for _ in range(200)]
    texts += ["", ""]
    rows = hb.synthetic_rows(texts, rng.random(len(texts)).astype(np.float32))
    got, _c, _c3 = assert_same(rows)
    assert got == texts
    assert_same(rows[:1])
    assert_same(hb.synthetic_rows(["", "", ""], [0.0, 0.0, 0.0], row_bytes=16))      # rows with no room for text at all
    assert H.parse_ctc_rows_native(np.zeros((0, 64), np.uint8)) == ([], [], [])


def test_confidences_on_the_rounding_boundaries():
    """float(f"{score:.3f}") rounds the float32's exact double value, half to even on the decimal expansion: values on both sides of
    every x.xxx5, 0.0 and 1.0."""
    ties = np.arange(0, 1000, dtype=np.float64) / 1000 + 0.0005
    near = np.concatenate([np.nextafter(ties.astype(np.float32), np.float32(d)) for d in (0, 2)] + [ties.astype(np.float32)])
    exact = np.array([0.0, 1.0, 0.5, 0.125, 0.0625, 0.9995, 0.99951172, 2.5e-4, 4.8828125e-4, 0.00048828125 * 3, 1e-8, 0.375, 0.8125], np.float32)
    rng = np.random.default_rng(11)
    conf = np.concatenate([near, exact, rng.random(3000).astype(np.float32)])
    _t, c, c3 = assert_same(hb.synthetic_rows(["x"] * len(conf), conf))
    assert c3[3000] == 0.0 and c3[3001] == 1.0 and c[3001] == 1.0
    assert max(abs(a - b) for a, b in zip(c, c3)) <= 0.0005 + 1e-12


def test_a_corrupt_row_is_refused():
    import pytest
    rows = hb.synthetic_rows(["abc"], [0.5], row_bytes=32)
    rows[0, :4] = np.frombuffer(np.array([17], "<i4").tobytes(), np.uint8)          # more text bytes than the row has room for
    with pytest.raises(RuntimeError):
        H.parse_ctc_rows_native(rows)
