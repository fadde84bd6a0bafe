"""CPU: bench.py --dump-outputs' array format (bench.dump_outputs) - one row per text line of the gathered, page-ordered result,
float64 only, a fixed seeded sample of the lines above the size cap."""
import numpy as np

import bench

OUT = [(0, [("ab", 0.5), ("", 0.25)]), (3, [("x中", 0.75)])]


def _load(d):
    return {p.stem: np.load(p) for p in sorted(d.glob("*.npy"))}


def test_dump_outputs_writes_every_line_as_float64(tmp_path):
    bench.dump_outputs(OUT, tmp_path)
    a = _load(tmp_path)
    assert sorted(a) == ["line_index", "line_page", "line_score", "line_text_codepoints"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert a["line_index"].tolist() == [0, 1, 2]
    assert a["line_page"].tolist() == [0, 0, 3]
    assert a["line_score"].tolist() == [0.5, 0.25, 0.75]
    assert a["line_text_codepoints"].tolist() == [[97, 98], [-1, -1], [120, 0x4E2D]]


def test_dump_outputs_samples_the_same_lines_above_the_cap(tmp_path, monkeypatch):
    out = [(p, [("line %d.%d" % (p, j), j / 10.0) for j in range(10)]) for p in range(20)]
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 50 * 8 * (3 + len("line 19.9")))
    bench.dump_outputs(out, tmp_path / "a")
    bench.dump_outputs(out, tmp_path / "b")
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert len(a["line_index"]) == 50
    assert all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["line_index"].astype(int)
    assert (np.diff(idx) > 0).all()
    assert a["line_page"].tolist() == [i // 10 for i in idx]
    assert a["line_score"].tolist() == [(i % 10) / 10.0 for i in idx]
