"""GPU: bench.py's plain run and its options on a small configuration (4 pages, one page set, no setup passes): --dump-outputs writes
the last timed step's lines, identical from run to run; the per-op profiling pass (roofline) runs only with --full."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
SMALL = ["--gpus", "1", "--scaling", "strong", "--global-pages", "4", "--rec-streams", "2", "--steps", "2", "--warmup", "1",
         "--setup-steps", "0", "--setup-passes", "0", "--vary-pages", "1"]


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), *SMALL, *extra], capture_output=True, text=True, cwd=ROOT, env=env,
                       timeout=420)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_same_outputs_twice_and_full_adds_the_profiling_pass(tmp_path):
    a = _bench("--dump-outputs", str(tmp_path / "a"))
    b = _bench("--dump-outputs", str(tmp_path / "b"))
    for r in (a, b):
        assert r["steps"] == 2 and r["ms_per_step"] > 0 and r["unit"] == "pages/s" and r["higher_is_better"] is True
        assert r["roofline"] is None and "cpu_baseline" not in r and "backbone" not in r
    assert a["config"]["result_crc32"] == b["config"]["result_crc32"]
    names = sorted(p.name for p in (tmp_path / "a").glob("*.npy"))
    assert names == ["line_index.npy", "line_page.npy", "line_score.npy", "line_text_codepoints.npy"]
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float64 and np.array_equal(x, y), n
    assert len(np.load(tmp_path / "a" / "line_page.npy")) == a["config"]["lines_per_step"] == 180
    assert sorted(set(np.load(tmp_path / "a" / "line_page.npy").tolist())) == [0, 1, 2, 3]
    f = _bench("--full", "--no-extra-passes", "--no-cpu-baseline")
    assert f["roofline"]["kernel"] and f["roofline"]["frac"] > 0
    assert f["config"]["gather_page_dets_v2_ms"] is not None and f["config"]["h2d_ms_per_batch_alone"] is not None
    assert f["config"]["result_crc32"] == a["config"]["result_crc32"]
