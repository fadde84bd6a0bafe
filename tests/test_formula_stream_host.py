"""CPU: what the refilled-slot formula decode (rd_formula_decode_stream) needs no GPU for - the host restatement of its schedule
(tests/stream_reference.py) against the properties of list scheduling, the new symbols, the window split of `FormulaRecognizer`, and the
loud failure without a GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stream_reference as SR

ROOT = Path(__file__).resolve().parents[1]


def test_simulated_schedule_is_list_scheduling():
    """200 random length sets: every slot serves its formulas in admission order, formulas are admitted in queue order, no slot idles while a
    formula waits, every formula is live for exactly lens - 1 consecutive steps from position 0, and the run ends within
    floor(sum / slots) + max steps."""
    rng = np.random.default_rng(7)
    for case in range(200):
        N, slots, cap = int(rng.integers(1, 40)), int(rng.integers(1, 33)), int(rng.integers(1, 30))
        tokens = np.minimum(rng.geometric(0.15, N), cap) if case % 3 else rng.integers(1, cap + 1, N)
        lens = tokens + 1
        sched = SR.simulate(lens, slots)
        steps = len(sched)
        assert steps <= SR.refill_bound(lens, slots) and steps >= max(int(tokens.max()), -(-int(tokens.sum()) // slots))
        first = {}
        for t in range(steps):
            for s in range(slots):
                f, p = int(sched[t, s, 0]), int(sched[t, s, 1])
                if f < 0:
                    assert p == 0
                    continue
                if f not in first:
                    assert p == 0
                    first[f] = (t, s)
                t0, s0 = first[f]
                assert s == s0 and p == t - t0 and p < tokens[f], (case, f, t)
        assert sorted(first) == list(range(N))
        for f in range(N):
            t0, s0 = first[f]
            assert (sched[t0: t0 + tokens[f], s0, 0] == f).all()                      # live for exactly lens - 1 steps
            assert t0 + tokens[f] == steps or sched[t0 + tokens[f], s0, 0] != f
        order = sorted(range(N), key=lambda f: (first[f][0], first[f][1]))
        assert order == list(range(N)), "admission follows the queue, the lowest slot first"
        for s in range(slots):
            mine = [f for f in range(N) if first[f][1] == s]
            assert mine == sorted(mine) and all(first[a][0] < first[b][0] for a, b in zip(mine, mine[1:]))
        admitted_by = np.zeros(steps, dtype=np.int64)                                 # formulas admitted up to and including step t
        for f in range(N):
            admitted_by[first[f][0]:] += 1
        for t in range(steps):
            if (sched[t, :, 0] < 0).any():
                assert admitted_by[t] == N, (case, t, "a slot idles while a formula waits")
        assert int((sched[:, :, 0] >= 0).sum()) == int(tokens.sum())
        assert SR.chunk_steps(lens, slots) >= max(int(tokens.max()), steps if N <= slots else 0)


def test_the_oracle_lengths_of_the_issue():
    """the fp32 oracle's lengths at S = 144 (24 sequences, 40 new tokens): chunks of 8 take 116 steps, eight refilled slots at most 75 (+ 7)"""
    tokens = [6, 33, 40, 1, 2, 16, 4, 1, 4, 11, 40, 1, 1, 3, 3, 16, 15, 36, 9, 9, 2, 1, 3, 23]
    lens = np.asarray(tokens) + 1
    assert SR.chunk_steps(lens, 8) == 116 and SR.refill_bound(lens, 8) == 75 and SR.refill_bound(lens, 8, look_ahead=7) == 82
    assert len(SR.simulate(lens, 8)) <= 75
    ids = np.full((2, 6), 1)
    ids[:, 0] = 0
    ids[0, 1:4] = (7, 9, 2)
    ids[1, 1:] = 7
    assert SR.lens_of(ids, 5).tolist() == [4, 6]


def test_new_symbols_exist_everywhere():
    from rapiddoc_amd import _lib, build as rd_build
    rd_build.build(verbose=False)
    lib = _lib.load()
    header = (ROOT / "include" / "rapiddoc_mi355.h").read_text()
    assert re.search(r"\bint rd_formula_decode_stream\s*\(", header) and "typedef struct rd_formula_stream_stats" in header
    m = re.search(r"#define RD_FORMULA_STREAM_MAX_TOKENS (\d+)", header)
    from rapiddoc_amd import engine
    assert m and int(m.group(1)) == engine.FORMULA_STREAM_MAX_TOKENS
    assert int(re.search(r"#define RD_FORMULA_STREAM_MAX_SLOTS (\d+)", header).group(1)) == engine.FORMULA_STREAM_MAX_SLOTS == 32
    assert "rd_formula_decode_stream" in _lib.SYMBOLS and "rd_debug_formula_decode_stream" in _lib.DEBUG_SYMBOLS
    assert hasattr(lib, "rd_formula_decode_stream") and hasattr(lib, "rd_debug_formula_decode_stream")
    assert "rd_debug_formula_decode_stream" in (ROOT / "rapiddoc_amd" / "csrc" / "api_debug.cpp").read_text()
    assert "rd_debug_formula_decode_stream" in (ROOT / "tools" / "README.md").read_text()
    assert C.sizeof(engine.FormulaStreamStats) == 16


def test_window_split_for_the_token_limit():
    from rapiddoc_amd.engine import FORMULA_STREAM_MAX_TOKENS as T
    from rapiddoc_amd.formula_host import stream_windows
    assert stream_windows(0, 144, T) == []
    assert stream_windows(5, 144, T) == [(0, 5)]
    per = T // 144
    assert per * 144 <= T < (per + 1) * 144
    assert stream_windows(per, 144, T) == [(0, per)] and stream_windows(per + 1, 144, T) == [(0, per), (per, per + 1)]
    w = stream_windows(3 * per + 2, 144, T)
    assert w == [(0, per), (per, 2 * per), (2 * per, 3 * per), (3 * per, 3 * per + 2)]
    assert all((e - b) * 144 <= T for b, e in w)
    assert stream_windows(7, 3, 7) == [(0, 2), (2, 4), (4, 6), (6, 7)]
    with pytest.raises(ValueError):
        stream_windows(1, T + 1, T)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_stream_fails_loudly_without_a_gpu():
    from rapiddoc_amd import _lib, build as rd_build
    rd_build.build(verbose=False)
    lib = _lib.load()
    assert not lib.rd_create(0, b"ppformulanet_head") and b"no HIP device" in lib.rd_create_error()
    assert lib.rd_formula_decode_stream(None, None, 1, 1, 1, 1, None, None, None, None) != 0          # no handle: refused, nothing touched
    from rapiddoc_amd.engine import EngineError
    from rapiddoc_amd.formula_host import FormulaRecognizer
    with pytest.raises(EngineError):
        FormulaRecognizer({}, batching="stream", slots=2)
    with pytest.raises(ValueError):
        FormulaRecognizer({}, batching="rows")
