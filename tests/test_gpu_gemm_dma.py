"""GPU: the LDS-DMA split GEMM alone (csrc/kernels_gemm_h3_dma.hip: gemm_h3_dma_kernel, 8 wavefronts, `dma256x128`; gemm_h3_dma16_kernel, 16
wavefronts, `dma16w256x128`) against torch's fp64 product through rd_debug_conv_ex on the natural route of a pointwise layer WITHOUT the
one-accumulator image - what such a layer gets in the engine (with the image every K % 32 == 0 shape runs on gemm_h1 instead).  256 x 128
output tiles, K tiles of 32 in three LDS stages, persistent workgroups.  Strided views in sentinel-filled buffers, a bound per output
element (conv_helpers), the route asserted per case.  Under RD_H3_DMA16=1 (read once per process: a child interpreter) every case runs on
the 16-wavefront kernel and meets the same bounds.  Cases and measured ratios: docs/notebook/conv_tile_kernels.md."""
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for _p in (str(ROOT), str(ROOT / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest
import torch

from conv_helpers import GELU, RELU, Problem, assert_bit_identical, check_launch, launch, pointwise

pytestmark = pytest.mark.gpu

DMA8, DMA16 = "dma256x128", "dma16w256x128"


def slots(k, ng, res=True):
    return dict(x_slot=(k + 28, 12), y_slot=(ng + 11, 5), r_slot=(ng + 3, 3) if res else None)


# (case, the route by default).  K >= 64, K % 4 == 0, Ng >= 96: what gemm_h3_dma_applies takes
CASES = [(pointwise(256 + 37, k, 133, act=RELU, why="K = %d: %d K tiles on 3 stages%s, M = 256 + 37, Ng = 128 + 5" % (k, -(-k // 32), ", K %% 32 = 4" if k % 32 else "")), DMA8)
         for k in (64, 68, 96, 100, 128)]
CASES += [
    (pointwise(1, 68, 96, why="M = 1, Ng = 96: one row of a tile narrower than DN (K = 68: at Cin <= 64 such a layer streams)"), DMA8),
    (pointwise(255, 68, 96, res=True, why="M = 255, Ng = 96: one row short of a tile"), DMA8),
    (pointwise(256 + 37, 100, 133, act=RELU, res=True, **slots(100, 133), why="K = 100 in slots: xld = K + 28, yld = Ng + 11, rld = Ng + 3"), DMA8),
    (pointwise(256 + 37, 192, 133, act=GELU, why="K = 192 + GELU: the short-K GELU rule"), DMA16),
    (pointwise(256 + 37, 196, 133, act=GELU, why="K = 196 + GELU: beyond the rule"), DMA8),
]


def run_case(i, route=None):
    cs, default = CASES[i]
    pb = Problem(cs, 3000 + i)
    r = launch(pb, 1)
    return pb, r, check_launch(pb, r, 1, route or default, "dma #%d %s" % (i, cs["why"]))


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: "%02d-M%d-K%d-N%d" % (i, CASES[i][0]["w"], CASES[i][0]["cin"], CASES[i][0]["cout"]))
def test_dma_gemm_matches_fp64(i):
    """#1, #2, #4"""
    run_case(i)


def test_k_tail_reads_nothing_beyond_k():
    """#3: K = 100 = 3 x 32 + 4 in a slot of a 128-wide buffer.  The chunks of the last K tile beyond K re-read the row's last chunk and meet
    the zero padding of the weight planes: the words of the x buffer beyond the view cannot reach the output, whatever finite value they hold"""
    pb = Problem(CASES[7][0], 3007)
    a = launch(pb, 1, x_fill=3.5)
    b = launch(pb, 1, x_fill=-1234.0)
    check_launch(pb, a, 1, DMA8, "dma #3 fill 3.5")
    check_launch(pb, b, 1, DMA8, "dma #3 fill -1234")
    assert_bit_identical(a.y, b.y, "dma #3: the buffer's columns beyond K reached the output")


def test_persistent_second_round():
    """#6: more 256 x 128 tiles than CUs (Ng = 133: two column tiles per row tile): the persistent loop's second round, whose first DMAs are
    issued across the epilogue of the previous tile"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ntm = cus // 2 + 1
    assert cus < 2 * ntm <= 2 * cus
    pb = Problem(pointwise(ntm * 256 - 19, 64, 133, act=RELU, res=True, **slots(64, 133), why="%d x 2 tiles on %d CUs" % (ntm, cus)), 3100)
    check_launch(pb, launch(pb, 1), 1, DMA8, "dma #6 " + pb.cs["why"])


def test_range_flag():
    """#7: one activation beyond the fp16 range raises the flag; the other rows are ordinary results and nothing outside the view is written"""
    pb = Problem(CASES[7][0], 3007)
    r = launch(pb, 1, x_poke=(3, 5, 1e5))
    assert r.ms >= 0 and r.route == DMA8 and r.flag == 1, (r.ms, r.route, r.flag)
    r.yv.assert_outside_untouched("dma #7")
    r.xv.assert_unchanged("dma #7")
    r.rv.assert_unchanged("dma #7")
    others = torch.arange(pb.rows) != 3
    assert bool(torch.isfinite(r.y[others]).all())
    assert bool(((r.y.double() - pb.ref).abs() <= pb.bound(1))[others].all())


def test_every_case_on_the_16_wavefront_kernel_under_rd_h3_dma16_1():
    """#5: the first fp64 test of gemm_h3_dma16_kernel: every case above, routed to it by the switch, within the same bounds"""
    env = dict(os.environ, RD_H3_DMA16="1")
    r = subprocess.run([sys.executable, __file__, "dma16"], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout[-6000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-2500:])
    assert r.stdout.count("[%s]" % DMA16) == len(CASES) + 3


if __name__ == "__main__":
    assert sys.argv[1] == "dma16" and os.environ.get("RD_H3_DMA16") == "1"
    for i_ in range(len(CASES)):
        run_case(i_, DMA16)
    pb_ = Problem(CASES[7][0], 3007)
    a_, b_ = launch(pb_, 1, x_fill=3.5), launch(pb_, 1, x_fill=-1234.0)
    check_launch(pb_, a_, 1, DMA16, "dma16 #3 fill 3.5")
    check_launch(pb_, b_, 1, DMA16, "dma16 #3 fill -1234")
    assert_bit_identical(a_.y, b_.y, "dma16 #3")
    cus_ = torch.cuda.get_device_properties(0).multi_processor_count
    pb_ = Problem(pointwise((cus_ // 2 + 1) * 256 - 19, 64, 133, act=RELU, res=True, **slots(64, 133), why="persistent"), 3100)
    check_launch(pb_, launch(pb_, 1), 1, DMA16, "dma16 #6")
    r_ = launch(Problem(CASES[7][0], 3007), 1, x_poke=(3, 5, 1e5))
    assert r_.route == DMA16 and r_.flag == 1, (r_.route, r_.flag)
    r_.yv.assert_outside_untouched("dma16 #7")
