"""CPU: the helpers that tests/test_gpu_attention.py judges the attention kernels with are themselves right - the fp64 reference equals
torch's own scaled-dot-product attention, and the ragged line table puts lines where the engine's `ragged_tables` puts them."""
import numpy as np
import torch

from test_gpu_attention import attention_reference, place_lines, random_qkv, rising_qkv


def test_reference_equals_torch_sdpa_in_fp64():
    heads, hd = 8, 15
    lengths = [33, 1, 70]
    seg, rows = place_lines(lengths)
    qkv = random_qkv(rows, heads, hd, 3, 5)
    scale = hd ** -0.5
    got = attention_reference(qkv, [tuple(r) for r in seg.tolist()], heads, hd, scale)
    assert got.dtype == torch.float64 and got.shape == (rows, heads * hd)
    for first, n in seg.tolist():
        r = qkv[first:first + n].double().reshape(n, 3, heads, hd).permute(1, 2, 0, 3)
        want = torch.nn.functional.scaled_dot_product_attention(r[0], r[1], r[2], scale=scale)       # [heads][n][hd]
        want = want.permute(1, 0, 2).reshape(n, heads * hd)
        assert float((got[first:first + n] - want).abs().max()) < 1e-13
    # a row that no line owns is NaN, so a comparison that reads it cannot pass by accident
    seg2, rows2 = place_lines([4, 0, 3], order=[2, 0, 1], gap_after=2, gap=2, guard=1)
    got2 = attention_reference(random_qkv(rows2, heads, hd, 1, 6), [tuple(r) for r in seg2.tolist()], heads, hd, scale)
    assert seg2.tolist() == [[5, 4], [9, 0], [0, 3]] and rows2 == 10
    assert torch.isnan(got2[:, 0]).tolist() == [False] * 3 + [True] * 2 + [False] * 4 + [True]


def test_line_table_matches_the_engine():
    from rapiddoc_amd.engine import ragged_tables
    lengths = [33, 1, 768, 769, 0, 5, 1153, 32]
    seg, rows = place_lines(lengths)
    eseg, tokinfo = ragged_tables(np.asarray(lengths))
    assert seg.dtype == eseg.dtype == np.int32 and np.array_equal(seg, eseg)
    assert rows == len(tokinfo) == sum(lengths)


def test_score_spread_of_the_inputs():
    """q, k ~ N(0, a2) give scaled scores of standard deviation a2; the rising set climbs by `rise` per 32 keys for even queries."""
    heads, hd, scale = 8, 15, 15 ** -0.5
    for a2 in (0.2, 3, 10):
        x = random_qkv(400, heads, hd, a2, 1).double().reshape(400, 3, heads, hd)
        s = torch.einsum("ihd,jhd->hij", x[:, 0], x[:, 1]) * scale
        assert abs(float(s.std()) / a2 - 1) < 0.05
    T = 96
    x = rising_qkv(1, T, heads, hd, scale, 2, rise=3.0).double().reshape(T, 3, heads, hd)
    s = torch.einsum("ihd,jhd->hij", x[:, 0], x[:, 1]) * scale
    tile_max = s.reshape(heads, T, 3, 32).max(dim=3).values
    up = tile_max[:, 0::2, 1:] - tile_max[:, 0::2, :-1]          # even queries: + u
    assert float(up.min()) > 2.0 and float(up.max()) < 4.0
    assert bool((tile_max[:, 1::2].argmax(dim=2) == 0).all())     # odd queries: the maximum sits in the first tile
