"""GPU: `td_select_kernel` and its per-slot copy `td_stream_select_kernel` (csrc/table_decoder.hip) alone, through the developer entry
`rd_debug_td_select`: the whitelist argmax against the documented rule (tests/td_reference.py `select_argmax`: NaN counts as -inf, ids
outside {1, 12 .. 509} at -1e9, the lowest id among equals) on random rows, on ties planted across the levels of the 1024-lane tree
reduction with the lower id on either side of the comparison, and on rows that are not finite; the bbox counter, the EOS latch and the
forced mode; what a launch writes - one column of `ids`, the state words, the next step's input row (emb[tok] + pos[step + 1] is one
rounding: bit-equal to torch fp32) - and that it writes nothing else.

A row whose whitelisted logits are all NaN or -inf names id 0, which lies outside the whitelist (-1e9 beats -inf): pinned here as the
behaviour, as the header of table_decoder.hip states it."""
import ctypes as C

import numpy as np
import pytest
import torch

import td_reference as R
import unitable_reference as U
from rapiddoc_amd import table_unitable as TU

pytestmark = pytest.mark.gpu

IDS = TU.STAND_IN_IDS
GUARD = 2
UNWRITTEN = -5
# (lower id, higher id).  Lane = id; at stride s lane t takes lane t + s where that one is greater, or equal with the lower id.  Two ids i < j
# meet at the stride s with i = j mod s, i != j mod 2 s, and i then sits in the UPPER lane of the two iff i mod 2 s >= s.  Lower id in the
# lower lane: neighbours (s = 1), the two whitelist ranges, s = 256, s = 128, the ends of the whitelist.  Lower id in the upper lane: s = 1,
# 2, 64, 128.
TIE_PAIRS = [(12, 13), (1, 12), (12, 268), (13, 141), (1, 509), (13, 14), (14, 16), (70, 134), (141, 269)]
_TABLES = {}


def tables():
    """emb [960][768], pos [1024][768] on the host and the device"""
    if not _TABLES:
        g = torch.Generator().manual_seed(9)
        _TABLES["emb"], _TABLES["pos"] = torch.randn((R.VOCAB, R.D), generator=g), torch.randn((R.MAXPOS, R.D), generator=g)
        _TABLES["dev"] = (_TABLES["emb"].cuda(), _TABLES["pos"].cuda())
    return _TABLES["emb"], _TABLES["pos"], _TABLES["dev"]


def random_logits(B, seed):
    return np.random.default_rng(seed).standard_normal((B, R.VOCAB)).astype(np.float32) * 3.0


def i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def hp(a):
    return None if a is None else a.ctypes.data


def run_batch(z, step, finished, boxcount, forced=None, ids_ld=None, max_new=R.MAXPOS):
    """One td_select_kernel launch.  Returns dict(ids [B][ids_ld], x [B][768], finished, boxcount, tok, chosen); the rows around `ids` and
    `x` must be unchanged."""
    _, _, (emb, pos) = tables()
    B = len(z)
    ids_ld = step + 2 if ids_ld is None else ids_ld
    zd = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).cuda()
    ids = torch.full((GUARD + B + GUARD, ids_ld), UNWRITTEN, dtype=torch.int64, device="cuda")
    x = torch.full((GUARD + B + GUARD, R.D), R.SENTINEL, device="cuda")
    fin, box, tok, chosen = i32(finished).copy(), i32(boxcount).copy(), np.full(B, -3, np.int32), np.full(B, -3, np.int32)
    fo = None if forced is None else i32(forced)
    cfg = TU.cfg_struct(IDS)
    rc = R.lib().rd_debug_td_select(0, zd.data_ptr(), B, C.addressof(cfg), max_new, ids[GUARD:].data_ptr(), ids_ld, emb.data_ptr(), pos.data_ptr(),
                                    x[GUARD:].data_ptr(), step, hp(fin), hp(box), hp(tok), hp(fo), 0 if fo is None else fo.shape[1], hp(chosen),
                                    None, None, None, None, None)
    assert rc == 0, rc
    idc, xc = ids.cpu(), x.cpu()
    for t, fill in ((idc, UNWRITTEN), (xc, R.SENTINEL)):
        assert bool((t[:GUARD] == fill).all() and (t[GUARD + B:] == fill).all()), "rows around the B written ones changed"
    return dict(ids=idc[GUARD:GUARD + B].numpy(), x=xc[GUARD:GUARD + B], finished=fin, boxcount=box, tok=tok, chosen=chosen)


def check_batch(z, step, finished, boxcount, forced=None, ids_ld=None, tag=""):
    """A launch against `select_reference`: the argmax, the one column of ids, the state words, the next input row - and nothing else"""
    emb, pos, _ = tables()
    got = run_batch(z, step, finished, boxcount, forced, ids_ld)
    ids_ld = got["ids"].shape[1]
    ref = R.select_reference(z, step, IDS, finished, boxcount, ids_ld, forced)
    assert got["chosen"].tolist() == ref["chosen"].tolist(), (tag, got["chosen"], ref["chosen"])
    assert bool(((got["chosen"] >= 0) & (got["chosen"] < R.VOCAB)).all()), tag
    want = np.full_like(got["ids"], UNWRITTEN)
    if ref["written"] is not None:
        want[:, step + 1] = ref["written"]
    assert np.array_equal(got["ids"], want), (tag, "ids")
    for k in ("finished", "boxcount", "tok"):
        assert got[k].tolist() == ref[k].tolist(), (tag, k, got[k], ref[k])
    rows = R.embed_row(emb, pos, ref["tok"], step + 1) if ref["embed"] else torch.full((len(z), R.D), R.SENTINEL)
    assert R.same_bits(got["x"], rows), (tag, "the next step's input row")
    return got, ref


def run_stream(z, src, pos_, box, done, max_new, n_tables, ids_ld=None):
    """One td_stream_select_kernel launch over len(z) slots.  Returns dict(ids [n_tables][ids_ld], lens [n_tables], x [M][768], pos, box, done)"""
    _, _, (emb, pos) = tables()
    M = len(z)
    ids_ld = max_new + 1 if ids_ld is None else ids_ld
    zd = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).cuda()
    ids = torch.full((GUARD + n_tables + GUARD, ids_ld), UNWRITTEN, dtype=torch.int64, device="cuda")
    lens = torch.full((GUARD + n_tables + GUARD,), UNWRITTEN, dtype=torch.int32, device="cuda")
    x = torch.full((GUARD + M + GUARD, R.D), R.SENTINEL, device="cuda")
    s, p, b, d = i32(src).copy(), i32(pos_).copy(), i32(box).copy(), i32(done).copy()
    cfg = TU.cfg_struct(IDS)
    rc = R.lib().rd_debug_td_select(1, zd.data_ptr(), M, C.addressof(cfg), max_new, ids[GUARD:].data_ptr(), ids_ld, emb.data_ptr(), pos.data_ptr(),
                                    x[GUARD:].data_ptr(), 0, None, None, None, None, 0, None, hp(s), hp(p), hp(b), hp(d), lens[GUARD:].data_ptr())
    assert rc == 0, rc
    idc, lc, xc = ids.cpu(), lens.cpu(), x.cpu()
    for t, n, fill in ((idc, n_tables, UNWRITTEN), (lc, n_tables, UNWRITTEN), (xc, M, R.SENTINEL)):
        assert bool((t[:GUARD] == fill).all() and (t[GUARD + n:] == fill).all()), "rows around the written ones changed"
    assert s.tolist() == i32(src).tolist()
    return dict(ids=idc[GUARD:GUARD + n_tables].numpy(), lens=lc[GUARD:GUARD + n_tables].numpy(), x=xc[GUARD:GUARD + M], pos=p, box=b, done=d)


def check_stream(z, src, pos_, box, max_new, n_tables, done=None, tag=""):
    emb, pos, _ = tables()
    M = len(z)
    done = [0] * M if done is None else done
    got = run_stream(z, src, pos_, box, done, max_new, n_tables)
    ref = R.stream_select_reference(z, IDS, max_new, src, pos_, box)
    want_ids, want_lens = np.full_like(got["ids"], UNWRITTEN), np.full_like(got["lens"], UNWRITTEN)
    for (tab, col), v in ref["writes"].items():
        want_ids[tab, col] = v
    for tab, n in ref["lens"].items():
        want_lens[tab] = n
    assert np.array_equal(got["ids"], want_ids), (tag, "ids")
    assert np.array_equal(got["lens"], want_lens), (tag, "lens")
    assert got["pos"].tolist() == ref["pos"].tolist() and got["box"].tolist() == ref["box"].tolist(), (tag, got, ref)
    assert got["done"].tolist() == np.maximum(ref["done"], i32(done)).tolist(), (tag, "done")
    for s in range(M):
        row = R.embed_row(emb, pos, int(ref["tok"][s]), int(ref["pos"][s])) if ref["tok"][s] >= 0 else torch.full((R.D,), R.SENTINEL)
        assert R.same_bits(got["x"][s], row), (tag, "the slot's next input row", s)
    return got, ref


def both_forms(z, tag):
    """The argmax of rows z through both kernels; returns the batch form's chosen ids"""
    B = len(z)
    got, _ = check_batch(z, 4, [0] * B, [0] * B, tag=tag + " batch")
    _, ref = check_stream(z, list(range(B)), [4] * B, [0] * B, 64, B, tag=tag + " stream")
    assert [ref["writes"][(b, 5)] for b in range(B)] == got["ids"][:, 5].tolist()
    return got["chosen"]


@pytest.mark.parametrize("B", [1, 3, 8])
def test_argmax_both_forms(B):
    z = random_logits(B, 20 + B)
    z[0, 700] = 99.0                                                   # outside the whitelist
    chosen = both_forms(z, f"argmax B{B}")
    assert all(c in U.WHITE for c in chosen)


@pytest.mark.parametrize("lower_first", [True, False])
def test_planted_ties_the_lower_id_wins(lower_first):
    """Row r: pair r holds the row's maximum twice.  `lower_first`: the two are the row's only maxima; otherwise a third, lower id holds a
    value just below, and a higher id outside the whitelist a greater one - the winner is still the pair's lower id."""
    z = random_logits(len(TIE_PAIRS), 31)
    for r, (a, b) in enumerate(TIE_PAIRS):
        top = np.float32(z[r].max() + 1.0)
        z[r, a] = z[r, b] = top
        if not lower_first:
            z[r, 15 if a != 15 else 16] = np.nextafter(top, np.float32(0))
            z[r, 600] = top + np.float32(1.0)
    chosen = [int(c) for r0 in range(0, len(z), R.MAXB) for c in both_forms(z[r0:r0 + R.MAXB], f"ties lower_first={lower_first} rows {r0} ..")]
    assert chosen == [a for a, _ in TIE_PAIRS]
    z = np.full((3, R.VOCAB), 2.5, np.float32)                          # flat rows: id 1, the lowest whitelisted
    z[1, 1] = np.nextafter(np.float32(2.5), np.float32(0))              # ... and with id 1 just below: id 12
    z[2, U.WHITE] = -1e9                                                # level with the ids outside the whitelist: id 0
    assert both_forms(z, "flat rows").tolist() == [1, 12, 0]


def test_rows_that_are_not_finite():
    z = random_logits(6, 41)
    z[0, U.WHITE[np.argmax(z[0, U.WHITE])]] = np.nan                    # one NaN: the row's best whitelisted entry
    z[1, :] = np.nan                                                    # all NaN: id 0
    z[2, U.WHITE] = -np.inf                                             # all -inf on the whitelist: id 0
    z[3, U.WHITE] = -np.inf
    z[3, 333] = -40.0                                                   # one finite value among -inf
    z[4, 21] = np.inf                                                   # +inf against NaN
    z[4, 20] = z[4, 22] = np.nan
    z[5, :] = np.inf                                                    # all +inf: id 1
    chosen = both_forms(z, "non-finite rows")
    assert chosen[1:].tolist() == [0, 0, 333, 21, 1] and chosen[0] in U.WHITE
    assert bool(((chosen >= 0) & (chosen < R.VOCAB)).all())


def _row_choosing(token, B=1):
    z = random_logits(B, 51)
    z[:, token] = 60.0
    return z


def test_bbox_counter():
    bbox, other = IDS.bbox_first + 7, 13
    for count in range(4):                                              # at 0 .. 3 a bbox id raises it
        got, _ = check_batch(_row_choosing(bbox), 6, [0], [count], tag=f"bbox count {count}")
        assert got["boxcount"].tolist() == [count + 1] and got["ids"][0, 7] == bbox
    got, _ = check_batch(_row_choosing(bbox), 6, [0], [4], tag="bbox overflow")             # at 4 it emits close_id and clears it
    assert got["boxcount"].tolist() == [0] and got["ids"][0, 7] == IDS.bbox_close and got["chosen"].tolist() == [bbox] and got["tok"].tolist() == [IDS.bbox_close]
    for count in (0, 3, 4):                                             # a non-bbox id leaves it alone
        got, _ = check_batch(_row_choosing(other), 6, [0], [count], tag="non-bbox")
        assert got["boxcount"].tolist() == [count] and got["ids"][0, 7] == other
    z = np.concatenate([_row_choosing(bbox), _row_choosing(other), _row_choosing(IDS.bbox_last)])       # a counter per table
    got, _ = check_batch(z, 0, [0, 0, 0], [4, 2, 1], tag="per table")
    assert got["boxcount"].tolist() == [0, 2, 2]


def test_eos_latch():
    z = np.concatenate([_row_choosing(IDS.eos), _row_choosing(40), _row_choosing(40)])
    got, _ = check_batch(z, 9, [0, 0, 1], [0, 0, 0], tag="latch")
    assert got["finished"].tolist() == [1, 0, 1]                        # a fresh EOS sets it
    assert got["ids"][:, 10].tolist() == [IDS.eos, 40, IDS.pad]         # a finished row writes pad ...
    assert got["tok"].tolist() == [IDS.eos, 40, IDS.eos]                # ... and feeds eos


def test_forced_mode():
    z = np.concatenate([_row_choosing(IDS.eos), _row_choosing(40), _row_choosing(41)])
    forced = np.array([[11, 30, 31, 32], [11, 5000, -9, 33], [11, 34, 35, 36]], np.int32)
    got, _ = check_batch(z, 0, [0, 0, 0], [0, 0, 0], forced=forced, tag="forced step 0")
    assert got["finished"].tolist() == [0, 0, 0] and got["ids"][:, 1].tolist() == [IDS.eos, 40, 41]     # the latch is off, the argmax is still recorded
    assert got["tok"].tolist() == [30, 959, 34]                         # forced[step + 1] is fed; ids outside the vocabulary are clamped
    got, _ = check_batch(z, 1, [0, 0, 0], [0, 0, 0], forced=forced, tag="forced step 1")
    assert got["tok"].tolist() == [31, 0, 35]
    got, _ = check_batch(z, 3, [0, 0, 0], [0, 0, 0], forced=forced, tag="forced past the list")
    assert got["tok"].tolist() == [IDS.eos] * 3


def test_writes_of_the_batch_form():
    z = random_logits(3, 61)
    got, _ = check_batch(z, 5, [0, 0, 0], [0, 0, 0], ids_ld=12, tag="one column")          # only column step + 1 (check_batch compares every entry)
    assert bool((got["ids"][:, 6] != UNWRITTEN).all())
    got, ref = check_batch(z, R.MAXPOS - 1, [0, 0, 0], [0, 0, 0], ids_ld=R.MAXPOS + 1, tag="step 1023")
    assert not ref["embed"] and bool((got["x"] == R.SENTINEL).all()) and bool((got["ids"][:, R.MAXPOS] != UNWRITTEN).all())
    got, ref = check_batch(z, R.MAXPOS - 2, [0, 0, 0], [0, 0, 0], tag="step 1022")         # the last row of the position table
    assert ref["embed"]
    got, _ = check_batch(z, 7, [0, 0, 0], [0, 0, 0], ids_ld=8, tag="no column step + 1")
    assert bool((got["ids"] == UNWRITTEN).all())


def test_stream_form_states():
    bbox = IDS.bbox_first + 3
    z = np.concatenate([_row_choosing(40), _row_choosing(IDS.eos), _row_choosing(41), _row_choosing(bbox), _row_choosing(bbox),
                        np.full((1, R.VOCAB), np.nan, np.float32), _row_choosing(42), _row_choosing(bbox)])
    src = [6, 2, 9, 0, 4, -1, 1, 10]
    pos = [0, 17, 29, 5, 22, 3, 28, 7]
    box = [0, 2, 0, 4, 1, 3, 0, 0]
    got, ref = check_stream(z, src, pos, box, 30, 11, tag="stream states")
    assert got["ids"][6, 1] == 40 and got["pos"][0] == 1 and got["done"][0] == 0                         # otherwise pos advances
    assert got["ids"][2, 18] == IDS.eos and got["lens"][2] == 19 and got["done"][1] == 1 and got["pos"][1] == 17     # the end by EOS
    assert got["ids"][9, 30] == 41 and got["lens"][9] == 31 and got["done"][2] == 1                       # the end by t + 1 == max_new
    assert bool((got["x"][1] == R.SENTINEL).all() and (got["x"][2] == R.SENTINEL).all())                  # ... and no row written
    assert got["ids"][0, 6] == IDS.bbox_close and got["box"].tolist() == [0, 2, 0, 0, 2, 3, 0, 1]         # box is per slot
    assert got["pos"][5] == 3 and got["done"][5] == 0 and bool((got["x"][5] == R.SENTINEL).all())          # an idle slot touches nothing
    assert got["pos"][6] == 29 and got["done"][6] == 0                                                    # t + 1 == max_new - 1 goes on
    # the last position: max_new = 1024, a slot at t = 1023 ends at the cap (ids column 1024), one at 1022 goes on to position row 1023
    got, ref = check_stream(z[[0, 0, 0]], [0, 1, 2], [1023, 1022, 1021], [0, 0, 0], 1024, 3, tag="stream cap")
    assert got["done"].tolist() == [1, 0, 0] and got["lens"].tolist() == [1025, UNWRITTEN, UNWRITTEN] and got["pos"].tolist() == [1023, 1023, 1022]


def test_arguments_no_launch_can_take():
    _, _, (emb, pos) = tables()
    z = torch.zeros((8, R.VOCAB), device="cuda")
    ids = torch.full((8, 8), UNWRITTEN, dtype=torch.int64, device="cuda")
    lens = torch.full((8,), UNWRITTEN, dtype=torch.int32, device="cuda")
    x = torch.full((8, R.D), R.SENTINEL, device="cuda")
    w = [np.zeros(8, np.int32) for _ in range(7)]
    cfg = TU.cfg_struct(IDS)
    f = R.lib().rd_debug_td_select

    def call(form=0, B=1, cfgp=C.addressof(cfg), max_new=8, ids_ld=8, step=0, zp=z.data_ptr(), fin=w[0], src=w[3]):
        return f(form, zp, B, cfgp, max_new, ids.data_ptr(), ids_ld, emb.data_ptr(), pos.data_ptr(), x.data_ptr(), step, hp(fin), hp(w[1]), hp(w[2]),
                 None, 0, None, hp(src), hp(w[4]), hp(w[5]), hp(w[6]), lens.data_ptr())
    assert call(B=0) == -1 and call(B=9) == -1 and call(cfgp=None) == -1 and call(zp=None) == -1
    assert call(max_new=0) == -1 and call(max_new=1025) == -1 and call(ids_ld=0) == -1
    assert call(step=-1) == -1 and call(step=1024) == -1 and call(fin=None) == -1
    assert call(form=1, src=None) == -1
    w[4][0] = 7
    assert call(form=1) == -1                                           # the slot's next column is no column of ids
    w[4][0] = -1
    assert call(form=1) == -1
    w[4][0], w[3][0] = 0, -2
    assert call(form=1) == -1
    assert bool((ids == UNWRITTEN).all() and (lens == UNWRITTEN).all() and (x == R.SENTINEL).all())
    assert all(int(a.sum()) == (-2 if i == 3 else 0) for i, a in enumerate(w))
    w[3][0] = 0
    assert call() == 0 and call(form=1) == 0
