#!/usr/bin/env python3
"""What PagePipeline's recogniser stage planned and read for seeded quads, recorded from a running pipeline (needs the GPU).

    python tests/golden/make_golden_rec_plan.py [--out PATH]       # writes tests/golden/rec_plan_parent.npz

Run ONCE at the commit BEFORE the stage was split into plan / enqueue / decode: the fixture pins the split to what the one-body stage
did.  It uses only what that commit offers - `keep_rec_inputs` (last_rec_descs, last_rec_batches, last_pool_order,
last_rec_crop_sizes) and, after a synchronise, the persistent buffers ("rec_linetab", int32) and (("tail_tab", g), int32) of
`pipe._bufs`, which pin the first token of every line, its token count and the padded lengths of every tail call.

Pages are zeros (the plan reads no pixel), at most 96 x 640; every line's reference width is at most 640.  Each line set holds two
lines of exactly equal aspect ratio, two all-zero quads and two quads with h / w >= 2.  The committed file holds quads, settings and
recorded arrays / strings: data only."""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))

SEED = 9            # chosen so that the launch planner at 256 CUs cuts both line sets into three launches
V6 = ("ppocrv6_det", "ppocrv6_rec")
# name -> (line set, state kinds, constructor arguments, RD_REC_TWO_STAGE)
CASES = {
    "a": ("one", V6, dict(n_rec_streams=2), "1"),
    "b": ("two", V6, dict(n_rec_streams=2), "1"),
    "c": ("one", ("ppocrv6_det", "ppocrv5_rec_server"), dict(n_rec_streams=2), "1"),
    "d": ("one", V6, dict(rec_mode="throughput", n_rec_streams=2), "1"),
    "e": ("one", V6, dict(rec_batch_num=16, n_rec_streams=2), "1"),
    "f": ("one", V6, dict(rec_mode="strict", n_rec_streams=2), "0"),
}


def seeded_quads(rng, n, H, W, special=True):
    """n quads inside an H x W page: boxes of height 14..40 with aspect ratios of 6 to 12.8 for most (reference widths below 640: wide
    enough that the planner cuts ~120 lines into three launches), a third of them with corners moved by a fraction of a pixel; then
    the special ones."""
    h = rng.integers(14, 41, n)
    w = np.where(rng.random(n) < 0.9, h * rng.uniform(6.0, 12.4, n), h * rng.integers(1, 6, n)).astype(np.int64)
    w = np.minimum(w, W - 8)
    x0, y0 = rng.integers(2, W - 2 - w), rng.integers(2, H - 2 - h)
    q = np.stack([np.stack([x0, y0], 1), np.stack([x0 + w, y0], 1), np.stack([x0 + w, y0 + h], 1), np.stack([x0, y0 + h], 1)], 1).astype(np.float64)
    move = rng.random(n) < 0.33
    q[move] += rng.uniform(-0.45, 0.45, (int(move.sum()), 4, 2))
    if not special:
        return q
    q[1] = q[0] + 1.0                                  # two lines of exactly equal aspect ratio (integer corners, one translated)
    q[0], q[1] = np.round(q[0]), np.round(q[1])
    q[2] = q[3] = 0.0                                  # two degenerate quads
    for i, (ww, hh) in ((4, (20, 60)), (5, (17, 34))):  # two tall ones: h / w >= 2, rotated by the crop
        q[i] = np.array([[30 * i, 10], [30 * i + ww, 10], [30 * i + ww, 10 + hh], [30 * i, 10 + hh]], np.float64)
    return q[rng.permutation(n)]


def line_sets():
    """name -> ([(image shape [P, H, W], quads per image)], image_keys or None)"""
    rng = np.random.default_rng(SEED)
    q = seeded_quads(rng, 122, 96, 640)
    one = ([((3, 96, 640), [q[:50], q[50:51], q[51:]])], None)
    qa, qb = seeded_quads(rng, 70, 96, 640), seeded_quads(rng, 52, 80, 512, special=False)
    two = ([((2, 96, 640), [qa[:35], qa[35:]]), ((3, 80, 512), [qb[:10], qb[10:10], qb[10:]])], [[2, 0], [1, 3, 1]])
    return {"one": one, "two": two}


def parse_tail_table(buf, n_real):
    """The head of a ("tail_tab", g) buffer -> the padded line lengths of that tail call: (first token, tokens) pairs for as long as
    they run back to back, then one tokinfo word per token."""
    lens, off = [], 0
    for a, t in buf[: 2 * (len(buf) // 2)].reshape(-1, 2).tolist():
        if a != off or t < 1:
            break
        lens.append(t)
        off += t
    lens = np.asarray(lens, np.int64)
    assert len(lens) > n_real and len(lens) % 32 == 0 and off % 256 == 0, (len(lens), n_real, off)
    tok = buf[2 * len(lens): 2 * len(lens) + off]
    assert np.array_equal(tok & 0xFFFF, np.arange(off) - np.repeat(np.cumsum(lens) - lens, lens)) and np.array_equal(tok >> 16, np.repeat(lens, lens))
    return lens


def record(name, sets):
    import torch
    from rapiddoc_amd import weights as W
    from rapiddoc_amd.pipeline import PagePipeline
    set_name, kinds, kw, two_stage = CASES[name]
    shapes_quads, image_keys = sets[set_name]
    os.environ["RD_REC_TWO_STAGE"] = two_stage
    states = {k: W.synth_state_dict(W.load_manifest(HERE / f"manifest_{k}.json"), 0) for k in kinds}
    pipe = PagePipeline(states, **kw)
    del os.environ["RD_REC_TWO_STAGE"]
    pipe.keep_rec_inputs = True
    sources = [(torch.zeros(shape + (3,), dtype=torch.uint8, device="cuda"), quads) for shape, quads in shapes_quads]
    res = pipe.rec_forward_sources(sources, image_keys=image_keys)
    torch.cuda.synchronize()
    S = len(pipe.rec_engines)
    descs, batch_base, starts = pipe.last_rec_descs
    cw, ch, rot, keep = pipe.last_rec_crop_sizes
    lines_mode = pipe.rec_mode == "strict" and pipe.rec_two_stage
    out = {"set": set_name, "kinds": list(kinds), "kw": kw, "two_stage": two_stage == "1", "n_cu": pipe.n_cu, "S": S,
           "rec_lines_in_launch": bool(pipe.rec_lines_in_launch),
           "texts": [[[t for t, _s in img] for img in src] for src in res]}
    arr = {"scores": np.array([s for src in res for img in src for _t, s in img], np.float64),
           "descs": descs.view(np.uint8).copy(), "batch_base": batch_base, "starts": starts,
           "ids": np.concatenate([b[0] for b in pipe.last_rec_batches]).astype(np.int64),
           "crop_w": cw, "crop_h": ch, "rot90": rot, "keep": keep.astype(np.int64),
           "perm": np.zeros(0, np.int64) if pipe.last_pool_order is None else pipe.last_pool_order.astype(np.int64)}
    assert len(starts) - 1 == len(pipe.last_rec_batches) == pipe.stats["rec_batches"]
    if lines_mode:
        arr["line_w"] = np.concatenate([np.asarray(b[2]) for b in pipe.last_rec_batches]).astype(np.int64)
        arr["launch_w"] = np.array([b[1].shape[3] for b in pipe.last_rec_batches], np.int64)
        assert int(arr["line_w"].max()) <= 640
    else:
        arr["launch_w"] = np.array([b[1].shape[3] for b in pipe.last_rec_batches], np.int64)
        assert int(arr["launch_w"].max()) <= 640
    if lines_mode and pipe.rec_lines_in_launch:
        arr["linetab"] = pipe._bufs[("rec_linetab", torch.int32)][: 4 * len(descs)].cpu().numpy().reshape(-1, 4)
    if pipe.rec_two_stage:
        nb = len(starts) - 1
        tabs = []
        for gi, g in enumerate(range(0, nb, S)):
            n_real = int(starts[min(g + S, nb)] - starts[g])
            tabs.append(parse_tail_table(pipe._bufs[(("tail_tab", gi), torch.int32)].cpu().numpy(), n_real))
        arr["tail_lens"] = np.concatenate(tabs)
        arr["tail_n"] = np.array([len(t) for t in tabs], np.int64)
    assert int(descs["rot90"].sum()) >= 1 and len(keep) == sum(len(q) for _s, qs in shapes_quads for q in qs) - 2
    if name in ("a", "b"):
        assert len(starts) - 1 >= 3, "needs a full group of launches and a partial one"
    print(f"case {name}: {len(descs)} lines, {len(starts) - 1} launches, widths {sorted(set(arr['launch_w'].tolist()))}, "
          f"{len(set(t for s in out['texts'] for i in s for t in i))} distinct texts", flush=True)
    return out, arr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(HERE / "rec_plan_parent.npz"))
    args = ap.parse_args()
    sets = line_sets()
    save, meta = {}, {}
    for sname, (shapes_quads, image_keys) in sets.items():
        quads = [q for _s, qs in shapes_quads for q in qs]
        save[f"{sname}/quads"] = np.concatenate(quads).astype(np.float64)
        meta[sname] = {"shapes": [list(s) for s, _q in shapes_quads], "counts": [[len(q) for q in qs] for _s, qs in shapes_quads],
                       "image_keys": image_keys}
    cases = {}
    for name in CASES:
        cases[name], arr = record(name, sets)
        save.update({f"{name}/{k}": v for k, v in arr.items()})
    save["meta"] = np.frombuffer(json.dumps({"sets": meta, "cases": cases}).encode(), np.uint8)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(args.out, **save)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
