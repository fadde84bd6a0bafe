#!/usr/bin/env python3
"""Mint the PP-OCRv5 mobile recogniser fixtures (PPLCNetV3 scale 0.95 + SVTR neck + CTC) from the REFERENCE's own
nn.Module definitions, with synthetic weights (``rapiddoc_amd.weights``).

Runs only in the build container (it imports the reference tree); what it writes next to itself is data only:

    manifest_ppocrv5_rec_mobile.json       weight names / shapes of the reference state dict
    rec5m_seed0_{b2_w320,b1_w96,b3_w640,b6_w1088}.npz
                                           x (or the seed / kind that regenerate it), backbone output (every `backbone_cs`-th channel
                                           where the full tensor would exceed the size limit of a committed file), neck output
                                           (head.ctc_encoder), idx, prob, top2gap, top2idx, logits_sub (every 61st class), logits_t0
    rec5m_seed0_b6_w1088_logits.npz        logits_sub of the full-width case (its own file: 0.98 MB on its own)
    rec5m_width_pair.npz                   one 200-px line alone and zero-padded to 320: backbone + neck outputs of both, d
    summary_v5_mobile.json                 per fixture: share of positions with top2gap <= 1e-2, mean per-channel std over T of the
                                           neck output and of the backbone output (relative to its absmax), distinct argmax classes;
                                           min / max of d; the weight checksum

It asserts conditions on the REFERENCE (never on the engine): masked share <= 1 % per fixture, backbone std over T >= 0.02 of its absmax,
>= 5 distinct argmax classes in every fixture of >= 80 positions, and the width pair >= 10 x the engine bound apart at the neck.

    python tests/golden/make_golden_v5_mobile.py
"""
import json
import sys
from pathlib import Path

import numpy as np
import torch
import yaml

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
REF = Path("/root/reference")

from rapiddoc_amd import weights as W  # noqa: E402

SEED = 0
ARCH = "ch_PP-OCRv5_rec_mobile"
LIMIT = 1 << 20
TOL = 1e-3           # the engine tests' bound; the width pair must lie >= 10 x TOL apart at every step


def make_input(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)


def input_seed(tag, shape):
    return 200 + len(tag) + shape[3]


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    sys.path.insert(0, str(REF / "rapid_doc/model/ocr"))
    from ppocrv6_pytorch.modeling.architectures.base_model import BaseModel

    arch = yaml.safe_load(open(REF / "rapid_doc/resources/arch_config.yaml"))
    rec = BaseModel(arch[ARCH])
    man = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in rec.state_dict().items()]
    (HERE / "manifest_ppocrv5_rec_mobile.json").write_text(json.dumps(man))
    state = W.synth_state_dict([(n, tuple(s), d) for n, s, d in man], SEED)
    rec.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    rec.eval()
    summary = {"checksum": W.checksum(state), "tensors": len(man),
               "parameters": int(sum(int(np.prod(s)) for n, s, d in man if d == "float32")), "fixtures": {}}

    def forward(x):
        with torch.no_grad():
            bb = rec.backbone(torch.from_numpy(x))
            neck = rec.head.ctc_encoder(bb)                 # [B, T, 120]
            logits = rec.head.ctc_head.fc(neck)
            prob = rec.head(bb)                             # softmax probabilities [B, T, C] (CTCHead, eval mode)
        assert float((torch.softmax(logits, dim=2) - prob).abs().max()) == 0.0
        return bb, neck, logits, prob

    for tag, shape in (("b2_w320", (2, 3, 48, 320)), ("b1_w96", (1, 3, 48, 96)), ("b3_w640", (3, 3, 48, 640)),
                       ("b6_w1088", (6, 3, 48, 1088))):
        # the input: the v6 fixtures' seed rule; where the REFERENCE's own top-2 gaps leave more than 1 % of the positions inside the
        # 1e-2 mask, the next seed is taken (the input changes, never the cap)
        seed = input_seed(tag, shape)
        while True:
            x = make_input(shape, seed)
            bb, neck, logits, prob = forward(x)
            top2 = torch.topk(logits, 2, dim=2)
            gap = (top2.values[..., 0] - top2.values[..., 1]).numpy()
            if float((gap <= 1e-2).mean()) <= 0.01:
                break
            print(f"{tag}: seed {seed} leaves {float((gap <= 1e-2).mean()):.4f} of the positions masked, trying the next")
            seed += 1
        p, idx = prob.max(dim=2)
        out = dict(neck=neck.numpy(), idx=idx.numpy().astype(np.int32), prob=p.numpy(), top2gap=gap,
                   top2idx=top2.indices.numpy().astype(np.int32), logits_t0=logits[:, 0, :].contiguous().numpy(),
                   x_seed=np.int64(seed), x_kind=np.array("pm1"), x_shape=np.array(shape, dtype=np.int64))
        if x.nbytes <= LIMIT // 2:
            out["x"] = x
        cs = 1
        while bb[:, ::cs].numel() * 4 > LIMIT // 3:
            cs *= 2
        out["backbone"] = bb[:, ::cs].contiguous().numpy()
        out["backbone_cs"] = np.int64(cs)
        sub = logits[:, :, ::61].contiguous().numpy()
        if sub.nbytes > LIMIT // 2:
            np.savez_compressed(HERE / f"rec5m_seed0_{tag}_logits.npz", logits_sub=sub)
            assert (HERE / f"rec5m_seed0_{tag}_logits.npz").stat().st_size <= LIMIT
        else:
            out["logits_sub"] = sub
        f = HERE / f"rec5m_seed0_{tag}.npz"
        np.savez_compressed(f, **out)
        assert f.stat().st_size <= LIMIT, (f, f.stat().st_size)
        share = float((gap <= 1e-2).mean())
        stdT = float(neck.numpy().std(axis=1).mean())
        bb_rel = float(bb.numpy().std(axis=3).mean() / bb.abs().max())      # the net is alive: its output varies along the line
        summary["fixtures"][tag] = {"masked_share": share, "neck_std_over_T": stdT, "backbone_std_over_T_rel": bb_rel, "distinct_argmax": int(len(np.unique(idx.numpy()))),
                                    "backbone_absmax": float(bb.abs().max()), "neck_absmax": float(neck.abs().max()),
                                    "logits_absmax": float(logits.abs().max()), "bytes": f.stat().st_size}
        print(tag, summary["fixtures"][tag])
        assert share <= 0.01, (tag, share)
        assert bb_rel >= 0.02, (tag, bb_rel)
        assert idx.numel() < 80 or len(np.unique(idx.numpy())) >= 5, (tag, len(np.unique(idx.numpy())))

    # one 200-px line alone and zero-padded to 320
    x200 = make_input((1, 3, 48, 200), 777)
    x320 = np.zeros((1, 3, 48, 320), np.float32)
    x320[..., :200] = x200
    bb_a, neck_a, _, _ = forward(x200)
    bb_b, neck_b, _, _ = forward(x320)
    T = neck_a.shape[1]
    d = (neck_a[0] - neck_b[0, :T]).abs().max(dim=1).values.numpy()
    f = HERE / "rec5m_width_pair.npz"
    np.savez_compressed(f, x200=x200, backbone200=bb_a.numpy(), neck200=neck_a.numpy(), backbone320=bb_b.numpy(), neck320=neck_b.numpy(), d=d)
    assert f.stat().st_size <= LIMIT, f.stat().st_size
    summary["width_pair"] = {"steps": int(T), "d_min": float(d.min()), "d_max": float(d.max()), "bytes": f.stat().st_size}
    print("width pair", summary["width_pair"])
    assert d.min() >= 10 * TOL, d.min()

    (HERE / "summary_v5_mobile.json").write_text(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
