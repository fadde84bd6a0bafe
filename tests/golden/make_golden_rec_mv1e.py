#!/usr/bin/env python3
"""Mint the fixtures of the multilingual PP-OCRv3 / v4 mobile recognisers (`ppocr_rec_mv1e`: MobileNetV1Enhance scale 0.5 + SVTR neck dims 64
+ CTCHead) from the REFERENCE's own nn.Module definitions, with synthetic weights (``rapiddoc_amd.weights``, kind gains "ppocr_rec_mv1e").

Runs only in the build container (it imports the reference tree); what it writes next to itself is data only:

    manifest_ppocr_rec_mv1e_korean.json    weight names / shapes of korean_PP-OCRv4_rec_mobile (3690 classes)
    manifest_ppocr_rec_mv1e_latin.json     ... of latin_PP-OCRv3_rec_mobile (187 classes: odd and small)
    recmv1e_korean_seed0_{b2_w320,b1_w96,b3_w640,b6_w1088}.npz, recmv1e_latin_seed0_{b6_w1088,b1_w96}.npz
                                           x (or the seed / kind that regenerate it), backbone output [B,512,1,T] (every `backbone_cs`-th channel where the
                                           full tensor would exceed the size limit of a committed file), neck output [B,T,64],
                                           idx, prob, top2gap, top2idx, logits_sub (every 61st class; latin: every 7th), logits_t0
    recmv1e_width_pair.npz                 korean: one 200-px line alone and zero-padded to 320: backbone + neck outputs of both, d
    summary_rec_mv1e.json                  per fixture: share of positions with top2gap <= 1e-2, std over T of the neck output and of the
                                           backbone output (relative to its absmax), distinct argmax classes; min / max of d; checksums

It asserts conditions on the REFERENCE (never on the engine): masked share <= 1 % per fixture and backbone std over T >= 0.01 of its absmax
(where an input seed misses either the next seed is taken, never the bound), >= 5 distinct argmax classes in every korean fixture of >= 80
positions, and the width pair >= 10 x the engine bound apart at the neck (its input seed is the first from 777 on that leaves twice that).

    python tests/golden/make_golden_rec_mv1e.py
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
KIND = "ppocr_rec_mv1e"
LIMIT = 1 << 20
TOL = 1e-3           # the engine tests' bound; the width pair must lie >= 10 x TOL apart at every step
FILES = {"korean": ("korean_PP-OCRv4_rec_mobile", 61, (("b2_w320", (2, 3, 48, 320)), ("b1_w96", (1, 3, 48, 96)), ("b3_w640", (3, 3, 48, 640)),
                                                        ("b6_w1088", (6, 3, 48, 1088)))),
         "latin": ("latin_PP-OCRv3_rec_mobile", 7, (("b6_w1088", (6, 3, 48, 1088)), ("b1_w96", (1, 3, 48, 96))))}


def make_input(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)


def load(arch_name):
    from ppocrv6_pytorch.modeling.architectures.base_model import BaseModel
    arch = yaml.safe_load(open(REF / "rapid_doc/resources/arch_config.yaml"))
    rec = BaseModel(arch[arch_name])
    man = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in rec.state_dict().items()]
    state = W.synth_state_dict([(n, tuple(s), d) for n, s, d in man], SEED, kind=KIND)
    rec.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    rec.eval()

    def forward(x):
        with torch.no_grad():
            bb = rec.backbone(torch.from_numpy(x))
            neck = rec.neck(bb)                             # [B, T, 64]
            logits = rec.head.fc(neck)
            prob = rec.head(neck)                           # softmax probabilities [B, T, C] (CTCHead, eval mode)
        assert float((torch.softmax(logits, dim=2) - prob).abs().max()) == 0.0
        return bb, neck, logits, prob
    return man, state, forward


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    sys.path.insert(0, str(REF / "rapid_doc/model/ocr"))
    summary = {"files": {}, "fixtures": {}}
    for lang, (arch_name, step, shapes) in FILES.items():
        man, state, forward = load(arch_name)
        (HERE / f"manifest_{KIND}_{lang}.json").write_text(json.dumps(man))
        summary["files"][lang] = {"stem": arch_name, "checksum": W.checksum(state), "tensors": len(man), "logits_step": step,
                                  "classes": int(state["head.fc.weight"].shape[0]),
                                  "parameters": int(sum(int(np.prod(s)) for n, s, d in man if d == "float32"))}
        for tag, shape in shapes:
            seed = 200 + shape[3]
            while True:
                x = make_input(shape, seed)
                bb, neck, logits, prob = forward(x)
                top2 = torch.topk(logits, 2, dim=2)
                gap = (top2.values[..., 0] - top2.values[..., 1]).numpy()
                bb_rel = float(bb.numpy().std(axis=3).mean() / bb.abs().max())      # the net is alive: its output varies along the line
                if float((gap <= 1e-2).mean()) <= 0.01 and bb_rel >= 0.01:
                    break
                print(f"{lang} {tag}: seed {seed} leaves {float((gap <= 1e-2).mean()):.4f} of the positions masked, backbone std {bb_rel:.4f}, trying the next")
                seed += 1
            p, idx = prob.max(dim=2)
            cs = 1
            while bb[:, ::cs].numel() * 4 > LIMIT // 3:
                cs *= 2
            out = dict(neck=neck.numpy(), idx=idx.numpy().astype(np.int32), prob=p.numpy(), top2gap=gap,
                       backbone=bb[:, ::cs].contiguous().numpy(), backbone_cs=np.int64(cs),
                       top2idx=top2.indices.numpy().astype(np.int32), logits_t0=logits[:, 0, :].contiguous().numpy(),
                       logits_sub=logits[:, :, ::step].contiguous().numpy(),
                       x_seed=np.int64(seed), x_kind=np.array("pm1"), x_shape=np.array(shape, dtype=np.int64))
            if x.nbytes <= LIMIT // 4:
                out["x"] = x
            f = HERE / f"recmv1e_{lang}_seed0_{tag}.npz"
            np.savez_compressed(f, **out)
            assert f.stat().st_size <= LIMIT, (f, f.stat().st_size)
            share = float((gap <= 1e-2).mean())
            key = f"{lang}_{tag}"
            summary["fixtures"][key] = {"masked_share": share, "neck_std_over_T": float(neck.numpy().std(axis=1).mean()),
                                        "backbone_std_over_T_rel": bb_rel, "distinct_argmax": int(len(np.unique(idx.numpy()))),
                                        "backbone_absmax": float(bb.abs().max()), "neck_absmax": float(neck.abs().max()),
                                        "logits_absmax": float(logits.abs().max()), "x_seed": int(seed), "bytes": f.stat().st_size}
            print(key, summary["fixtures"][key])
            assert share <= 0.01, (key, share)
            assert bb_rel >= 0.01, (key, bb_rel)
            assert lang != "korean" or idx.numel() < 80 or len(np.unique(idx.numpy())) >= 5, (key, len(np.unique(idx.numpy())))
        if lang != "korean":
            continue
        # one 200-px line alone and zero-padded to 320
        seed = 777
        while True:
            x200 = make_input((1, 3, 48, 200), seed)
            x320 = np.zeros((1, 3, 48, 320), np.float32)
            x320[..., :200] = x200
            bb_a, neck_a, _, _ = forward(x200)
            bb_b, neck_b, _, _ = forward(x320)
            T = neck_a.shape[1]
            d = (neck_a[0] - neck_b[0, :T]).abs().max(dim=1).values.numpy()
            if d.min() >= 20 * TOL:
                break
            print(f"width pair: seed {seed} leaves d_min {d.min():.4f}, trying the next")
            seed += 1
        f = HERE / "recmv1e_width_pair.npz"
        np.savez_compressed(f, x200=x200, backbone200=bb_a.numpy(), neck200=neck_a.numpy(), backbone320=bb_b.numpy(), neck320=neck_b.numpy(), d=d,
                            x_seed=np.int64(seed))
        assert f.stat().st_size <= LIMIT, f.stat().st_size
        summary["width_pair"] = {"steps": int(T), "d_min": float(d.min()), "d_max": float(d.max()), "x_seed": int(seed), "bytes": f.stat().st_size}
        print("width pair", summary["width_pair"])
        assert d.min() >= 10 * TOL, d.min()

    (HERE / "summary_rec_mv1e.json").write_text(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
