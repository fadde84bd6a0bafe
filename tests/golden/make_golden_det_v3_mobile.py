#!/usr/bin/env python3
"""Mint the PP-OCRv3 multilingual detector fixtures (MobileNetV3 large scale 0.5 without SE + RSEFPN 96 + DBHead) from the REFERENCE's own nn.Module
definitions, with synthetic weights (``rapiddoc_amd.weights``, gains of kind ``ppocrv3_det_mobile``).

Runs only in the build container (it imports the reference tree); what it writes next to itself is data only:

    manifest_ppocrv3_det_mobile.json       weight names / shapes of the reference state dict
    det3m_seed0_{b2_h64_w96,b1_h160_w224,b3_h96_w352,b1_h960_w704}.npz
                                           the seed / kind / shape that regenerate x, `maps`, the pre-sigmoid map (shrink_logit), the
                                           neck output `fuse` and the backbone's four stage features `stage0` .. `stage3`.  A tensor that would exceed its share of the size limit of a committed
                                           file is sub-sampled: `<name>_cs` = channel stride, `<name>_ps` = pixel stride along H and W
                                           (odd, so that every row / column parity is met)
    summary_det_v3_mobile.json                the weight checksum; per fixture the abs-max of fuse and of the four stage features, the std of
                                           maps and the share of maps inside [0.05, 0.95]

The generator asserts share >= 0.75, std >= 0.15 and sigmoid(shrink_logit) == maps per fixture.  Where a fixture misses, the input seed
moves (or the gains in weights._KIND_GAINS), never the cap.

    python tests/golden/make_golden_det_v3_mobile.py
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
KIND = "ppocrv3_det_mobile"
ARCH = "multi_PP-OCRv3_det_mobile"     # en_PP-OCRv3_det_mobile is the same graph
LIMIT = 1 << 20
MAP_BYTES = 220 << 10        # maps, shrink_logit
FEAT_BYTES = 200 << 10       # fuse
STAGE_BYTES = 60 << 10       # each of the four stage features
MIN_SHARE, MIN_STD = 0.75, 0.15


def make_input(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)


def strides_for(t, budget, max_cs):
    """(channel stride, pixel stride) that bring t [B,C,H,W] under `budget` bytes: channels first (powers of two), then odd pixel strides"""
    cs, ps = 1, 1
    size = lambda: t[:, ::cs, ::ps, ::ps].numel() * 4
    while size() > budget and cs < min(max_cs, t.shape[1]):
        cs *= 2
    while size() > budget:
        ps += 2
    return cs, ps


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    sys.path.insert(0, str(REF / "rapid_doc/model/ocr"))
    from ppocrv6_pytorch.modeling.architectures.base_model import BaseModel

    arch = yaml.safe_load(open(REF / "rapid_doc/resources/arch_config.yaml"))
    det = BaseModel(arch[ARCH])
    man = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in det.state_dict().items()]
    (HERE / f"manifest_{KIND}.json").write_text(json.dumps(man))
    state = W.synth_state_dict([(n, tuple(s), d) for n, s, d in man], SEED, kind=KIND)
    det.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    det.eval()
    summary = {"checksum": W.checksum(state), "tensors": len(man), "parameters": int(sum(p.numel() for p in det.parameters())), "fixtures": {}}

    def forward(x):
        with torch.no_grad():
            xt = torch.from_numpy(x)
            feats = det.backbone(xt)
            fuse = det.neck(feats)
            _, f = det.head.binarize(fuse, return_f=True)
            shrink_logit = det.head.binarize.conv3(f)
            maps = det(xt)["maps"]
        assert float((torch.sigmoid(shrink_logit) - maps).abs().max()) == 0.0
        return feats, fuse, shrink_logit, maps

    for tag, shape in (("b2_h64_w96", (2, 3, 64, 96)), ("b1_h160_w224", (1, 3, 160, 224)), ("b3_h96_w352", (3, 3, 96, 352)),
                       ("b1_h960_w704", (1, 3, 960, 704))):
        seed = 300 + shape[3]
        while True:
            x = make_input(shape, seed)
            feats, fuse, shrink_logit, maps = forward(x)
            share = float(((maps >= 0.05) & (maps <= 0.95)).float().mean())
            std = float(maps.double().std())
            if share >= MIN_SHARE and std >= MIN_STD:
                break
            print(f"{tag}: seed {seed} gives share {share:.3f} std {std:.3f}, trying the next")
            seed += 1
        out = dict(x_seed=np.int64(seed), x_kind=np.array("pm1"), x_shape=np.array(shape, dtype=np.int64))
        _, mps = strides_for(maps, MAP_BYTES, 1)
        for name, t in (("maps", maps), ("shrink_logit", shrink_logit)):
            out[name] = t[:, :, ::mps, ::mps].contiguous().numpy()
        out["maps_ps"] = np.int64(mps)
        cs, ps = strides_for(fuse, FEAT_BYTES, 4)
        out["fuse"] = fuse[:, ::cs, ::ps, ::ps].contiguous().numpy()
        out["fuse_cs"] = np.int64(cs)
        out["fuse_ps"] = np.int64(ps)
        for i, f in enumerate(feats):
            cs, ps = strides_for(f, STAGE_BYTES, 8)
            out[f"stage{i}"] = f[:, ::cs, ::ps, ::ps].contiguous().numpy()
            out[f"stage{i}_cs"] = np.int64(cs)
            out[f"stage{i}_ps"] = np.int64(ps)
        fn = HERE / f"det3m_seed0_{tag}.npz"
        np.savez_compressed(fn, **out)
        assert fn.stat().st_size <= LIMIT, (fn, fn.stat().st_size)
        summary["fixtures"][tag] = {"x_seed": int(seed), "fuse_absmax": float(fuse.abs().max()),
                                    "stage_absmax": [float(f.abs().max()) for f in feats],
                                    "maps_std": std, "maps_share_05_95": share, "maps_min": float(maps.min()), "maps_max": float(maps.max()),
                                    "shrink_logit_absmax": float(shrink_logit.abs().max()), "bytes": fn.stat().st_size}
        print(tag, summary["fixtures"][tag])
        assert share >= MIN_SHARE and std >= MIN_STD, (tag, share, std)

    (HERE / "summary_det_v3_mobile.json").write_text(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
