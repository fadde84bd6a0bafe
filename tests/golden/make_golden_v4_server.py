#!/usr/bin/env python3
"""Mint the PP-OCRv4 server fixtures (PPHGNet_small + LKPAN with IntraCL + PFHeadLocal; PPHGNet_small + SVTR neck + CTC) from the
REFERENCE's own nn.Module definitions, with synthetic weights (``rapiddoc_amd.weights``, the opt-in gains of kind "ppocrv4_server").

Runs only in the build container (it imports the reference tree); what it writes next to itself is data only:

    manifest_ppocrv4_det_server.json       weight names / shapes of the reference state dicts (417 and 320 tensors)
    manifest_ppocrv4_rec_server.json
    det4s_seed0_{b2_h64_w96,b1_h160_w224,b3_h96_w352}.npz
                                           the seed / kind / shape that regenerate x, `maps`, the neck output `fuse` and the four backbone
                                           stage outputs stage0 .. stage3.  A tensor that would exceed its share of the size limit of a
                                           committed file is sub-sampled: `<name>_cs` = channel stride, `<name>_ps` = pixel stride along
                                           H and W (odd, so that every row / column parity is met)
    rec4s_seed0_{b2_w64,b3_w104,b2_w100,b3_w320}.npz
                                           the input recipe, the backbone output (every `backbone_cs`-th channel), the neck output, idx, prob,
                                           top2gap (of the softmax probabilities), top2idx, logits_sub (every 61st class), logits_t0
    summary_v4_server.json                 weight checksums; per detector fixture the std of maps and its share inside [0.05, 0.95]; per
                                           recogniser fixture the smallest top-2 probability gap; per HG_Block the min / max / std of the
                                           ESE gate's pre-sigmoid logits over the fixtures of each network

Asserted here: share >= 0.75 and std >= 0.15 per detector fixture; smallest top-2 probability gap >= 1e-2 per recogniser fixture (so the
tests compare the indices at EVERY position); gate-logit std >= 0.5 in every block.  Where a fixture misses, the input seed moves (or the
gains in rapiddoc_amd.weights), never the gate.

    python tests/golden/make_golden_v4_server.py
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
GAINS = "ppocrv4_server"
LIMIT = 1 << 20
MAP_BYTES = 200 << 10
FEAT_BYTES = 160 << 10
STAGE_BYTES = 48 << 10
MIN_SHARE, MIN_STD, MIN_GAP, MIN_GATE_STD = 0.75, 0.15, 1e-2, 0.5
BLOCKS = ("stages.0.blocks.0", "stages.1.blocks.0", "stages.2.blocks.0", "stages.2.blocks.1", "stages.3.blocks.0")


def make_input(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)


def input_seed(tag, shape):
    return 200 + len(tag) + shape[3]


def strides_for(t, budget, max_cs):
    cs, ps = 1, 1
    size = lambda: t[:, ::cs, ::ps, ::ps].numel() * 4
    while size() > budget and cs < min(max_cs, t.shape[1]):
        cs *= 2
    while size() > budget:
        ps += 2
    return cs, ps


def load(arch, name, stem):
    from ppocrv6_pytorch.modeling.architectures.base_model import BaseModel
    net = BaseModel(arch[name])
    man = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in net.state_dict().items()]
    (HERE / f"manifest_{stem}.json").write_text(json.dumps(man))
    state = W.synth_state_dict([(n, tuple(s), d) for n, s, d in man], SEED, kind=GAINS)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    net.eval()
    gate_logits = {b: [] for b in BLOCKS}
    mods = dict(net.backbone.named_modules())
    for b in BLOCKS:
        mods[b + ".att.conv"].register_forward_hook(lambda m, i, o, b=b: gate_logits[b].append(o.detach().flatten().numpy().copy()))
    info = {"checksum": W.checksum(state), "tensors": len(man), "parameters": int(sum(int(np.prod(s)) for n, s, d in man if d == "float32")),
            "fixtures": {}}
    return net, info, gate_logits


def gate_summary(gate_logits):
    out = {}
    for b, chunks in gate_logits.items():
        v = np.concatenate(chunks)
        out[b] = {"min": float(v.min()), "max": float(v.max()), "std": float(v.std())}
        assert out[b]["std"] >= MIN_GATE_STD, (b, out[b])
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    sys.path.insert(0, str(REF / "rapid_doc/model/ocr"))
    arch = yaml.safe_load(open(REF / "rapid_doc/resources/arch_config.yaml"))
    summary = {}

    # ---------------------------------------------------------------------------------------------------------------- detector
    det, info, gates = load(arch, "ch_PP-OCRv4_det_server", "ppocrv4_det_server")
    assert info["tensors"] == 417 and info["parameters"] == 28486083, info
    for tag, shape in (("b2_h64_w96", (2, 3, 64, 96)), ("b1_h160_w224", (1, 3, 160, 224)), ("b3_h96_w352", (3, 3, 96, 352))):
        seed = input_seed(tag, shape)
        while True:
            x = make_input(shape, seed)
            with torch.no_grad():
                xt = torch.from_numpy(x)
                stages = det.backbone(xt)
                fuse = det.neck(stages)
                maps = det(xt)["maps"]
            share = float(((maps >= 0.05) & (maps <= 0.95)).float().mean())
            std = float(maps.double().std())
            if share >= MIN_SHARE and std >= MIN_STD:
                break
            print(f"{tag}: seed {seed} gives share {share:.3f} std {std:.3f}, trying the next")
            seed += 1
        out = dict(x_seed=np.int64(seed), x_kind=np.array("pm1"), x_shape=np.array(shape, dtype=np.int64))
        _, mps = strides_for(maps, MAP_BYTES, 1)
        out["maps"] = maps[:, :, ::mps, ::mps].contiguous().numpy()
        out["maps_ps"] = np.int64(mps)
        feats = [("fuse", fuse, FEAT_BYTES)] + [(f"stage{i}", s, STAGE_BYTES) for i, s in enumerate(stages)]
        for name, t, budget in feats:
            cs, ps = strides_for(t, budget, 8)
            out[name] = t[:, ::cs, ::ps, ::ps].contiguous().numpy()
            out[name + "_cs"] = np.int64(cs)
            out[name + "_ps"] = np.int64(ps)
        fn = HERE / f"det4s_seed0_{tag}.npz"
        np.savez_compressed(fn, **out)
        assert fn.stat().st_size <= LIMIT, (fn, fn.stat().st_size)
        info["fixtures"][tag] = {"x_seed": int(seed), "fuse_absmax": float(fuse.abs().max()), "stage_absmax": [float(s.abs().max()) for s in stages],
                                 "maps_std": std, "maps_share_05_95": share, "maps_min": float(maps.min()), "maps_max": float(maps.max()),
                                 "bytes": fn.stat().st_size}
        print(tag, info["fixtures"][tag])
    info["gate_logits"] = gate_summary(gates)
    summary["det"] = info

    # ---------------------------------------------------------------------------------------------------------------- recogniser
    rec, info, gates = load(arch, "ch_PP-OCRv4_rec_server", "ppocrv4_rec_server")
    assert info["tensors"] == 320 and info["parameters"] == 24184473, info
    for tag, shape in (("b2_w64", (2, 3, 48, 64)), ("b3_w104", (3, 3, 48, 104)), ("b2_w100", (2, 3, 48, 100)), ("b3_w320", (3, 3, 48, 320))):
        seed = input_seed(tag, shape)
        while True:
            x = make_input(shape, seed)
            with torch.no_grad():
                bb = rec.backbone(torch.from_numpy(x))
                neck = rec.head.ctc_encoder(bb)
                logits = rec.head.ctc_head.fc(neck)
                prob = rec.head(bb)
            assert float((torch.softmax(logits, dim=2) - prob).abs().max()) == 0.0
            top2 = torch.topk(prob, 2, dim=2)
            gap = (top2.values[..., 0] - top2.values[..., 1]).numpy()
            if float(gap.min()) >= MIN_GAP:
                break
            print(f"{tag}: seed {seed} gives a smallest top-2 gap of {float(gap.min()):.4f}, trying the next")
            seed += 1
        p, idx = prob.max(dim=2)
        cs = 1
        while bb[:, ::cs].numel() * 4 > LIMIT // 3:
            cs *= 2
        out = dict(neck=neck.numpy(), idx=idx.numpy().astype(np.int32), prob=p.numpy(), top2gap=gap, top2idx=top2.indices.numpy().astype(np.int32),
                   logits_t0=logits[:, 0, :].contiguous().numpy(), logits_sub=logits[:, :, ::61].contiguous().numpy(),
                   backbone=bb[:, ::cs].contiguous().numpy(), backbone_cs=np.int64(cs),
                   x_seed=np.int64(seed), x_kind=np.array("pm1"), x_shape=np.array(shape, dtype=np.int64))
        fn = HERE / f"rec4s_seed0_{tag}.npz"
        np.savez_compressed(fn, **out)
        assert fn.stat().st_size <= LIMIT, (fn, fn.stat().st_size)
        info["fixtures"][tag] = {"x_seed": int(seed), "tokens": int(bb.shape[3]), "min_top2_gap": float(gap.min()),
                                 "distinct_argmax": int(len(np.unique(idx.numpy()))), "backbone_absmax": float(bb.abs().max()),
                                 "neck_absmax": float(neck.abs().max()), "logits_absmax": float(logits.abs().max()), "bytes": fn.stat().st_size}
        print(tag, info["fixtures"][tag])
        assert info["fixtures"][tag]["min_top2_gap"] >= MIN_GAP
    info["gate_logits"] = gate_summary(gates)
    summary["rec"] = info
    summary["gates"] = {"min_share": MIN_SHARE, "min_std": MIN_STD, "min_top2_gap": MIN_GAP, "min_gate_logit_std": MIN_GATE_STD}
    (HERE / "summary_v4_server.json").write_text(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
