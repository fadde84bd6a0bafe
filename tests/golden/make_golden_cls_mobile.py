#!/usr/bin/env python3
"""Mint the text-line direction classifier fixtures (ch_ptocr_mobile_v2.0_cls_mobile: MobileNetV3 small scale 0.35 + ClsHead) from the
REFERENCE's own nn.Module definitions, with synthetic weights (``rapiddoc_amd.weights``, gains and bias offsets of kind ``ppocr_cls_mobile``).

Runs only in the build container (it imports the reference tree); what it writes next to itself is data only:

    manifest_ppocr_cls_mobile.json     weight names / shapes of the reference state dict (248 tensors)
    cls_seed0_{b7_h48_w192,b1_h48_w192,b3_h40_w100}.npz
                                       the recipe that regenerates x (``weights.synth_cls_lines(x_seed, B, H, W)``: ragged content widths
                                       12 ... W with zero right-padding, brightness and contrast per line), the content widths, `prob`
                                       [B,2], `logits` [B,2], the pooled features `feat` [B,200] and the outputs of blocks 0, 3, 8, 10
                                       (`b0`, `b3`, `b8`, `b10`, NCHW)
    summary_cls_mobile.json            the weight checksum; per fixture the probabilities; `draw48`: p1 of a 48-line draw
                                       (synth_cls_lines(DRAW_SEED, 48)); `left_out`: the lines of either set within 1e-3 of 0.5 or of 0.9 -
                                       the only lines a decision test may leave out

The generator asserts, over the 7-line fixture plus the 48-line draw: at least a quarter of the lines on each side of p1 = 0.5, at least
three label-1 lines on each side of 0.9, at most 10 % of the lines left out.  Where a draw misses, the seed or the gains move, never the caps.

    python tests/golden/make_golden_cls_mobile.py
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
DRAW_SEED = 0
KIND = "ppocr_cls_mobile"
ARCH = "ch_ptocr_mobile_v2.0_cls_mobile"
LIMIT = 1 << 20
THRESH, NEAR = 0.9, 1e-3
TAPS = {"b0": 0, "b3": 3, "b8": 8, "b10": 10}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    sys.path.insert(0, str(REF / "rapid_doc/model/ocr"))
    from ppocrv6_pytorch.modeling.architectures.base_model import BaseModel

    arch = yaml.safe_load(open(REF / "rapid_doc/resources/arch_config.yaml"))
    net = BaseModel(arch[ARCH])
    man = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in net.state_dict().items()]
    (HERE / f"manifest_{KIND}.json").write_text(json.dumps(man))
    state = W.synth_state_dict([(n, tuple(s), d) for n, s, d in man], SEED, kind=KIND)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    net.eval()
    summary = {"checksum": W.checksum(state), "tensors": len(man), "parameters": int(sum(p.numel() for p in net.parameters())),
               "thresh": THRESH, "near": NEAR, "fixtures": {}}

    got = {}
    for name, i in TAPS.items():
        net.backbone.blocks[i].register_forward_hook(lambda m, a, o, name=name: got.__setitem__(name, o.detach().clone()))
    net.head.fc.register_forward_hook(lambda m, a, o: got.__setitem__("logits", o.detach().clone()))
    net.head.fc.register_forward_pre_hook(lambda m, a: got.__setitem__("feat", a[0].detach().clone()))

    def forward(x):
        with torch.no_grad():
            out = net(torch.from_numpy(x))
        prob = out if torch.is_tensor(out) else next(iter(out.values()))
        assert prob.shape == (x.shape[0], 2)
        assert float((torch.softmax(got["logits"], dim=1) - prob).abs().max()) == 0.0
        return prob.numpy()

    def near(p1):
        return [int(i) for i in np.flatnonzero((np.abs(p1 - 0.5) <= NEAR) | (np.abs(p1 - THRESH) <= NEAR))]

    for tag, shape in (("b7_h48_w192", (7, 48, 192)), ("b1_h48_w192", (1, 48, 192)), ("b3_h40_w100", (3, 40, 100))):
        x, widths = W.synth_cls_lines(SEED, *shape)
        prob = forward(x)
        out = dict(x_seed=np.int64(SEED), x_kind=np.array("cls_lines"), x_shape=np.array((shape[0], 3, shape[1], shape[2]), dtype=np.int64),
                   widths=widths, prob=prob, logits=got["logits"].numpy(), feat=got["feat"].numpy())
        for name in TAPS:
            out[name] = got[name].numpy()
        fn = HERE / f"cls_seed0_{tag}.npz"
        np.savez_compressed(fn, **out)
        assert fn.stat().st_size <= LIMIT, (fn, fn.stat().st_size)
        summary["fixtures"][tag] = {"prob": prob.tolist(), "logit_absmax": float(got["logits"].abs().max()), "feat_absmax": float(got["feat"].abs().max()),
                                    "block_absmax": {n: float(got[n].abs().max()) for n in TAPS}, "left_out": near(prob[:, 1]),
                                    "bytes": fn.stat().st_size}
        print(tag, summary["fixtures"][tag])

    x48, _ = W.synth_cls_lines(DRAW_SEED, 48, 48, 192)
    p48 = forward(x48)[:, 1]
    summary["draw48"] = {"x_seed": DRAW_SEED, "p1": p48.tolist(), "left_out": near(p48)}
    p1 = np.concatenate([np.asarray(summary["fixtures"]["b7_h48_w192"]["prob"])[:, 1], p48])
    n = p1.size
    lo, hi = int((p1 < 0.5).sum()), int((p1 > 0.5).sum())
    under, over = int(((p1 > 0.5) & (p1 < THRESH)).sum()), int((p1 >= THRESH).sum())
    left = len(summary["fixtures"]["b7_h48_w192"]["left_out"]) + len(summary["draw48"]["left_out"])
    summary["spread"] = {"lines": n, "label0": lo, "label1": hi, "label1_below_thresh": under, "label1_at_or_above_thresh": over, "left_out": left}
    print(summary["spread"])
    assert lo * 4 >= n and hi * 4 >= n, (lo, hi, n)
    assert under >= 3 and over >= 3, (under, over)
    assert left * 10 <= n, (left, n)
    (HERE / "summary_cls_mobile.json").write_text(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
