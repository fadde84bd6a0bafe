#!/usr/bin/env python3
"""Microbenchmark of the UniTable table-structure encoder (`unitable_encoder`; bench.py measures the default page path, which has no table
network, and stays as it is).

The forward at [B, 3, 448, 448] (T = 784 tokens per table), B = 1 and 8, in the `auto` and `fp32` precisions, against a plain torch fp32
restatement of the same graph (torch.matmul / softmax / layer_norm / gelu) on the same GPU, same weights and input, in the same process:
the three run in turn (alternating), `--warmup` untimed rounds and then `--steps` timed ones of `iters` forwards each between two HIP
events on a stream of the tool's own (the engine replays the plan's hipGraph there, as a pipeline would).  Per contender the median ms per
forward and the spread (max - min) / median; the largest |engine - torch| of `memory`.  Then the per-op-kind table of one profiled
`auto` launch (HIP events around every op, launch gaps included) and the plan's workspace size.

Then the decoder (`unitable_decoder`): ms per decode step at B = 1 and 8, at S = 784 and at S = 6 (the difference is what the cross-attention
over `memory` costs), against a KV-cached plain torch fp32 step on the same GPU, and the weight bytes the step streams per second.

    python tools/mb_unitable.py [--steps 7] [--warmup 3] > profiles/mb_unitable.txt
"""
import argparse
import os
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from rapiddoc_amd import weights as W  # noqa: E402
from rapiddoc_amd.engine import RdEngine  # noqa: E402

KIND = "unitable_encoder"
GOLDEN = ROOT / "tests" / "golden"
D, HEADS, HD, LAYERS = 768, 12, 64, 12


def med_spread(v):
    v = np.asarray(v, dtype=np.float64)
    m = float(np.median(v))
    return m, float((v.max() - v.min()) / m) if m > 0 else 0.0


def engine_for(state, precision):
    old = os.environ.get("RD_PRECISION")
    os.environ["RD_PRECISION"] = precision
    try:
        return RdEngine(KIND, guard="off", reuse_outputs=True).load_weights(state)
    finally:
        if old is None:
            os.environ.pop("RD_PRECISION", None)
        else:
            os.environ["RD_PRECISION"] = old


class TorchEncoder:
    """the same graph in plain torch fp32 on the device"""

    def __init__(self, state):
        self.w = {k: torch.from_numpy(v).cuda() for k, v in state.items()}
        self.w["patch"] = self.w["backbone.conv_proj.weight"].reshape(D, -1).T.contiguous()

    @torch.no_grad()
    def __call__(self, x):
        w = self.w
        B, C, H, W_ = x.shape
        t = x.reshape(B, C, H // 16, 16, W_ // 16, 16).permute(0, 2, 4, 1, 3, 5).reshape(B, -1, C * 256) @ w["patch"] + w["backbone.conv_proj.bias"]
        T = t.shape[1]
        t = t + w["pos_embed.embedding.weight"][:T]
        for i in range(LAYERS):
            p = f"encoder.layers.{i}."
            y = F.layer_norm(t, (D,), w[p + "norm1.weight"], w[p + "norm1.bias"], 1e-5)
            r = (y @ w[p + "self_attn.in_proj_weight"].T + w[p + "self_attn.in_proj_bias"]).reshape(B, T, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
            a = (torch.softmax((r[0] * 0.125) @ r[1].transpose(-1, -2), dim=-1) @ r[2]).permute(0, 2, 1, 3).reshape(B, T, D)
            t = t + a @ w[p + "self_attn.out_proj.weight"].T + w[p + "self_attn.out_proj.bias"]
            y = F.layer_norm(t, (D,), w[p + "norm2.weight"], w[p + "norm2.bias"], 1e-5)
            t = t + F.gelu(y @ w[p + "linear1.weight"].T + w[p + "linear1.bias"]) @ w[p + "linear2.weight"].T + w[p + "linear2.bias"]
        return F.layer_norm(t, (D,), w["norm.weight"], w["norm.bias"], 1e-6)


def timed(fn, x, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn(x)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


class TorchDecoder:
    """GPTFastDecoder's step in plain torch fp32 on the device, KV-cached: the yardstick of the decode step"""

    def __init__(self, state, memory):
        self.w = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in state.items()}
        B, S, _ = memory.shape
        self.B = B
        lin = self.lin
        self.ck = [lin(memory, f"layers.{i}.multihead_attn.key").reshape(B, S, HEADS, HD).transpose(1, 2) for i in range(4)]
        self.cv = [lin(memory, f"layers.{i}.multihead_attn.value").reshape(B, S, HEADS, HD).transpose(1, 2) for i in range(4)]
        self.kc = [torch.zeros((B, HEADS, 1024, HD), device="cuda") for _ in range(4)]
        self.vc = [torch.zeros((B, HEADS, 1024, HD), device="cuda") for _ in range(4)]

    def lin(self, x, p):
        return x @ self.w[p + ".weight"].T + self.w[p + ".bias"]

    @torch.no_grad()
    def step(self, tok, pos):
        w, B = self.w, self.B
        x = w["token_embed.embedding.weight"][tok] + w["pos_embed.embedding.weight"][pos]
        ln = lambda t, p: F.layer_norm(t, (D,), w[p + ".weight"], w[p + ".bias"], 1e-5)
        for i in range(4):
            p = f"layers.{i}."
            q, k, v = self.lin(ln(x, p + "norm1"), p + "self_attn.wqkv").split(D, dim=-1)
            self.kc[i][:, :, pos] = k.reshape(B, HEADS, HD)
            self.vc[i][:, :, pos] = v.reshape(B, HEADS, HD)
            a = torch.softmax((q.reshape(B, HEADS, 1, HD) * 0.125) @ self.kc[i][:, :, :pos + 1].transpose(-1, -2), dim=-1) @ self.vc[i][:, :, :pos + 1]
            x = x + self.lin(a.reshape(B, D), p + "self_attn.wo")
            q = self.lin(ln(x, p + "norm2"), p + "multihead_attn.query")
            a = torch.softmax((q.reshape(B, HEADS, 1, HD) * 0.125) @ self.ck[i].transpose(-1, -2), dim=-1) @ self.cv[i]
            x = x + self.lin(a.reshape(B, D), p + "multihead_attn.out")
            x = x + self.lin(F.gelu(self.lin(ln(x, p + "norm3"), p + "linear1")), p + "linear2")
        return self.lin(x, "generator")


def decode_timing(args):
    """ms per decode step: rd_debug_table_decode with forced tokens (no early stop) at 16 and at 80 steps on a stream of the tool's own (the
    step replays as one hipGraph there); per step = (t80 - t16) / 64, which takes the once-per-batch K / V projections and the capture out"""
    import time
    from rapiddoc_amd.table_unitable import STAND_IN_IDS as IDS
    dstate = W.synth_state_dict(W.load_manifest(GOLDEN / "manifest_unitable_decoder.json"), 0)
    dec = RdEngine("unitable_decoder").load_weights(dstate)
    side = torch.cuda.Stream()
    rng = np.random.default_rng(0)
    print(f"== decode step (4 blocks, generator, select; 47 launches, 160 MB of fp32 weights streamed per step), forced tokens, alternating, "
          f"{args.warmup} warm-up + {args.steps} timed rounds")
    for S in (784, 6):
        for B in (1, 8):
            memory = torch.from_numpy(W.synth_memory(3, B, S)).cuda()
            forced = torch.from_numpy(rng.integers(12, 510, (B, 80)).astype(np.int32)).cuda()
            td = TorchDecoder(dstate, memory)
            t = {"engine": [], "torch": []}
            with torch.cuda.stream(side):
                for r in range(args.warmup + args.steps):
                    ms = []
                    for n in (16, 80):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        out = dec.table_decode_debug(memory, IDS, n, forced=forced[:, :n].contiguous())
                        torch.cuda.synchronize()
                        ms.append((time.perf_counter() - t0) * 1e3)
                    for pos in range(16):          # (untimed: fills the yardstick's cache rows 0 .. 15)
                        td.step(forced[:, pos].long(), pos)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for pos in range(16, 80):
                        lg = td.step(forced[:, pos].long(), pos)
                    e1.record()
                    e1.synchronize()
                    if r >= args.warmup:
                        t["engine"].append((ms[1] - ms[0]) / 64)
                        t["torch"].append(e0.elapsed_time(e1) / 64)
            side.synchronize()
            diff = float((out["logits"][79] - lg).abs().max())
            (me, se), (mt, st_) = med_spread(t["engine"]), med_spread(t["torch"])
            print(f"S {S:3d} B {B}  engine {me:7.4f} ms/step (spread {100 * se:4.1f} %, {160.3 / me:6.1f} GB/s of weights)   torch {mt:7.4f} ms/step "
                  f"(spread {100 * st_:4.1f} %)   max |logits - torch| at step 79: {diff:.2e}")
    dec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    print(f"# {torch.cuda.get_device_name(0)}; tools/mb_unitable.py {' '.join(sys.argv[1:])}")
    state = W.synth_state_dict(W.load_manifest(GOLDEN / f"manifest_{KIND}.json"), 0)
    contenders = {"auto": engine_for(state, "auto").table_encoder_forward, "fp32": engine_for(state, "fp32").table_encoder_forward,
                  "torch": TorchEncoder(state)}
    engines = {k: v.__self__ for k, v in contenders.items() if k != "torch"}
    side = torch.cuda.Stream()
    print(f"== encoder forward [B, 3, 448, 448] (T = 784): engine auto / engine fp32 / plain torch fp32, alternating, {args.warmup} warm-up + "
          f"{args.steps} timed rounds")
    for B, iters in ((1, 10), (8, 3)):
        x = torch.from_numpy(W.synth_normal_image(3, B, 448, 448)).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            outs = {}
            for k, fn in contenders.items():
                for _ in range(3):          # build the plan, let the library capture and replay its graph
                    outs[k] = fn(x)
                outs[k] = outs[k].clone()
            t = {k: [] for k in contenders}
            for r in range(args.warmup + args.steps):
                for k, fn in contenders.items():
                    ms = timed(fn, x, iters)
                    if r >= args.warmup:
                        t[k].append(ms)
        side.synchronize()
        flop = B * (2.0 * 784 * 768 * (768 + 12 * (2304 + 768 + 2 * 3072)) + 12 * 4.0 * 12 * 784 * 784 * 64)
        for k in contenders:
            m, s = med_spread(t[k])
            diff = "" if k == "torch" else f"   max |memory - torch| {float((outs[k] - outs['torch']).abs().max()):.2e}"
            print(f"B {B}  {k:6s} {m:8.3f} ms (spread {100 * s:4.1f} %, {iters} forwards per round)   {flop / m / 1e9:6.1f} TFLOP/s{diff}")
        print(f"      workspace (auto): {engines['auto'].workspace_bytes(B, 448, 448) / 2 ** 20:8.1f} MiB")
    for B in (1, 8):
        x = torch.from_numpy(W.synth_normal_image(3, B, 448, 448)).cuda()
        eng = engines["auto"]
        eng.set_profiling(True)
        rounds = []
        for _ in range(args.steps):
            eng.profile_log.clear()
            eng.table_encoder_forward(x)
            rounds.append(list(eng.profile_log))
        eng.set_profiling(False)
        kinds = {}
        for log in rounds:
            per = {}
            for r in log:
                k = r["kind"] + ("/h3" if r["cfg"].endswith("/h3") else "")
                per.setdefault(k, [0, 0.0])
                per[k][0] += 1
                per[k][1] += r["ms"]
            for k, (n, ms) in per.items():
                kinds.setdefault(k, (n, []))[1].append(ms)
        total = sum(float(np.median(v)) for _n, v in kinds.values())
        print(f"-- auto, per op kind, B {B} (profiled launches: HIP events around every op, median of {args.steps}); sum {total:.3f} ms over "
              f"{sum(n for n, _v in kinds.values())} ops")
        for k, (n, v) in sorted(kinds.items(), key=lambda kv: -np.median(kv[1][1])):
            print(f"   {k:16s} {n:3d} ops   {np.median(v):8.4f} ms   {100 * np.median(v) / total:5.1f} %")
    for e in engines.values():
        e.close()
    print()
    decode_timing(args)


if __name__ == "__main__":
    main()
