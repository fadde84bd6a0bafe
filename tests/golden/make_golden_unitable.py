#!/usr/bin/env python3
"""Mint the UniTable encoder fixtures (table-structure recogniser: ViT-B encoder, 12 pre-norm nn.TransformerEncoderLayer of d = 768,
12 heads of 64, FFN 3072, patch 16) from the REFERENCE's own nn.Module definition (``unitable_modules.py``, imported by file path: it
needs nothing else of the package), with the plain synthetic weights of ``rapiddoc_amd.weights`` (no gains: the encoder is alive under
the plain rule, `memory` absmax about 4, std 1).

Runs only in the build container (it imports the reference tree); what it writes next to itself is data only:

    manifest_unitable_encoder.json     weight names / shapes of the reference state dict (149 tensors, 86 433 024 parameters)
    unitable_enc_seed0_{b1_h32_w48,b2_h48_w208,b1_h64_w272,b1_h448_w448}.npz
                                       the recipe that regenerates x (``weights.synth_normal_image(x_seed, B, H, W)``) and four taps as
                                       [B, T, 768] token rows: `patch` (conv_proj, flattened), `layer0`, `layer11` (the outputs of encoder
                                       layers 0 and 11) and `memory` (after the final LayerNorm).  A tap that does not fit the size
                                       limit of a committed file is sub-sampled: `<tap>_ts` = token stride (odd), `<tap>_cs` = channel
                                       stride; the stored array is tap[:, ::ts, ::cs]
    summary_unitable.json              the weight checksum and per fixture the absmax / std of every tap; under "decoder" the decoder's
                                       figures, the recorded outputs of the reference's host functions ("host") and the expected ids,
                                       html and boxes of the whole chain on a 448 x 448 input ("class448")
    manifest_unitable_decoder.json     GPTFastDecoder's state dict (92 tensors, 40 069 056 parameters)
    unitable_dec_seed0_{free_s6,free_s784,forced_s39,bbox_s6,eos_b3_s6}.npz
                                       per decode step the hidden row after each block, the logits, the chosen id, the whitelist top-2
                                       gap and the `compare` mask (mint_decoder below)

Which ids a test may compare.  Step tests feed the reference's own tokens and compare the chosen id only where `compare` holds: whitelist
top-2 gap >= 10 x the logit bound 1e-3 max(1, max|logit|).  The LOOP fixtures (eos_b3_s6, class448) are compared id by id over the whole
free run, lengths included, under a rule of their own, which the search enforces before it accepts an input seed (LOOP_RULES): EOS at
least 0.25 away from winning or losing at every step and every other decision on the way at least 0.05 wide or, where no offset of the
seed gives that, 0.1 and 0.02.  The engine's logit error is 1e-5 (measured, docs/notebook/unitable.md), so 0.02 is 2000 times what could
flip a decision; the 10 x bound rule (0.2 here) left no seed among sixty whose three tables stop at three different steps.

T = (H / 16) (W / 16): 6, 39, 68 (crosses a 64-key tile of the attention kernel) and 784 (the product shape 448 x 448).

    python tests/golden/make_golden_unitable.py
"""
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
REF = Path("/root/reference")
MODULES = REF / "rapid_doc/model/table/rapid_table_self/table_structure/unitable/unitable_modules.py"

from rapiddoc_amd import weights as W  # noqa: E402

SEED = 0
X_SEED = 3
KIND = "unitable_encoder"
LIMIT = 1 << 20
TAP_BYTES = 200 << 10            # per tap, before compression (random floats barely compress)
SHAPES = ((1, 32, 48), (2, 48, 208), (1, 64, 272), (1, 448, 448))
TAPS = ("patch", "layer0", "layer11", "memory")


def strides_for(t):
    """(token stride, channel stride) that bring t [B, T, C] under TAP_BYTES: channels first (1, 2, 3), then odd token strides"""
    ts, cs = 1, 1
    size = lambda: t[:, ::ts, ::cs].numel() * 4
    while size() > TAP_BYTES and cs < 3:
        cs += 1
    while size() > TAP_BYTES:
        ts += 2
    return ts, cs


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    spec = importlib.util.spec_from_file_location("unitable_modules_ref", MODULES)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = mod.Encoder()
    man = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in net.state_dict().items()]
    (HERE / f"manifest_{KIND}.json").write_text(json.dumps(man))
    state = W.synth_state_dict([(n, tuple(s), d) for n, s, d in man], SEED)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    net.eval()
    summary = {"checksum": W.checksum(state), "tensors": len(man), "parameters": int(sum(p.numel() for p in net.parameters())),
               "x_seed": X_SEED, "fixtures": {}}

    got = {}
    net.backbone.register_forward_hook(lambda m, a, o: got.__setitem__("patch", o.detach().clone()))
    net.encoder.layers[0].register_forward_hook(lambda m, a, o: got.__setitem__("layer0", o.detach().clone()))
    net.encoder.layers[11].register_forward_hook(lambda m, a, o: got.__setitem__("layer11", o.detach().clone()))

    for B, H, Wd in SHAPES:
        x = W.synth_normal_image(X_SEED, B, H, Wd)
        with torch.no_grad():
            got["memory"] = net(torch.from_numpy(x))
        T = (H // 16) * (Wd // 16)
        out = dict(x_seed=np.int64(X_SEED), x_kind=np.array("normal_image"), x_shape=np.array((B, 3, H, Wd), dtype=np.int64))
        stats = {}
        for name in TAPS:
            t = got[name]
            assert t.shape == (B, T, 768), (name, t.shape)
            ts, cs = strides_for(t)
            out[name] = t[:, ::ts, ::cs].contiguous().numpy()
            out[name + "_ts"], out[name + "_cs"] = np.int64(ts), np.int64(cs)
            stats[name] = {"absmax": float(t.abs().max()), "std": float(t.std()), "ts": ts, "cs": cs}
        tag = f"b{B}_h{H}_w{Wd}"
        fn = HERE / f"unitable_enc_seed0_{tag}.npz"
        np.savez_compressed(fn, **out)
        assert fn.stat().st_size <= LIMIT, (fn, fn.stat().st_size)
        summary["fixtures"][tag] = {"T": T, "taps": stats, "bytes": fn.stat().st_size}
        print(tag, summary["fixtures"][tag])
        assert stats["memory"]["std"] > 0.5, "the encoder's output is not alive"
    summary["decoder"] = mint_decoder(mod, net)
    (HERE / "summary_unitable.json").write_text(json.dumps(summary, indent=1))


# ---------------------------------------------------------------------------------------------------------------- decoder
DEC_KIND = "unitable_decoder"
MEM_SEED = 3
LOOP_RULES = ((0.25, 0.05), (0.1, 0.02))     # (EOS margin, width of every other decision) a loop fixture's seed must give: the first that any offset meets
GAP_FACTOR = 10.0            # every compared id: whitelist top-2 gap >= 10 x the logit bound 1e-3 max(1, max|logit|)


def whitelist_gap(logits, white):
    v = np.sort(logits[..., white], axis=-1)
    return v[..., -1] - v[..., -2]


def mint_decoder(mod, enc):
    """Decoder fixtures unitable_dec_seed0_*.npz, from GPTFastDecoder itself (one table at a time, as the reference decodes) and the loop
    of main.py restated around it (`table_unitable.loop_reference`; the class there needs the vocabulary file).  Per step: `hidden`
    [steps, 4, B, 768 / 4] = the row after each block (channel stride 4), `logits` [steps, B, 960] as the generator wrote them,
    `chosen` = the whitelist argmax, `ids` = the loop's context, `gap` = the whitelist top-2 gap.  Ids: table_unitable.STAND_IN_IDS."""
    from rapiddoc_amd import table_unitable as TU
    ids = TU.STAND_IN_IDS
    dec = mod.GPTFastDecoder()
    man = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in dec.state_dict().items()]
    (HERE / f"manifest_{DEC_KIND}.json").write_text(json.dumps(man))
    base = W.synth_state_dict([(n, tuple(s), d) for n, s, d in man], SEED)
    white = np.array(sorted(dec.token_white_list))
    assert white.tolist() == [1] + list(range(12, 510))
    got = {}
    for i, layer in enumerate(dec.layers):
        layer.register_forward_hook(lambda m, a, o, i=i: got.__setitem__(i, o.detach()[:, -1].clone()))
    dec.generator.register_forward_hook(lambda m, a, o: got.__setitem__("logits", o.detach()[:, -1].clone()))
    dec.eval()

    def load(state):
        dec.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)

    def run(memory, steps, forced=None):
        """one table; returns (context, hidden [n,4,768], logits [n,960], chosen [n])"""
        dec.setup_caches(max_batch_size=1, max_seq_length=1024, dtype=torch.float32, device="cpu")
        mem = torch.from_numpy(memory)[None]
        hid, lg, ch = [], [], []

        def next_token(ctx):
            with torch.no_grad():
                t = int(dec(mem, torch.tensor([ctx], dtype=torch.int32))[0, 0])
            hid.append(torch.stack([got[i][0] for i in range(4)]).numpy())
            lg.append(got["logits"][0].numpy())
            ch.append(t)
            return t
        if forced is not None:
            ctx = []
            for t in forced:
                ctx.append(int(t))
                next_token(ctx)
            ctx = [int(forced[0])]
        else:
            ctx = TU.loop_reference(next_token, ids, steps)
        return ctx, np.stack(hid), np.stack(lg), np.array(ch, dtype=np.int32)

    out_summary = {"tensors": len(man), "parameters": int(sum(p.numel() for p in dec.parameters())), "checksum": W.checksum(base), "runs": {}}

    def save(tag, tables, steps, extra, need_all=False):
        """tables: list of run() results; padded to `steps` rows with NaN / -1 behind a table's EOS"""
        B = len(tables)
        hidden = np.full((steps, 4, B, 192), np.nan, dtype=np.float32)
        logits = np.full((steps, B, 960), np.nan, dtype=np.float32)
        chosen = np.full((steps, B), -1, dtype=np.int32)
        ctxs = np.full((B, steps + 1), -1, dtype=np.int64)
        for b, (ctx, h, l, c) in enumerate(tables):
            n = len(c)
            hidden[:n, :, b], logits[:n, b], chosen[:n, b] = h[:, :, ::4], l, c
            ctxs[b, :len(ctx)] = ctx
        gap = whitelist_gap(logits, white)
        bound = 1e-3 * max(1.0, float(np.nanmax(np.abs(logits))))
        fn = HERE / f"unitable_dec_seed0_{tag}.npz"
        compare = np.nan_to_num(gap, nan=0.0) >= GAP_FACTOR * bound       # the steps whose chosen id a test may compare
        np.savez_compressed(fn, hidden=hidden, logits=logits, chosen=chosen, ids=ctxs, gap=gap.astype(np.float32), compare=compare,
                            mem_seed=np.int64(MEM_SEED), **extra)
        assert fn.stat().st_size <= LIMIT, (fn, fn.stat().st_size)
        mg = float(np.nanmin(gap))
        out_summary["runs"][tag] = {"steps": steps, "B": B, "min_gap": mg, "logit_absmax": float(np.nanmax(np.abs(logits))), "distinct_ids": int(len(set(chosen[chosen >= 0].tolist()))),
                                    "lengths": [len(t[0]) for t in tables], "bytes": fn.stat().st_size}
        print(tag, out_summary["runs"][tag])
        out_summary["runs"][tag]["compared_steps"] = int(compare.sum())
        ran = chosen >= 0
        assert compare.sum() * 2 >= ran.sum(), (tag, int(compare.sum()), int(ran.sum()))
        if need_all:
            assert bool(compare[ran].all()), (tag, mg, bound)

    def enc_memory(seed, b=1):
        """`memory` [b, 6, 768] of the reference encoder on synth_normal_image(seed, b, 32, 48): stored in the fixture"""
        with torch.no_grad():
            return enc(torch.from_numpy(W.synth_normal_image(seed, b, 32, 48))).numpy()

    # 1. free runs on the plain weights: S = 6 on the encoder's own output (stored), S = 784 on synth_memory (the recipe is stored)
    load(base)
    mem6 = enc_memory(X_SEED)
    save("free_s6", [run(mem6[0], 48)], 48, dict(S=np.int64(6), variant=np.array("plain"), memory=mem6))
    save("free_s784", [run(W.synth_memory(MEM_SEED, 1, 784)[0], 48)], 48, dict(S=np.int64(784), variant=np.array("plain")))
    # 2. forced run: 40 arbitrary whitelist tokens behind the prefix
    rng = np.random.default_rng(7)
    forced = np.concatenate([[ids.prefix], rng.choice(white[1:], 39)]).astype(np.int32)
    save("forced_s39", [run(W.synth_memory(MEM_SEED, 1, 39)[0], 40, forced)], 40, dict(S=np.int64(39), variant=np.array("plain"), forced=forced[None]))
    # 3. bbox variant: every step chooses a bbox token, the rule fires every fifth step
    st = dict(base)
    st["generator.bias"] = base["generator.bias"].copy()
    st["generator.bias"][ids.bbox_first:ids.bbox_last + 1] += 30.0
    load(st)
    t = run(mem6[0], 24)
    assert all((c == ids.bbox_close) == (i % 5 == 4) for i, c in enumerate(t[0][1:])), t[0]
    save("bbox_s6", [t], 24, dict(S=np.int64(6), variant=np.array("bbox"), bias_add=np.float32(30.0), memory=mem6))
    # 4. EOS variant at B = 3: generator.bias[eos] raised until the three tables stop at three different steps inside [5, 60]; the input
    # seed moves until they do under LOOP_RULES (module docstring), so that the stop steps are the trajectory's and not the rounding's
    ids_no = TU.TableIds(ids.prefix, -1, ids.pad, ids.bbox_close, ids.bbox_first, ids.bbox_last)

    def eos_margin(memory):
        """a free trajectory that never sees EOS (61 steps, plain weights): (the margin EOS lacks at every step, the top-2 gap of the rest)"""
        dec.setup_caches(max_batch_size=1, max_seq_length=1024, dtype=torch.float32, device="cpu")
        lg = []

        def nt(ctx):
            with torch.no_grad():
                t_ = int(dec(torch.from_numpy(memory)[None], torch.tensor([ctx], dtype=torch.int32))[0, 0])
            lg.append(got["logits"][0].numpy())
            return t_
        TU.loop_reference(nt, ids_no, 61)
        L = np.stack(lg)
        return L[:, white[1:]].max(axis=1) - L[:, ids.eos], whitelist_gap(L, white[1:])

    load(base)
    for seed in range(MEM_SEED, MEM_SEED + 60):
        mems = enc_memory(seed, 3)
        margins, gaps = zip(*(eos_margin(mems[b]) for b in range(3)))
        found = None
        cand = np.unique(np.concatenate(margins))
        for m_thr, g_thr in LOOP_RULES:
            for beta in (cand[:-1] + cand[1:]) / 2:
                stops = [int(np.argmax(m < beta)) if (m < beta).any() else -1 for m in margins]
                ok = all(5 <= s_ <= 60 for s_ in stops) and len(set(stops)) == 3
                ok = ok and all(np.abs(m[:s_ + 1] - beta).min() > m_thr for m, s_ in zip(margins, stops))
                ok = ok and all(g_[:s_].min() > g_thr for g_, s_ in zip(gaps, stops))
                if ok:
                    found = (float(beta), stops)
                    break
            if found:
                break
        print("eos search: seed", seed, "margin ranges", [(round(float(m.min()), 2), round(float(m.max()), 2)) for m in margins], "found", found, flush=True)
        if found:
            break
    assert found, "no EOS offset separates the three tables"
    beta, stops = found
    st = dict(base)
    st["generator.bias"] = base["generator.bias"].copy()
    st["generator.bias"][ids.eos] += np.float32(beta)
    load(st)
    tables = [run(mems[b], 64) for b in range(3)]
    assert [len(t[0]) - 2 for t in tables] == stops, ([len(t[0]) for t in tables], stops)
    save("eos_b3_s6", tables, 64, dict(S=np.int64(6), variant=np.array("eos"), bias_add=np.float32(beta), eos_mem_seed=np.int64(seed), memory=mems))
    out_summary["eos"] = {"bias_add": beta, "stops": stops, "mem_seed": seed}
    # host functions: recorded outputs of the reference's own decode_tokens / rescale_bboxes / wrap_with_html_struct on a stand-in vocabulary
    out_summary["host"], ref_fns = mint_host(TU)
    # 5. the whole chain on one 448 x 448 input: reference encoder -> the loop around the reference decoder (EOS variant with an offset of
    # this input's own, same rule) -> the reference's decode_tokens / rescale_bboxes / wrap_with_html_struct.  What
    # Mi355UniTableStructure.forward_tensor must return for synth_normal_image(x_seed, 1, 448, 448) and an original size of 600 x 1000
    load(base)
    found = None
    for x_seed in range(X_SEED, X_SEED + 40):
        with torch.no_grad():
            mem448 = enc(torch.from_numpy(W.synth_normal_image(x_seed, 1, 448, 448))).numpy()[0]
        m, g_ = eos_margin(mem448)
        cand = np.unique(m)
        for m_thr, g_thr in LOOP_RULES:
            for beta in (cand[:-1] + cand[1:]) / 2:
                stop = int(np.argmax(m < beta)) if (m < beta).any() else -1
                if 20 <= stop <= 60 and np.abs(m[:stop + 1] - beta).min() > m_thr and g_[:stop].min() > g_thr:
                    found = (float(beta), stop)
                    break
            if found:
                break
        print("class448 search: x seed", x_seed, "found", found, flush=True)
        if found:
            break
    assert found, "no EOS offset stops the 448 x 448 table inside [20, 60]"
    st = dict(base)
    st["generator.bias"] = base["generator.bias"].copy()
    st["generator.bias"][ids.eos] += np.float32(found[0])
    load(st)
    ctx = run(mem448, 64)[0]
    assert len(ctx) - 2 == found[1] and ctx[-1] == ids.eos
    boxes, html = ref_fns["decode_tokens"](ref_fns["Self"](), torch.tensor([ctx]))
    out_summary["class448"] = {"x_seed": x_seed, "bias_add": found[0], "ids": ctx, "html": html, "wrapped": ref_fns["wrap_with_html_struct"](list(html)),
                               "ori_hw": [600, 1000], "boxes": (ref_fns["rescale_bboxes"](600, 1000, boxes.copy()) if len(boxes) else boxes).tolist()}
    print("class448", {k: out_summary["class448"][k] for k in ("x_seed", "bias_add", "html")}, "tokens", len(ctx))
    return out_summary


def mint_host(TU):
    import ast
    import re
    base = MODULES.parent
    ns = {"re": re, "np": np, "TASK_TOKENS": TU.TASK_TOKENS, "IMG_SIZE": 448, "List": list}
    for path, names in ((base / "main.py", ("decode_tokens",)), (base / "post_process.py", ("rescale_bboxes",)), (base.parent / "utils.py", ("wrap_with_html_struct",))):
        for node in ast.walk(ast.parse(path.read_text())):
            if isinstance(node, ast.FunctionDef) and node.name in names:
                node.returns = None
                for a in node.args.args:
                    a.annotation = None
                exec(compile(ast.Module([node], []), str(path), "exec"), ns)
    toks = TU.stand_in_tokens()

    class Vocab:
        def decode(self, ids_, skip_special_tokens=False):
            return " ".join(toks[int(i)] for i in ids_)

    class Self:
        vocab = Vocab()

    t = {s_: i for i, s_ in enumerate(toks)}
    bb = lambda *v: [t[f"bbox-{x}"] for x in v]
    cases = {
        "two_rows": [11, t["<tr>"], t["<td>["], *bb(1, 2, 30, 40), t["]</td>"], t["<td></td>"], t["</tr>"], t["<tr>"], t["<td"], t[' colspan="2"'], t[">["], *bb(5, 6, 448, 447),
                     t["]</td>"], t["</tr>"], 1],
        "span_no_box": [11, t["<tr>"], t["<td"], t[' rowspan="3"'], t[' colspan="2"'], t["></td>"], t["<td>["], *bb(0, 0, 0), t["]</td>"], t["</tr>"], 1],
        "empty": [11, 1],
        "after_eos": [11, t["<tr>"], t["<td></td>"], t["</tr>"], 1, t["<tr>"], t["<td></td>"], t["</tr>"]],
    }
    rec = {}
    for name, ids_ in cases.items():
        boxes, html = ns["decode_tokens"](Self(), torch.tensor([ids_]))
        r = {"ids": ids_, "boxes": boxes.tolist(), "html": html, "wrapped": ns["wrap_with_html_struct"](list(html))}
        if len(boxes):
            r["rescaled_600x1000"] = ns["rescale_bboxes"](600, 1000, boxes.copy()).tolist()
            r["rescaled_100x50"] = ns["rescale_bboxes"](100, 50, boxes.copy()).tolist()
        rec[name] = r
    ns["Self"] = Self
    return rec, ns


if __name__ == "__main__":
    main()
