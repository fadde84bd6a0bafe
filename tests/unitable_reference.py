"""Shared by the UniTable tests (no test of its own): the fixtures' loader and a restatement of the encoder graph AS THE ENGINE RUNS IT -
the 16 x 16 patches gathered into rows of (c, ky, kx) order and multiplied with conv_proj's weight read as a [768][768] matrix, the position
rows, twelve pre-norm layers (LayerNorm eps 1e-5, packed in_proj, 12 heads of 64 at scale 1/8, out_proj + residual, linear1 + erf GELU,
linear2 + residual) and the final LayerNorm (eps 1e-6) - in any torch dtype, on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F

from rapiddoc_amd import weights as W

KIND = "unitable_encoder"
TAGS = ("b1_h32_w48", "b2_h48_w208", "b1_h64_w272", "b1_h448_w448")
TAPS = ("patch", "layer0", "layer11", "memory")
D, HEADS, HD, LAYERS, PATCH = 768, 12, 64, 12, 16
FIXTURE_TOL = 1e-3          # the project's fixture bound: 1e-3 max(1, max|ref|) per tap

_CACHE = {}


def state(golden_dir):
    if "state" not in _CACHE:
        _CACHE["state"] = W.synth_state_dict(W.load_manifest(golden_dir / f"manifest_{KIND}.json"), 0)
    return _CACHE["state"]


def fixture(golden_dir, tag):
    """(x [B,3,H,W] float32 regenerated from the stored recipe, the npz)"""
    key = ("fixture", tag)
    if key not in _CACHE:
        g = np.load(golden_dir / f"unitable_enc_seed0_{tag}.npz")
        assert str(g["x_kind"]) == "normal_image"
        B, _, H, W_ = (int(v) for v in g["x_shape"])
        _CACHE[key] = (W.synth_normal_image(int(g["x_seed"]), B, H, W_), g)
    return _CACHE[key]


def sub(t, g, name):
    """the fixture's sub-sampling of tap `name` applied to a full [B,T,768] tensor"""
    return t[:, :: int(g[name + "_ts"]), :: int(g[name + "_cs"])]


def patch_rows(x):
    """x [B,3,H,W] -> [B, T, 768], column (c * 16 + ky) * 16 + kx"""
    B, C, H, W_ = x.shape
    t = x.reshape(B, C, H // PATCH, PATCH, W_ // PATCH, PATCH).permute(0, 2, 4, 1, 3, 5)
    return t.reshape(B, (H // PATCH) * (W_ // PATCH), C * PATCH * PATCH)


def attention(qkv, dtype):
    """softmax(q / 8 @ k^T) @ v per (image, head) on packed qkv [B,T,3 * 768] -> [B,T,768]"""
    B, T, _ = qkv.shape
    r = qkv.to(dtype).reshape(B, T, 3, HEADS, HD).permute(2, 0, 3, 1, 4)         # [3][B][heads][T][64]
    p = torch.softmax((r[0] * 0.125) @ r[1].transpose(-1, -2), dim=-1)
    return (p @ r[2]).permute(0, 2, 1, 3).reshape(B, T, HEADS * HD)


def encoder_forward(st, x, dtype=torch.float64):
    """{tap: [B,T,768]} of the graph above; st = name -> float32 ndarray"""
    w = lambda n: torch.from_numpy(np.asarray(st[n])).to(dtype)
    t = patch_rows(torch.from_numpy(x).to(dtype)) @ w("backbone.conv_proj.weight").reshape(D, -1).T + w("backbone.conv_proj.bias")
    out = {"patch": t}
    t = t + w("pos_embed.embedding.weight")[: t.shape[1]]
    for i in range(LAYERS):
        p = f"encoder.layers.{i}."
        y = F.layer_norm(t, (D,), w(p + "norm1.weight"), w(p + "norm1.bias"), 1e-5)
        a = attention(y @ w(p + "self_attn.in_proj_weight").T + w(p + "self_attn.in_proj_bias"), dtype)
        t = t + a @ w(p + "self_attn.out_proj.weight").T + w(p + "self_attn.out_proj.bias")
        y = F.layer_norm(t, (D,), w(p + "norm2.weight"), w(p + "norm2.bias"), 1e-5)
        m = F.gelu(y @ w(p + "linear1.weight").T + w(p + "linear1.bias"))
        t = t + m @ w(p + "linear2.weight").T + w(p + "linear2.bias")
        if i == 0:
            out["layer0"] = t
        if i == LAYERS - 1:
            out["layer11"] = t
    out["memory"] = F.layer_norm(t, (D,), w("norm.weight"), w("norm.bias"), 1e-6)
    return out


# ---------------------------------------------------------------------------------------------------------------- decoder
DEC_KIND = "unitable_decoder"
DEC_TAGS = ("free_s6", "free_s784", "forced_s39", "bbox_s6", "eos_b3_s6")
WHITE = np.array([1] + list(range(12, 510)))


def dec_state(golden_dir, g=None):
    """the plain synthetic decoder weights, or the variant a fixture names (bbox: generator.bias raised on the bbox ids; eos: on eos)"""
    from rapiddoc_amd.table_unitable import STAND_IN_IDS as I
    if "dec_state" not in _CACHE:
        _CACHE["dec_state"] = W.synth_state_dict(W.load_manifest(golden_dir / f"manifest_{DEC_KIND}.json"), 0)
    st = _CACHE["dec_state"]
    variant = str(g["variant"]) if g is not None else "plain"
    if variant == "plain":
        return st
    st = dict(st)
    b = st["generator.bias"].copy()
    if variant == "bbox":
        b[I.bbox_first:I.bbox_last + 1] += np.float32(g["bias_add"])
    else:
        b[I.eos] += np.float32(g["bias_add"])
    st["generator.bias"] = b
    return st


def dec_fixture(golden_dir, tag):
    """(memory [B,S,768] float32, the npz)"""
    key = ("dec", tag)
    if key not in _CACHE:
        g = np.load(golden_dir / f"unitable_dec_seed0_{tag}.npz")
        mem = g["memory"] if "memory" in g.files else W.synth_memory(int(g["mem_seed"]), 1, int(g["S"]))
        _CACHE[key] = (np.ascontiguousarray(mem, dtype=np.float32), g)
    return _CACHE[key]


def fed_tokens(g, b=0):
    """the token the reference fed to every step it ran of table b: its context without the last entry (the forced list of a forced run)"""
    if "forced" in g.files:
        return [int(v) for v in g["forced"][b]]
    ctx = [int(v) for v in g["ids"][b] if v >= 0]
    return ctx[:int((g["chosen"][:, b] >= 0).sum())]


def decoder_forward(st, memory, tokens, dtype=torch.float64):
    """Teacher-forced GPTFastDecoder over one table in one causal pass: memory [S,768], tokens [n] -> (hidden [n,4,768], logits [n,960])"""
    w = lambda n: torch.from_numpy(np.asarray(st[n])).to(dtype)
    lin = lambda x, p: x @ w(p + ".weight").T + w(p + ".bias")
    n = len(tokens)
    mem = torch.from_numpy(memory).to(dtype)
    x = w("token_embed.embedding.weight")[torch.tensor(tokens)] + w("pos_embed.embedding.weight")[:n]
    heads = lambda t: t.reshape(t.shape[0], HEADS, HD).transpose(0, 1)
    mask = torch.tril(torch.ones(n, n, dtype=torch.bool))
    hid = []
    for i in range(4):
        p = f"layers.{i}."
        q, k, v = lin(F.layer_norm(x, (D,), w(p + "norm1.weight"), w(p + "norm1.bias"), 1e-5), p + "self_attn.wqkv").split(D, dim=-1)
        s = (heads(q) * 0.125) @ heads(k).transpose(-1, -2)
        a = torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1) @ heads(v)
        x = x + lin(a.transpose(0, 1).reshape(n, D), p + "self_attn.wo")
        q = lin(F.layer_norm(x, (D,), w(p + "norm2.weight"), w(p + "norm2.bias"), 1e-5), p + "multihead_attn.query")
        k, v = lin(mem, p + "multihead_attn.key"), lin(mem, p + "multihead_attn.value")
        a = torch.softmax((heads(q) * 0.125) @ heads(k).transpose(-1, -2), dim=-1) @ heads(v)
        x = x + lin(a.transpose(0, 1).reshape(n, D), p + "multihead_attn.out")
        x = x + lin(F.gelu(lin(F.layer_norm(x, (D,), w(p + "norm3.weight"), w(p + "norm3.bias"), 1e-5), p + "linear1")), p + "linear2")
        hid.append(x)
    return torch.stack(hid, dim=1), lin(x, "generator")


def whitelist_argmax(logits):
    """[n,960] -> the decoder's next token per row: every id outside the whitelist at -1e9"""
    m = np.full(logits.shape, -1e9)
    m[:, WHITE] = np.asarray(logits)[:, WHITE]
    return m.argmax(axis=1)
