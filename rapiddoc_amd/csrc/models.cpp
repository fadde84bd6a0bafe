// Network topologies of the page hot path, written against the reference's state-dict names so the
// shipped .safetensors load unchanged.  Reference definitions (file:line, relative to /root/reference):
//   PPLCNetV4 ............ rapid_doc/model/ocr/ppocrv6_pytorch/modeling/backbones/rec_lcnetv4.py:7-311
//   RepLKFPN ............. .../necks/db_fpn.py:288-415
//   DBHead (ppocrv6) ..... .../heads/det_db_head.py:52-149
//   LightSVTR ............ .../necks/rnn.py:225-379
//   MultiHead CTC branch . .../heads/rec_multi_head.py:43-75
//   LKPAN ................ .../necks/db_fpn.py:418-525, IntraCLBlock .../necks/intracl.py
//   PFHeadLocal .......... .../heads/det_db_head.py:8-49, 152-180
//   PPLCNetV3 (rec) ...... .../backbones/rec_lcnetv3.py:45-64, 76-351, 493-517
//   PPLCNetV3 (det) ...... .../backbones/rec_lcnetv3.py:24-43, 469-511; RSEFPN .../necks/db_fpn.py:210-285; SEModule
//                          .../backbones/det_mobilenet_v3.py:55-85; DBHead (non-v6 branch) .../heads/det_db_head.py:8-49, 148-149
//   PPHGNetV2-B4 (det) ... rapid_doc/model/formula/rapid_formula_self/networks/backbones/rec_pphgnetv2.py:860-1477
#include "engine.h"

#include <cmath>

namespace rd {

using G = Builder::ConvGeom;

static G geom(int k, int s = 1) {
    G g;
    g.kh = g.kw = k;
    g.sh = g.sw = s;
    g.pt = g.pl = g.pb = g.pr = (k - 1) / 2;
    return g;
}
static G geom_same_even(int k) {  // padding='same' with an even kernel / explicit F.pad(0,1,0,1): pad right+bottom only
    G g;
    g.kh = g.kw = k;
    g.pt = g.pl = (k - 1) / 2;
    g.pb = g.pr = (k - 1) - (k - 1) / 2;
    return g;
}

// ---------------------------------------------------------------------------------------------------
// PPLCNetV4
// ---------------------------------------------------------------------------------------------------
struct LcBlockCfg { int k, cin, cout, sh, sw; bool se; };
bool g_disable_fused_mixer = false;  // RD_DISABLE_FUSED_MIXER=1: A/B switch for parity tests and profiling

static TView lc_stem(Builder& b, const std::string& p, const TView& x_nchw, int c1, int c2) {
    auto cw = [&](const char* n) { return p + "." + n + ".convolution.weight"; };
    auto bn = [&](const char* n) { return p + "." + n + ".normalization"; };
    // stem1 (H/2, c1) -> [max-pool | stem2a (c1/2) -> stem2b (c1)] -> cat (2 c1): one fused kernel in the split-fp16 modes
    (void)c1;
    TView cat = b.stem_front(cw("stem1"), bn("stem1"), cw("stem2a"), bn("stem2a"), cw("stem2b"), bn("stem2b"), x_nchw);
    TView s4 = b.stem_tail(cw("stem3"), bn("stem3"), cw("stem4"), bn("stem4"), cat, ACT_RELU, ACT_RELU);
    b.release(cat);
    (void)c2;
    return s4;
}

static TView lc_block(Builder& b, const std::string& p, const TView& x, const LcBlockCfg& c) {
    const bool rep = c.sh == 1 && c.sw == 1 && c.cin == c.cout;
    G g = geom(c.k);
    g.sh = c.sh;
    g.sw = c.sw;
    TView t;
    Builder::GapOut gap;  // the depthwise kernel also emits the SE pooling partial sums of its output
    Builder::GapOut* gp = c.se ? &gap : nullptr;
    // (round 6) a no-SE 3x3 block whose mixer runs on the resident-weights kernel: the depthwise conv is computed in that kernel's tile load
    // and its output never written (the PREPARE pass still folds the depthwise weights through dwconv)
    const bool fuse_dw = rep && !c.se && c.k == 3 && mixer_fused_supported(c.cin) && !g_disable_fused_mixer && b.mixer_takes_dw(p, c.cin);
    if (fuse_dw) {
        const std::string key = Builder::dw_key(p + ".token_conv.weight", "");
        return b.mixer_fused(p, x, nullptr, &key);
    }
    if (rep) t = b.dwconv(p + ".token_conv.weight", p + ".token_conv.bias", "", x, g, ACT_NONE, nullptr, nullptr, gp);
    else t = b.dwconv(p + ".token_conv.convolution.weight", "", p + ".token_conv.normalization", x, g, ACT_NONE, nullptr, nullptr, gp);
    TView gate;
    bool has_gate = false;
    if (c.se) {
        const std::string s = p + ".token_squeeze_excitation.convolutions.";
        gate = b.se_gate(s + "0.weight", s + "0.bias", s + "2.weight", s + "2.bias", t, ACT_HSIG, &gap);
        has_gate = true;
    }
    if (rep && mixer_fused_supported(c.cin) && !g_disable_fused_mixer) {
        // SE gate, expand, GELU, project and the residual add in one kernel; the gated tensor is never written
        TView o = b.mixer_fused(p, t, has_gate ? &gate : nullptr);
        if (has_gate) b.release(gate);
        b.release(t);
        return o;
    }
    if (has_gate) {
        b.scale(t, gate, 0.f, t);
        b.release(gate);
    }
    TView m = b.conv(p + ".channel_conv1.convolution.weight", "", p + ".channel_conv1.normalization", t, geom(1), ACT_GELU);
    TView o = b.conv(p + ".channel_conv2.convolution.weight", "", p + ".channel_conv2.normalization", m, geom(1), ACT_NONE,
                     nullptr, rep ? &t : nullptr);
    b.release(m);
    b.release(t);
    return o;
}

static const std::vector<std::vector<LcBlockCfg>> kDetSmall = {
    {{3, 48, 48, 1, 1, true}, {3, 48, 48, 1, 1, false}},
    {{3, 48, 96, 2, 2, false}, {3, 96, 96, 1, 1, true}, {3, 96, 96, 1, 1, false}},
    {{3, 96, 192, 2, 2, false}, {3, 192, 192, 1, 1, true}, {3, 192, 192, 1, 1, false}, {3, 192, 192, 1, 1, true},
     {3, 192, 192, 1, 1, false}},
    {{3, 192, 384, 2, 2, false}, {3, 384, 384, 1, 1, true}, {3, 384, 384, 1, 1, false}},
};
static const std::vector<std::vector<LcBlockCfg>> kRecSmall = {
    {{3, 96, 96, 1, 1, true}},
    {{3, 96, 96, 1, 1, false}, {3, 96, 96, 1, 1, false}},
    {{3, 96, 192, 2, 1, false}, {3, 192, 192, 1, 1, true}, {3, 192, 192, 1, 1, false}, {3, 192, 192, 1, 1, true},
     {3, 192, 192, 1, 1, false}, {3, 192, 192, 1, 1, true}, {3, 192, 192, 1, 1, false}},
    {{3, 192, 384, 2, 1, false}, {3, 384, 384, 1, 1, true}, {3, 384, 384, 1, 1, false}},
};

// returns the 4 stage outputs; the caller releases them
static std::vector<TView> lcnetv4(Builder& b, const TView& x_nchw, const std::vector<std::vector<LcBlockCfg>>& cfg,
                                  int c1, int c2, bool keep_all) {
    const std::string enc = "backbone.encoder";
    TView h = lc_stem(b, enc + ".convolution", x_nchw, c1, c2);
    std::vector<TView> feats;
    for (size_t si = 0; si < cfg.size(); ++si) {
        for (size_t bi = 0; bi < cfg[si].size(); ++bi) {
            TView o = lc_block(b, enc + ".blocks." + std::to_string(si) + ".blocks." + std::to_string(bi), h, cfg[si][bi]);
            const bool is_feat = !feats.empty() && feats.back().buf == h.buf;
            if (!is_feat) b.release(h);
            h = o;
        }
        if (keep_all || si + 1 == cfg.size()) feats.push_back(h);
    }
    return feats;
}

// ---------------------------------------------------------------------------------------------------
// PP-OCRv6 det small.   ext[0] = x NCHW [B,3,H,W];  ext[1] = prob map [B,1,H,W]
// ---------------------------------------------------------------------------------------------------
void build_ppocrv6_det(Builder& b, int B, int H, int W, int /*flags*/) {
    RD_CHECK(H % 32 == 0 && W % 32 == 0 && H >= 32 && W >= 32, "det input H, W must be multiples of 32");
    TView x = b.external(0, B, H, W, 3);
    TView out = b.external(1, B, H, W, 1);
    std::vector<TView> f = lcnetv4(b, x, kDetSmall, 24, 48, true);

    // RepLKFPN
    std::vector<TView> fused(4);
    for (int i = 0; i < 4; ++i) {
        const std::string p = "neck.insert_conv." + std::to_string(i);
        TView y = b.conv(p + ".in_conv.weight", "", "", f[i], geom(1), ACT_NONE);
        b.release(f[i]);
        const std::string s = p + ".squeeze_excitation_block.";
        TView gate = b.se_gate(s + "conv1.weight", s + "conv1.bias", s + "conv2.weight", s + "conv2.bias", y, ACT_HSIG_PADDLE);
        b.scale(y, gate, 1.f, y);  // y + y*s
        b.release(gate);
        fused[i] = y;
    }
    for (int i = 2; i >= 0; --i) b.upsample(fused[i + 1], fused[i], 2, true);
    TView cat = b.alloc(B, H / 4, W / 4, 96);
    for (int i = 0; i < 4; ++i) {
        const std::string p = "neck.input_conv." + std::to_string(i);
        TView d = b.dwconv(p + ".depthwise_convolution.weight", p + ".depthwise_convolution.bias", "", fused[i], geom(7), ACT_NONE);
        b.release(fused[i]);
        TView z = b.conv(p + ".pointwise_convolution.weight", "", "", d, geom(1), ACT_NONE);
        b.release(d);
        const std::string s = p + ".squeeze_excitation_module.";
        TView gate = b.se_gate(s + "conv1.weight", s + "conv1.bias", s + "conv2.weight", s + "conv2.bias", z, ACT_HSIG_PADDLE);
        TView slot = b.slice(cat, 24 * (3 - i), 24);  // cat(processed[::-1]) : deepest level first (db_fpn.py:415)
        if (i == 0) {
            b.scale(z, gate, 1.f, slot);
        } else {
            b.scale(z, gate, 1.f, z);
            b.upsample(z, slot, 1 << i, false);
        }
        b.release(gate);
        b.release(z);
    }
    // DBHead v6
    TView c = b.conv("head.conv_down.convolution.weight", "", "head.conv_down.norm", cat, geom(3), ACT_RELU);
    b.release(cat);
    if (b.deconv_pair_to_prob("head.conv_up.convolution.weight", "head.conv_up.convolution.bias", "head.conv_up.norm", "head.conv_final.weight",
                              "head.conv_final.bias", c, out)) {
        b.release(c);
    } else {
        TView u = b.deconv2x2("head.conv_up.convolution.weight", "head.conv_up.convolution.bias", "head.conv_up.norm", c, ACT_RELU);
        b.release(c);
        b.deconv2x2("head.conv_final.weight", "head.conv_final.bias", "", u, ACT_SIGMOID, &out);
        b.release(u);
    }
}

// ---------------------------------------------------------------------------------------------------
// PP-OCRv6 rec small.  ext[0] = x NCHW [B,3,48,W]; ext[1] = idx i32 [B*T]; ext[2] = prob f32 [B*T];
// ext[3] = optional [B,T,C] softmax probabilities or raw logits (flags)
//
// Two-stage form for the page pipeline (the neck + head of one 64-line batch is ~25 launches of 17-30 us on 4352 tokens:
// pure launch latency, ~45 % of a batch's kernel count for ~3 % of its FLOPs):
//   REC_STAGE_BACKBONE   x -> avg-pooled backbone tokens only: ext[1] = [B][T][384] f32 out (the caller points it INTO one
//                        token buffer shared by all batches of the page group)
//   REC_STAGE_TAIL       LightSVTR neck + CTC head ONCE over the tokens of all batches: B = text lines, H = the longest
//                        line in tokens, W = all tokens; ext[0] = tokens [W][384], ext[1] / ext[2] = idx / prob [W],
//                        ext[4] = seg i32 [B][2] (first token, tokens per line), ext[5] = tokinfo i32 [W] (position in the
//                        line | tokens of the line << 16).  Every layer of the neck is row-wise except the 1x7 depthwise
//                        conv and the attention, which take the line structure from those two tables; lines of different
//                        batches (different widths) simply have different lengths.
// ---------------------------------------------------------------------------------------------------
void build_ppocrv6_rec(Builder& b, int B, int H, int W, int flags) {
    const bool tail_only = (flags & REC_STAGE_TAIL) != 0, backbone_only = (flags & REC_STAGE_BACKBONE) != 0;
    RD_CHECK(!(tail_only && backbone_only), "rec: choose one stage");
    RD_CHECK(!(flags & REC_WANT_NECK), "RD_REC_WANT_NECK is offered by the ppocrv5 recognisers only");
    const std::string e = "head.encoder";
    auto cw = [&](int i) { return e + ".conv_block." + std::to_string(i) + ".convolution.weight"; };
    auto cbn = [&](int i) { return e + ".conv_block." + std::to_string(i) + ".normalization"; };
    TView pooled, seg, tokinfo;
    int T, n_seq = B;
    if (tail_only) {
        RD_CHECK((flags & ~REC_STAGE_TAIL) == 0, "rec tail: fused CTC only");
        RD_CHECK(B >= 1 && H >= 1 && H < 32768 && W >= B, "rec tail: B lines, H = longest line (tokens), W = all tokens");
        pooled = b.external(0, 1, 1, W, b.weight_dim(cw(0), 1));
        seg = b.external(4, B, 1, 1, 2);
        tokinfo = b.external(5, 1, 1, W, 1);
        T = H;
    } else {
        RD_CHECK(H == 48, "rec input height must be 48");
        RD_CHECK(W >= 16, "rec input width must be >= 16");
        TView x = b.external(0, B, H, W, 3);
        if (flags & REC_LINE_WIDTHS) {
            RD_CHECK(backbone_only, "rec: per-line widths belong to the backbone stage");
            b.set_line_table(b.external(2, B, 1, 1, kLineTabStride));
        }
        std::vector<TView> f = lcnetv4(b, x, kRecSmall, 48, 96, false);
        if (backbone_only) {
            RD_CHECK((flags & ~(REC_STAGE_BACKBONE | REC_LINE_WIDTHS)) == 0, "rec backbone stage takes no other flag");
            TView out = b.external(1, B, 1, (f[0].w - 2) / 2 + 1, f[0].c);
            b.avgpool3x2(f[0], &out);
            b.release(f[0]);
            return;
        }
        pooled = b.avgpool3x2(f[0]);  // [B,1,W/8,384]
        b.release(f[0]);
        T = pooled.w;
        RD_CHECK(pooled.h == 1, "rec: pooled height");
    }
    const TView* ti = tail_only ? &tokinfo : nullptr;
    const TView* sg = tail_only ? &seg : nullptr;

    TView res = b.conv(cw(0), "", cbn(0), pooled, geom(1), ACT_SILU);
    TView h = b.conv(cw(1), "", cbn(1), pooled, geom(1), ACT_SILU);
    b.release(pooled);
    G g17;
    g17.kh = 1;
    g17.kw = b.weight_dim(cw(2), 3);
    g17.pl = g17.pr = g17.kw / 2;
    TView t = b.dwconv(cw(2), "", cbn(2), h, g17, ACT_SILU, nullptr, &h, nullptr, ti);  // h + silu(bn(dw(h)))
    b.release(h);
    const int C = t.c, heads = 8, hd = C / heads;
    int depth = 0;
    while (b.has_weight(e + ".svtr_block." + std::to_string(depth) + ".layer_norm1.weight")) ++depth;
    for (int d = 0; d < depth; ++d) {
        const std::string p = e + ".svtr_block." + std::to_string(d);
        TView y = b.layernorm(p + ".layer_norm1", t, 1e-6f);
        TView qkv = b.linear(p + ".self_attn.qkv", y, ACT_NONE);
        b.release(y);
        TView a = b.attention(qkv, n_seq, T, heads, hd, sg);
        b.release(qkv);
        TView t2 = b.linear(p + ".self_attn.projection", a, ACT_NONE, nullptr, &t);
        b.release(a);
        b.release(t);
        TView y2 = b.layernorm(p + ".layer_norm2", t2, 1e-6f);
        TView m = b.linear(p + ".mlp.fc1", y2, ACT_SILU);
        b.release(y2);
        t = b.linear(p + ".mlp.fc2", m, ACT_NONE, nullptr, &t2);
        b.release(m);
        b.release(t2);
    }
    TView n = b.layernorm(e + ".norm", t, 1e-6f);
    b.release(t);
    TView seq = b.add(n, res);  // [B,1,T,120]
    b.release(n);
    b.release(res);

    const int ncls = b.weight_dim("head.head.weight", 0);
    TView idx = tail_only ? b.external(1, 1, 1, W, 1) : b.external(1, B, 1, T, 1);
    TView prob = tail_only ? b.external(2, 1, 1, W, 1) : b.external(2, B, 1, T, 1);
    const bool want_full = (flags & (REC_WANT_SOFTMAX | REC_WANT_LOGITS)) != 0;
    if ((flags & REC_UNFUSED_CTC) || want_full) {
        if (flags & REC_WANT_LOGITS) {
            TView lg = b.external(3, B, 1, T, ncls);
            b.linear("head.head", seq, ACT_NONE, &lg);
            b.ctc_stats(lg, idx, prob);
        } else {
            TView lg = b.linear("head.head", seq, ACT_NONE);
            if (flags & REC_WANT_SOFTMAX) {
                // (idx, prob) = numpy's argmax / max of the softmax tensor as written: what the host's CTC decode would compute from it
                TView sm = b.external(3, B, 1, T, ncls);
                b.softmax_rows(lg, sm, &idx, &prob);
            } else {
                b.ctc_stats(lg, idx, prob);
            }
            b.release(lg);
        }
    } else {
        b.ctc_head("head.head", seq, idx, prob);
    }
    b.release(seq);
}

// ---------------------------------------------------------------------------------------------------
// PPHGNetV2-B4 (det=True): the PP-DocLayout-L / plus-L / V2 / V3 backbone.
// ext[0] = x NCHW [B,3,H,W]; ext[1..4] = stage outputs NCHW (strides 4/8/16/32; 128/512/1024/2048 ch)
// ---------------------------------------------------------------------------------------------------
struct HgStageCfg { int cin, mid, cout, blocks; bool down, light; int k, layers; int sh = 2, sw = 2; };   // (sh, sw): strides of the depthwise downsample
static const HgStageCfg kB4Det[4] = {
    {48, 48, 128, 1, false, false, 3, 6},
    {128, 96, 512, 1, true, false, 3, 6},
    {512, 192, 1024, 3, true, true, 5, 6},
    {1024, 384, 2048, 1, true, true, 5, 6},
};

// text_rec=True geometry (ocr .../backbones/rec_pphgnetv2.py:1437-1443): every stage downsamples, one axis at a time; stem3 has stride 1
static const HgStageCfg kB4Rec[4] = {
    {48, 48, 128, 1, true, false, 3, 6, 2, 1},
    {128, 96, 512, 1, true, false, 3, 6, 1, 2},
    {512, 192, 1024, 3, true, true, 5, 6, 2, 1},
    {1024, 384, 2048, 1, true, true, 5, 6, 2, 1},
};

static const HgStageCfg kB6Formula[4] = {   // rec_pphgnetv2.py:1601-1607
    {96, 96, 192, 2, false, false, 3, 6},
    {192, 192, 512, 3, true, false, 3, 6},
    {512, 384, 1024, 6, true, true, 5, 6},
    {1024, 768, 2048, 3, true, true, 5, 6},
};

// Shared PPHGNetV2 body.  `pre` = state-dict prefix ("" or "backbone.pphgnet_b6.").  Every stage output listed in
// `want` is handed to `emit(stage, view)`.
template <typename Emit>
static void build_pphgnetv2(Builder& b, const TView& x, const HgStageCfg (&cfg)[4], const std::string& pre, Emit emit, int stem3_stride = 2) {
    const int B = x.n;
    auto cw = [&](const std::string& p) { return pre + p + ".conv.weight"; };
    auto bn = [&](const std::string& p) { return pre + p + ".bn"; };
    // stem (StemBlock, rec_pphgnetv2.py:979-1056)
    TView cat = b.stem_front(cw("stem.stem1"), bn("stem.stem1"), cw("stem.stem2a"), bn("stem.stem2a"), cw("stem.stem2b"),
                             bn("stem.stem2b"), x);

    // stage inputs are produced straight into channel slot 0 of the stage's dense-concat buffer
    TView cur, cur_cat;
    auto new_cat = [&](int n, int h, int w, const HgStageCfg& c, int cin) { return b.alloc(n, h, w, cin + c.layers * c.mid); };
    {
        const HgStageCfg& c = cfg[0];
        const int s3h = (cat.h + 2 - 3) / stem3_stride + 1, s3w = (cat.w + 2 - 3) / stem3_stride + 1;      // stem3: 3x3 / pad 1
        // (a first stage that downsamples takes the stem's output from a plain buffer; its own concat buffer is made below)
        cur_cat = c.down ? b.alloc(B, s3h, s3w, c.cin) : new_cat(B, s3h, s3w, c, c.cin);
        cur = b.slice(cur_cat, 0, c.cin);
        b.stem_tail(cw("stem.stem3"), bn("stem.stem3"), cw("stem.stem4"), bn("stem.stem4"), cat, ACT_RELU, ACT_RELU, &cur, stem3_stride);
        b.release(cat);
    }
    for (int si = 0; si < 4; ++si) {
        const HgStageCfg& c = cfg[si];
        const std::string sp = "stages." + std::to_string(si);
        RD_CHECK(si == 0 || c.down, "PPHGNetV2: stages 2-4 downsample");
        if (c.down) {  // depthwise 3x3 stride (sh, sw) + BN, no activation (HGV2_Stage.downsample)
            const int oh = (cur.h + 2 - 3) / c.sh + 1, ow = (cur.w + 2 - 3) / c.sw + 1;
            TView ncat = new_cat(B, oh, ow, c, c.cin);
            TView nin = b.slice(ncat, 0, c.cin);
            G gd = geom(3, 2);
            gd.sh = c.sh;
            gd.sw = c.sw;
            b.dwconv(cw(sp + ".downsample"), "", bn(sp + ".downsample"), cur, gd, ACT_NONE, &nin);
            b.release(cur_cat);
            cur_cat = ncat;
            cur = nin;
        }
        for (int bi = 0; bi < c.blocks; ++bi) {
            const std::string bp = sp + ".blocks." + std::to_string(bi);
            const int cin = bi == 0 ? c.cin : c.cout;
            TView prev = cur;
            for (int li = 0; li < c.layers; ++li) {
                const std::string lp = bp + ".layers." + std::to_string(li);
                TView slot = b.slice(cur_cat, cin + li * c.mid, c.mid);
                if (c.light) {
                    TView t = b.conv(cw(lp + ".conv1"), "", bn(lp + ".conv1"), prev, geom(1), ACT_NONE);
                    b.dwconv(cw(lp + ".conv2"), "", bn(lp + ".conv2"), t, geom(c.k), ACT_RELU, &slot);
                    b.release(t);
                } else {
                    b.conv(cw(lp), "", bn(lp), prev, geom(c.k), ACT_RELU, &slot);
                }
                prev = slot;
            }
            TView full = b.slice(cur_cat, 0, cin + c.layers * c.mid);
            TView sq = b.conv(cw(bp + ".aggregation_squeeze_conv"), "", bn(bp + ".aggregation_squeeze_conv"), full, geom(1), ACT_RELU);
            // destination of the block output: slot 0 of the next block's concat buffer, or a plain buffer at a stage end
            const bool last_block = bi + 1 == c.blocks;
            TView ncat, nout;
            if (!last_block) {
                ncat = new_cat(B, cur.h, cur.w, c, c.cout);
                nout = b.slice(ncat, 0, c.cout);
            } else {
                ncat = b.alloc(B, cur.h, cur.w, c.cout);
                nout = ncat;
            }
            const bool identity = bi > 0;
            b.conv(cw(bp + ".aggregation_excitation_conv"), "", bn(bp + ".aggregation_excitation_conv"), sq, geom(1), ACT_RELU,
                   &nout, identity ? &cur : nullptr);
            b.release(sq);
            b.release(cur_cat);
            cur_cat = ncat;
            cur = nout;
        }
        emit(si, cur);
    }
    b.release(cur_cat);
}

// ---------------------------------------------------------------------------------------------------
// PPHGNet_small (rec_hgnet.py:255-290): the backbone of the PP-OCRv4 server detector and recogniser, served under the two v5 server kinds
// when the weights carry it (pphgnet_small_marker).  Stem = three 3x3 ConvBN + ReLU (3 -> 64 stride 2, 64 -> 64, 64 -> 128), det only:
// MaxPool2d(3, 2, 1).  A stage = optional depthwise 3x3 + BN downsample, then HG_Blocks: six 3x3 + BN + ReLU layers (the first from the
// block input, the others from their predecessor), a 1x1 + BN + ReLU aggregation over the concatenation, the ESE gate, and - every block
// but a stage's first - the identity.  The concatenation is never copied: one [B,H,W,in + 6 mid] buffer, block input in slot 0.
// Each 3x3 layer of 128 .. 224 output channels takes the route hg_small_conv_route gives it; the opt-in to conv3x3_wide_h1
// (Builder::set_conv3x3_wide) lives here, nowhere else.
// ---------------------------------------------------------------------------------------------------
struct HgSmallStageCfg { int cin, mid, cout, blocks; bool down; int sh, sw; };
static const HgSmallStageCfg kHgSmallDet[4] = {{128, 128, 256, 1, false, 2, 2}, {256, 160, 512, 1, true, 2, 2}, {512, 192, 768, 2, true, 2, 2}, {768, 224, 1024, 1, true, 2, 2}};
static const HgSmallStageCfg kHgSmallRec[4] = {{128, 128, 256, 1, true, 2, 1}, {256, 160, 512, 1, true, 1, 2}, {512, 192, 768, 2, true, 2, 1}, {768, 224, 1024, 1, true, 2, 1}};
static const int kHgSmallLayers = 6;

// The route of one wide 3x3 layer, by the LAYER (never by the batch or the map), from the per-layer A/B of tools/mb_v4_server.py at the
// detector's and the recogniser's map sizes (profiles/mb_v4_server.txt, docs/notebook/v4_server.md):
//   WIDE     conv3x3_wide_h1: 64 -> 128, 128 -> 128 and 768 -> 192 (1.36 - 1.77 x the generic route, level with the pieces where those exist);
//   PIECES   two launches of conv3x3_h1 over <= 96 output channels (Cin <= 512): the 160- and 192-channel layers, where they measure
//            1.05 - 1.33 x the new kernel (two independent workgroups per CU hide the patch staging that its one workgroup exposes);
//   GENERIC  the split implicit GEMM: the 224-channel layers of stage 4, whose 1/32 maps (30 x 22 per page, 3 x 272 per line) leave
//            much of an 8 x 32 tile empty - the new kernel measures 0.64 x (recogniser) to 0.99 x (detector) of it there.
enum HgSmallConvRoute { HG_CONV_WIDE, HG_CONV_PIECES, HG_CONV_GENERIC };
static HgSmallConvRoute hg_small_conv_route(int cin, int cout) {
    if (cout >= 224) return HG_CONV_GENERIC;
    if (cout > 128 && conv3x3_h1_shape_ok(3, 3, cin, 96)) return HG_CONV_PIECES;
    return HG_CONV_WIDE;
}
static void hg_small_conv3x3(Builder& b, const std::string& w, const std::string& bn, const TView& x, const TView& out) {
    const HgSmallConvRoute route = hg_small_conv_route(x.c, out.c);
    if (route == HG_CONV_PIECES) {
        for (int r0 = 0; r0 < out.c; r0 += 96) {
            const int n = std::min(96, out.c - r0);
            TView piece = b.slice(out, r0, n);
            b.set_conv_rows(r0, n);
            b.conv(w, "", bn, x, geom(3), ACT_RELU, &piece);
        }
        b.set_conv_rows(0, 0);
        return;
    }
    b.set_conv3x3_wide(route == HG_CONV_WIDE);      // the opt-in: only here does a layer ask for the new kernel
    b.conv(w, "", bn, x, geom(3), ACT_RELU, &out);
    b.set_conv3x3_wide(false);
}

template <typename Emit>
static void build_pphgnet_small(Builder& b, const TView& x, bool det, const std::string& pre, Emit emit) {
    const HgSmallStageCfg (&cfg)[4] = det ? kHgSmallDet : kHgSmallRec;
    const int B = x.n;
    auto cw = [&](const std::string& p) { return pre + p + ".conv.weight"; };
    auto bn = [&](const std::string& p) { return pre + p + ".bn"; };
    TView e = b.stem3x3s2(cw("stem.0"), bn("stem.0"), x, ACT_RELU);
    TView s1 = b.conv(cw("stem.1"), "", bn("stem.1"), e, geom(3), ACT_RELU);
    b.release(e);
    TView cur_cat = b.alloc(B, s1.h, s1.w, 128);
    hg_small_conv3x3(b, cw("stem.2"), bn("stem.2"), s1, cur_cat);
    b.release(s1);
    TView cur = cur_cat;
    for (int si = 0; si < 4; ++si) {
        const HgSmallStageCfg& c = cfg[si];
        const std::string sp = "stages." + std::to_string(si);
        RD_CHECK(c.down || (det && si == 0), "PPHGNet_small: only the detector's first stage has no downsample (the stem's max-pool feeds it)");
        {   // the stage input goes straight into slot 0 of the first block's concat buffer
            const int oh = (cur.h + 2 - 3) / c.sh + 1, ow = (cur.w + 2 - 3) / c.sw + 1;
            TView ncat = b.alloc(B, oh, ow, c.cin + kHgSmallLayers * c.mid);
            TView nin = b.slice(ncat, 0, c.cin);
            if (c.down) {
                G gd = geom(3, 2);
                gd.sh = c.sh;
                gd.sw = c.sw;
                b.dwconv(cw(sp + ".downsample"), "", bn(sp + ".downsample"), cur, gd, ACT_NONE, &nin);
            } else {
                b.maxpool3x3s2(cur, &nin);
            }
            b.release(cur_cat);
            cur_cat = ncat;
            cur = nin;
        }
        for (int bi = 0; bi < c.blocks; ++bi) {
            const std::string bp = sp + ".blocks." + std::to_string(bi);
            const int cin = bi == 0 ? c.cin : c.cout;
            TView prev = cur;
            for (int li = 0; li < kHgSmallLayers; ++li) {
                const std::string lp = bp + ".layers." + std::to_string(li);
                TView slot = b.slice(cur_cat, cin + li * c.mid, c.mid);
                hg_small_conv3x3(b, cw(lp), bn(lp), prev, slot);
                prev = slot;
            }
            TView agg = b.conv(cw(bp + ".aggregation_conv"), "", bn(bp + ".aggregation_conv"), cur_cat, geom(1), ACT_RELU);
            const bool identity = bi > 0;
            if (bi + 1 < c.blocks) {     // the gated output is the next block's input: slot 0 of its concat buffer
                TView ncat = b.alloc(B, cur.h, cur.w, c.cout + kHgSmallLayers * c.mid);
                TView nout = b.slice(ncat, 0, c.cout);
                b.ese(pre + bp + ".att.conv", agg, nout, identity ? &cur : nullptr);
                b.release(agg);
                b.release(cur_cat);
                cur_cat = ncat;
                cur = nout;
            } else {
                b.ese(pre + bp + ".att.conv", agg, agg, identity ? &cur : nullptr);
                b.release(cur_cat);
                cur_cat = agg;
                cur = agg;
            }
        }
        emit(si, cur);
    }
    b.release(cur_cat);
}

// ---------------------------------------------------------------------------------------------------
// PP-OCRv5 server det (arch_config.yaml ch_PP-OCRv5_det_server): PPHGNetV2_B4(det=True) -> LKPAN(256, mode large, intracl) -> PFHeadLocal
// (mode large).  ext[0] = x NCHW [B,3,H,W]; ext[1] = maps [B,1,H,W]; DET_WANT_NECK: ext[2] = fuse NCHW [B,256,H/4,W/4].
// head.thresh.* is in the file and unused in eval mode: never asked for.
// Two linear identities: (1) the three branches of an IntraCL level (k x k + k x 1 + 1 x k, biases included) are ONE k x k convolution
// (derive_ppocrv5_det_server_weights); (2) last_3 over cat[shrink, up2(f)] = a 64-channel part over up2(f) + a 1-channel part over shrink,
// both inside the fused tail kernel (Builder::det_local_tail), which also folds the 3 x 3 over the 2x upsample into a 2 x 2 per parity.
// ---------------------------------------------------------------------------------------------------
static const int kIntraK[3] = {7, 5, 3};
static std::string intra_fold_name(const std::string& p, int k) { return p + ".fold_" + std::to_string(k) + "x" + std::to_string(k); }

void derive_ppocrv5_det_server_weights(WeightStore& ws) {
    for (int lvl = 1; lvl <= 4; ++lvl) {
        const std::string p = "neck.incl" + std::to_string(lvl);
        for (int k : kIntraK) {
            const std::string ks = std::to_string(k);
            const HostTensor& wc = ws.get(p + ".c_layer_" + ks + "x" + ks + ".weight");
            const HostTensor& wv = ws.get(p + ".v_layer_" + ks + "x1.weight");
            const HostTensor& wq = ws.get(p + ".q_layer_1x" + ks + ".weight");
            RD_CHECK(wc.shape.size() == 4 && wc.shape[2] == k && wc.shape[3] == k, "IntraCL: c_layer shape");
            const int co = (int)wc.shape[0], ci = (int)wc.shape[1];
            RD_CHECK(wv.numel() == (size_t)co * ci * k && wq.numel() == (size_t)co * ci * k, "IntraCL: v / q layer shape");
            std::vector<float> w(wc.f32(), wc.f32() + wc.numel());
            for (int o = 0; o < co; ++o)
                for (int i = 0; i < ci; ++i)
                    for (int t = 0; t < k; ++t) {
                        const size_t base = ((size_t)o * ci + i) * k * k;
                        w[base + (size_t)t * k + k / 2] += wv.f32()[((size_t)o * ci + i) * k + t];      // k x 1: the middle column
                        w[base + (size_t)(k / 2) * k + t] += wq.f32()[((size_t)o * ci + i) * k + t];    // 1 x k: the middle row
                    }
            std::vector<float> bias(co);
            const float* bc = ws.get(p + ".c_layer_" + ks + "x" + ks + ".bias").f32();
            const float* bv = ws.get(p + ".v_layer_" + ks + "x1.bias").f32();
            const float* bq = ws.get(p + ".q_layer_1x" + ks + ".bias").f32();
            for (int o = 0; o < co; ++o) bias[o] = bc[o] + bv[o] + bq[o];
            ws.add_derived(intra_fold_name(p, k) + ".weight", {co, ci, k, k}, std::move(w));
            ws.add_derived(intra_fold_name(p, k) + ".bias", {co}, std::move(bias));
        }
    }
}

void build_ppocrv5_det_server(Builder& b, int B, int H, int W, int flags) {
    RD_CHECK(H % 32 == 0 && W % 32 == 0 && H >= 64 && W >= 64, "det server input H, W must be multiples of 32 (>= 64)");
    RD_CHECK((flags & ~DET_WANT_NECK) == 0, "det server: unknown flag");
    TView x = b.external(0, B, H, W, 3);
    TView out = b.external(1, B, H, W, 1);
    auto idx = [](const char* p, int i) { return std::string(p) + "." + std::to_string(i) + ".weight"; };

    // backbone; ins_conv[i] (1x1 to 256) runs while stage i's buffer is live
    TView in[4];
    auto ins = [&](int si, const TView& v) { in[si] = b.conv(idx("neck.ins_conv", si), "", "", v, geom(1), ACT_NONE); };
    if (b.has_weight(std::string(pphgnet_small_marker()))) build_pphgnet_small(b, x, true, "backbone.", ins);      // the PP-OCRv4 server file
    else build_pphgnetv2(b, x, kB4Det, "backbone.", ins);
    for (int i = 2; i >= 0; --i) b.upsample(in[i + 1], in[i], 2, true);          // out4, out3, out2 in place
    TView f[4];
    for (int i = 3; i >= 0; --i) {
        f[i] = b.conv(idx("neck.inp_conv", i), "", "", in[i], geom(9), ACT_NONE);
        b.release(in[i]);
    }
    // bottom-up path: pan_{i+1} = f_{i+1} + pan_head_conv[i](pan_i), the add as the convolution's residual
    TView pan[4];
    pan[0] = f[0];
    for (int i = 0; i < 3; ++i) {
        pan[i + 1] = b.conv(idx("neck.pan_head_conv", i), "", "", pan[i], geom(3, 2), ACT_NONE, nullptr, &f[i + 1]);
        b.release(f[i + 1]);
    }
    TView cat = b.alloc(B, H / 4, W / 4, 256);
    for (int i = 0; i < 4; ++i) {
        TView pl = b.conv(idx("neck.pan_lat_conv", i), "", "", pan[i], geom(9), ACT_NONE);
        // IntraCLBlock (reduce_factor 2): 1x1 down, three folded k x k levels, 1x1 back + BN + ReLU, + the block's input
        const std::string p = "neck.incl" + std::to_string(i + 1);
        TView t = b.conv(p + ".conv1x1_reduce_channel.weight", p + ".conv1x1_reduce_channel.bias", "", pl, geom(1), ACT_NONE);
        for (int k : kIntraK) {
            TView u = b.conv(intra_fold_name(p, k) + ".weight", intra_fold_name(p, k) + ".bias", "", t, geom(k), ACT_NONE);
            b.release(t);
            t = u;
        }
        TView slot = b.slice(cat, 64 * (3 - i), 64);                            // cat([p5, p4, p3, p2])
        const std::string rw = p + ".conv1x1_return_channel.weight", rb = p + ".conv1x1_return_channel.bias";
        if (i == 0) {
            b.conv(rw, rb, p + ".bn", t, geom(1), ACT_RELU, &slot, &pl);
        } else {
            TView o = b.conv(rw, rb, p + ".bn", t, geom(1), ACT_RELU, nullptr, &pl);
            b.upsample(o, slot, 1 << i, false);
            b.release(o);
        }
        b.release(t);
        b.release(pl);
    }
    for (int i = 0; i < 4; ++i) b.release(pan[i]);
    if (flags & DET_WANT_NECK) {
        TView o = b.external(2, B, cat.h, cat.w, cat.c);
        b.to_nchw(cat, o);
    }
    // PFHeadLocal: binarize = conv1 + BN + ReLU -> transposed 2x2 + BN + ReLU (= f) -> transposed 2x2 + sigmoid (= shrink); then the local tail
    TView c = b.conv("head.binarize.conv1.weight", "", "head.binarize.conv_bn1", cat, geom(3), ACT_RELU);
    b.release(cat);
    TView ff = b.deconv2x2("head.binarize.conv2.weight", "head.binarize.conv2.bias", "head.binarize.conv_bn2", c, ACT_RELU);
    b.release(c);
    TView shrink = b.deconv2x2("head.binarize.conv3.weight", "head.binarize.conv3.bias", "", ff, ACT_SIGMOID);
    b.det_local_tail("head.cbn_layer.last_3.conv.weight", "head.cbn_layer.last_3.bn", "head.cbn_layer.last_1.weight", "head.cbn_layer.last_1.bias", ff,
                     shrink, out);
    b.release(shrink);
    b.release(ff);
}

void build_pphgnetv2_b4(Builder& b, int B, int H, int W, int /*flags*/) {
    RD_CHECK(H % 32 == 0 && W % 32 == 0 && H >= 64 && W >= 64, "backbone input H, W must be multiples of 32 (>= 64)");
    TView x = b.external(0, B, H, W, 3);
    build_pphgnetv2(b, x, kB4Det, "", [&](int si, const TView& v) {
        TView o = b.external(1 + si, B, v.h, v.w, v.c);
        b.to_nchw(v, o);
    });
}

// ---------------------------------------------------------------------------------------------------
// PP-FormulaNet_plus-M encoder = PPHGNetV2_B6_Formula (rec_pphgnetv2.py:1587-1642): x [B,1|3,H,W] -> [B, H/32*W/32, 2048].
// NHWC [B,h,w,2048] IS the reference's reshape(b,c,h*w).permute(0,2,1), so the result is written without a transpose.
// ext[0] = x NCHW; ext[1] = encoder states [B, h*w, 2048]
// ---------------------------------------------------------------------------------------------------
void build_pphgnetv2_b6_formula(Builder& b, int B, int H, int W, int flags) {
    RD_CHECK(H % 32 == 0 && W % 32 == 0 && H >= 64 && W >= 64, "formula encoder input H, W must be multiples of 32 (>= 64)");
    TView x = b.external(0, B, H, W, (flags & 1) ? 1 : 3);
    build_pphgnetv2(b, x, kB6Formula, "backbone.pphgnet_b6.", [&](int si, const TView& v) {
        if (si != 3) return;
        TView o = b.external(1, B, v.h, v.w, v.c);
        b.copy(v, o);
    });
}

// the PPLCNetV3 backbone of the mobile recogniser and MobileNetV1Enhance of the multilingual ones (below): image -> pooled tokens
static TView lcnetv3_rec(Builder& b, const TView& x, const TView* tokens_out);
static TView mv1e_rec(Builder& b, const TView& x, const TView* tokens_out);
static int rec_tokens_of_width(int W) {      // rd_rec_seq_len
    const int w2 = (W - 1) / 2 + 1, w4 = (w2 - 1) / 2 + 1;
    return w4 / 2;
}

// ---------------------------------------------------------------------------------------------------
// PP-OCRv5 server rec (arch_config.yaml ch_PP-OCRv5_rec_server): PPHGNetV2_B4(text_rec=True) -> EncoderWithSVTR (necks/rnn.py:90-200,
// dims 120, depth 2, kernel [1, 3], use_guide) -> CTCHead Linear(120, classes).  Externals and the two-stage form as build_ppocrv6_rec
// (tokens are [.][2048]); per-line widths inside one backbone launch (REC_LINE_WIDTHS) are not offered for this kind.
// RecSvtrCfg: the same neck and head behind another backbone - PPLCNetV3 (build_ppocrv5_rec_mobile below) or MobileNetV1Enhance
// (build_ppocr_rec_mv1e, whose neck lives under `neck.encoder` and whose classifier is `head.fc`) - both with REC_LINE_WIDTHS served.
// ---------------------------------------------------------------------------------------------------
// the server kind's backbone: image -> pooled tokens [B][1][w4 / 2][2048] (external 1 in the backbone stage)
static TView pphgnetv2_rec_tokens(Builder& b, const TView& x, int B, int Cb, bool backbone_only) {
    TView h;
    // the height collapse avg_pool2d([3, 2]) runs while the last stage's buffer is live
    auto pool = [&](int si, const TView& v) {
        if (si != 3) return;
        RD_CHECK(v.c == Cb, "rec server: backbone width");
        if (backbone_only) {
            TView out = b.external(1, B, 1, (v.w - 2) / 2 + 1, v.c);
            b.avgpool3x2(v, &out);
        } else {
            h = b.avgpool3x2(v);
        }
    };
    if (b.has_weight(std::string(pphgnet_small_marker()))) build_pphgnet_small(b, x, false, "backbone.", pool);   // the PP-OCRv4 server file (1024-wide tokens)
    else build_pphgnetv2(b, x, kB4Rec, "backbone.", pool, 1);
    return h;
}

enum RecBackbone { REC_BB_PPHGNETV2, REC_BB_LCNETV3, REC_BB_MV1E };
struct RecSvtrCfg { const char* neck; const char* fc; RecBackbone backbone; };   // neck / classifier tensor prefixes

// the mobile kinds': the line table (REC_LINE_WIDTHS, backbone stage only) is external 2
static TView lcnetv3_rec_tokens(Builder& b, const TView& x, int B, int W, int Cb, int flags, bool mv1e) {
    const bool backbone_only = (flags & REC_STAGE_BACKBONE) != 0;
    if (flags & REC_LINE_WIDTHS) {
        RD_CHECK(backbone_only, "rec: per-line widths belong to the backbone stage");
        b.set_line_table(b.external(2, B, 1, 1, kLineTabStride));
    }
    if (!backbone_only) return mv1e ? mv1e_rec(b, x, nullptr) : lcnetv3_rec(b, x, nullptr);
    TView out = b.external(1, B, 1, rec_tokens_of_width(W), Cb);
    return mv1e ? mv1e_rec(b, x, &out) : lcnetv3_rec(b, x, &out);
}

static void build_ppocrv5_rec(Builder& b, int B, int H, int W, int flags, const RecSvtrCfg& cfg) {
    const bool mobile = cfg.backbone != REC_BB_PPHGNETV2;
    const bool tail_only = (flags & REC_STAGE_TAIL) != 0, backbone_only = (flags & REC_STAGE_BACKBONE) != 0;
    RD_CHECK(!(tail_only && backbone_only), "rec: choose one stage");
    RD_CHECK(mobile || !(flags & REC_LINE_WIDTHS), "ppocrv5_rec_server: per-line widths inside one backbone launch are out of scope for this kind");
    const std::string e = cfg.neck;
    auto cw = [&](const char* n) { return e + "." + n + ".conv.weight"; };
    auto cbn = [&](const char* n) { return e + "." + n + ".norm"; };
    const int Cb = b.weight_dim(cw("conv1"), 1);
    TView h, seg, tokinfo;
    int T, n_seq = B;
    if (tail_only) {
        RD_CHECK((flags & ~REC_STAGE_TAIL) == 0, "rec tail: fused CTC only");
        RD_CHECK(B >= 1 && H >= 1 && H < 32768 && W >= B, "rec tail: B lines, H = longest line (tokens), W = all tokens");
        h = b.external(0, 1, 1, W, Cb);
        seg = b.external(4, B, 1, 1, 2);
        tokinfo = b.external(5, 1, 1, W, 1);
        T = H;
    } else {
        RD_CHECK(H == 48, "rec input height must be 48");
        RD_CHECK(W >= 16, "rec input width must be >= 16");
        TView x = b.external(0, B, H, W, 3);
        if (backbone_only) RD_CHECK((flags & ~(REC_STAGE_BACKBONE | REC_LINE_WIDTHS)) == 0, "rec backbone stage takes no other flag");
        h = mobile ? lcnetv3_rec_tokens(b, x, B, W, Cb, flags, cfg.backbone == REC_BB_MV1E) : pphgnetv2_rec_tokens(b, x, B, Cb, backbone_only);
        if (backbone_only) return;
        T = h.w;
        RD_CHECK(h.h == 1, "rec: pooled height");
    }
    const TView* ti = tail_only ? &tokinfo : nullptr;
    const TView* sg = tail_only ? &seg : nullptr;

    TView z1 = b.seqconv(cw("conv1"), cbn("conv1"), h, nullptr, ACT_SILU, ti);
    TView t = b.conv(cw("conv2"), "", cbn("conv2"), z1, geom(1), ACT_SILU);
    b.release(z1);
    const int C = t.c, heads = 8, hd = C / heads;
    int depth = 0;
    while (b.has_weight(e + ".svtr_block." + std::to_string(depth) + ".norm1.weight")) ++depth;
    for (int d = 0; d < depth; ++d) {    // Block(prenorm=False) of THIS reference: x + mixer(norm1(x)); x + mlp(norm2(x)) (rec_svtrnet.py:255-262)
        const std::string p = e + ".svtr_block." + std::to_string(d);
        TView y = b.layernorm(p + ".norm1", t, 1e-5f);
        TView qkv = b.linear(p + ".mixer.qkv", y, ACT_NONE);
        b.release(y);
        TView a = b.attention(qkv, n_seq, T, heads, hd, sg);
        b.release(qkv);
        TView t2 = b.linear(p + ".mixer.proj", a, ACT_NONE, nullptr, &t);
        b.release(a);
        b.release(t);
        TView y2 = b.layernorm(p + ".norm2", t2, 1e-5f);
        TView m = b.linear(p + ".mlp.fc1", y2, ACT_SILU);
        b.release(y2);
        t = b.linear(p + ".mlp.fc2", m, ACT_NONE, nullptr, &t2);
        b.release(m);
        b.release(t2);
    }
    TView n = b.layernorm(e + ".norm", t, 1e-6f);
    b.release(t);
    TView z3 = b.conv(cw("conv3"), "", cbn("conv3"), n, geom(1), ACT_SILU);
    b.release(n);
    TView z4 = b.seqconv(cw("conv4"), cbn("conv4"), h, &z3, ACT_SILU, ti);   // cat(h, z3) is never written: two K segments
    b.release(z3);
    b.release(h);
    TView seq = b.conv(cw("conv1x1"), "", cbn("conv1x1"), z4, geom(1), ACT_SILU);
    b.release(z4);

    if (flags & REC_WANT_NECK) {         // the classifier's input, for the parity tests of the neck
        RD_CHECK(flags == REC_WANT_NECK, "rec: RD_REC_WANT_NECK goes with no other flag");
        TView o = b.external(3, B, 1, T, seq.c);
        b.copy(seq, o);
    }
    const std::string fc = cfg.fc;
    const int ncls = b.weight_dim(fc + ".weight", 0);
    TView idx = tail_only ? b.external(1, 1, 1, W, 1) : b.external(1, B, 1, T, 1);
    TView prob = tail_only ? b.external(2, 1, 1, W, 1) : b.external(2, B, 1, T, 1);
    const bool want_full = (flags & (REC_WANT_SOFTMAX | REC_WANT_LOGITS)) != 0;
    if ((flags & REC_UNFUSED_CTC) || want_full) {
        if (flags & REC_WANT_LOGITS) {
            TView lg = b.external(3, B, 1, T, ncls);
            b.linear(fc, seq, ACT_NONE, &lg);
            b.ctc_stats(lg, idx, prob);
        } else {
            TView lg = b.linear(fc, seq, ACT_NONE);
            if (flags & REC_WANT_SOFTMAX) {
                TView sm = b.external(3, B, 1, T, ncls);
                b.softmax_rows(lg, sm, &idx, &prob);
            } else {
                b.ctc_stats(lg, idx, prob);
            }
            b.release(lg);
        }
    } else {
        b.ctc_head(fc, seq, idx, prob);
    }
    b.release(seq);
}

static const RecSvtrCfg kRecV5Server = {"head.ctc_encoder.encoder", "head.ctc_head.fc", REC_BB_PPHGNETV2};
static const RecSvtrCfg kRecV5Mobile = {"head.ctc_encoder.encoder", "head.ctc_head.fc", REC_BB_LCNETV3};
static const RecSvtrCfg kRecMv1e = {"neck.encoder", "head.fc", REC_BB_MV1E};
void build_ppocrv5_rec_server(Builder& b, int B, int H, int W, int flags) { build_ppocrv5_rec(b, B, H, W, flags, kRecV5Server); }

// ---------------------------------------------------------------------------------------------------
// PP-OCRv5 mobile rec (arch_config.yaml ch_PP-OCRv5_rec_mobile): PPLCNetV3(scale 0.95, rec geometry) -> the server kind's neck and
// head (dims 120; the neck's two sequence convolutions are 60 wide here).  Externals, flags and stages as build_ppocrv6_rec, per-line
// widths (REC_LINE_WIDTHS) included; tokens are [.][480].
// A block is dw_conv -> (SE) -> pw_conv, each a LearnableRepLayer = lab(sum of branches) -> hardswish -> act.lab.  At load time every
// layer becomes one convolution + bias (derive_ppocrv5_rec_mobile_weights).  `act.lab` stays a scalar affine after the activation: the
// depthwise kernel applies hardswish and its own affine in its epilogue; a pointwise layer writes convolution + bias, and its hardswish
// and affine are applied by its consumer - the next depthwise kernel on load (inside the map only: the padding stays zero, as in the
// reference) or the final pooling kernel - so the matrix kernels' shared epilogue does not change (kernels_lcv3.hip says why).
// Every layer here is activated: the rec geometry's strides are 1 or tuples and the reference skips the activation for `stride == 2` only.
// ---------------------------------------------------------------------------------------------------
struct Lcv3Cfg { const char* name; int k, cin, cout, sh, sw; bool se; };
static const Lcv3Cfg kLcv3Rec[] = {
    {"blocks2.0", 3, 16, 32, 1, 1, false},
    {"blocks3.0", 3, 32, 64, 1, 1, false},   {"blocks3.1", 3, 64, 64, 1, 1, false},
    {"blocks4.0", 3, 64, 128, 2, 1, false},  {"blocks4.1", 3, 128, 128, 1, 1, false},
    {"blocks5.0", 3, 128, 240, 1, 2, false}, {"blocks5.1", 5, 240, 240, 1, 1, false}, {"blocks5.2", 5, 240, 240, 1, 1, false},
    {"blocks5.3", 5, 240, 240, 1, 1, false}, {"blocks5.4", 5, 240, 240, 1, 1, false},
    {"blocks6.0", 5, 240, 480, 2, 1, true},  {"blocks6.1", 5, 480, 480, 1, 1, true},  {"blocks6.2", 5, 480, 480, 2, 1, false},
    {"blocks6.3", 5, 480, 480, 1, 1, false},
};

// lab(sum_i BN_i(conv_i) + BN_1x1(conv_1x1) + BN_id(x)) as ONE k x k convolution + bias: the BN-folded branch sum in double, the 1 x 1
// and the identity on the centre tap, `lab` multiplied in, rounded once
static void fold_rep_layer(WeightStore& ws, const std::string& p, bool depthwise) {
    const HostTensor& w0 = ws.get(p + ".conv_kxk.0.conv.weight");
    const int co = (int)w0.shape[0], ci = (int)w0.shape[1], k = (int)w0.shape[2];
    RD_CHECK(w0.shape.size() == 4 && w0.shape[3] == k && (depthwise ? ci == 1 : k == 1), "LearnableRepLayer: branch shape: " + p);
    const size_t per = (size_t)ci * k * k;
    std::vector<double> w((size_t)co * per, 0.0), bias(co, 0.0);
    auto bn = [&](const std::string& q, int o, double& scale, double& shift) {
        const double g = ws.get(q + ".weight").f32()[o], be = ws.get(q + ".bias").f32()[o], m = ws.get(q + ".running_mean").f32()[o],
                     v = ws.get(q + ".running_var").f32()[o];
        scale = g / std::sqrt(v + 1e-5);
        shift = be - m * scale;
    };
    for (int i = 0; ws.has(p + ".conv_kxk." + std::to_string(i) + ".conv.weight"); ++i) {
        const std::string q = p + ".conv_kxk." + std::to_string(i);
        const HostTensor& wi = ws.get(q + ".conv.weight");
        RD_CHECK(wi.numel() == (size_t)co * per, "LearnableRepLayer: branch shape: " + q);
        for (int o = 0; o < co; ++o) {
            double sc, sh;
            bn(q + ".bn", o, sc, sh);
            for (size_t t = 0; t < per; ++t) w[o * per + t] += sc * wi.f32()[o * per + t];
            bias[o] += sh;
        }
    }
    const size_t centre = (size_t)(k / 2) * k + k / 2;
    if (ws.has(p + ".conv_1x1.conv.weight")) {
        const HostTensor& w1 = ws.get(p + ".conv_1x1.conv.weight");
        RD_CHECK(w1.numel() == (size_t)co * ci, "LearnableRepLayer: 1x1 branch shape: " + p);
        for (int o = 0; o < co; ++o) {
            double sc, sh;
            bn(p + ".conv_1x1.bn", o, sc, sh);
            for (int c = 0; c < ci; ++c) w[o * per + (size_t)c * k * k + centre] += sc * w1.f32()[(size_t)o * ci + c];
            bias[o] += sh;
        }
    }
    if (ws.has(p + ".identity.weight")) {
        for (int o = 0; o < co; ++o) {
            double sc, sh;
            bn(p + ".identity", o, sc, sh);
            w[o * per + (size_t)(depthwise ? 0 : o) * k * k + centre] += sc;
            bias[o] += sh;
        }
    }
    const double ls = ws.get(p + ".lab.scale").f32()[0], lb = ws.get(p + ".lab.bias").f32()[0];
    std::vector<float> wf(w.size()), bf(co);
    for (size_t i = 0; i < w.size(); ++i) wf[i] = (float)(w[i] * ls);
    for (int o = 0; o < co; ++o) bf[o] = (float)(bias[o] * ls + lb);
    ws.add_derived(p + ".fold.weight", {co, ci, k, k}, std::move(wf));
    ws.add_derived(p + ".fold.bias", {co}, std::move(bf));
}

// both layers of every block of a PPLCNetV3 configuration; the fold goes by the tensors the file has (an identity BatchNorm exists only
// where cin == cout and the stride is 1)
template <size_t N>
static void fold_lcv3_blocks(WeightStore& ws, const Lcv3Cfg (&cfg)[N]) {
    for (const Lcv3Cfg& c : cfg) {
        const std::string p = std::string("backbone.") + c.name;
        fold_rep_layer(ws, p + ".dw_conv", true);
        fold_rep_layer(ws, p + ".pw_conv", false);
    }
}

void derive_ppocrv5_rec_mobile_weights(WeightStore& ws) { fold_lcv3_blocks(ws, kLcv3Rec); }

// x NCHW image -> pooled tokens [B][1][w4 / 2][480] (into *tokens_out when given)
static TView lcnetv3_rec(Builder& b, const TView& x, const TView* tokens_out) {
    TView h = b.stem3x3s2("backbone.conv1.conv.weight", "backbone.conv1.bn", x, ACT_NONE);   // columns >= a line's w2 are ignored by every reader
    Builder::Affine pre;
    bool has_pre = false;     // conv1 has neither activation nor affine
    int lt_col = 1;           // LineTab column of the current map's valid width: w2 up to blocks5.0's input, w4 after it
    for (const Lcv3Cfg& c : kLcv3Rec) {
        const std::string p = std::string("backbone.") + c.name;
        RD_CHECK(h.c == c.cin, "PPLCNetV3: channel chain: " + p);
        const int lt_out = c.sw == 2 ? 2 : lt_col;
        TView fused;
        if (c.k == 3 && c.sh == 1 && c.sw == 1 && !c.se &&
            b.lcv3_block(p + ".dw_conv.fold.weight", p + ".pw_conv.fold.weight", p + ".pw_conv.fold.bias", h, has_pre ? &pre : nullptr,
                         b.affine(p + ".dw_conv.act.lab"), lt_col, &fused)) {     // RD_LCV3_FUSED=1: the block in one launch
            b.release(h);
            h = fused;
            pre = b.affine(p + ".pw_conv.act.lab");
            has_pre = true;
            continue;
        }
        // (strip 1: a 5x5 layer may take the LDS-staged strip kernel of kernels_mv1e.hip under RD_LCV3_DW_STRIP=1 - opt-in, measured in
        // docs/notebook/rec_mv1e.md; the default route and its bits are the direct kernel's)
        TView t = b.lcv3_dw(p + ".dw_conv.fold.weight", p + ".dw_conv.fold.bias", h, c.k, c.sh, c.sw, has_pre ? &pre : nullptr,
                            b.affine(p + ".dw_conv.act.lab"), lt_col, lt_out, c.k == 5 ? 1 : 0);
        b.release(h);
        lt_col = lt_out;
        if (c.se) {
            Builder::GapOut gap = b.lcv3_gap(t, lt_col);
            TView gate = b.se_gate(p + ".se.conv1.weight", p + ".se.conv1.bias", p + ".se.conv2.weight", p + ".se.conv2.bias", t, ACT_HSIG, &gap);
            b.scale(t, gate, 0.f, t);
            b.release(gate);
        }
        h = b.conv(p + ".pw_conv.fold.weight", p + ".pw_conv.fold.bias", "", t, geom(1), ACT_NONE);    // hardswish + act.lab: the consumer's
        b.release(t);
        pre = b.affine(p + ".pw_conv.act.lab");
        has_pre = true;
        RD_CHECK(h.c == c.cout, "PPLCNetV3: channel chain: " + p);
    }
    TView tok = b.lcv3_pool(h, pre, tokens_out);
    b.release(h);
    return tok;
}

void build_ppocrv5_rec_mobile(Builder& b, int B, int H, int W, int flags) { build_ppocrv5_rec(b, B, H, W, flags, kRecV5Mobile); }

// ---------------------------------------------------------------------------------------------------
// Multilingual PP-OCRv3 / v4 mobile rec (arch_config.yaml latin_ / cyrillic_ / chinese_cht_PP-OCRv3_rec_mobile, arabic_ / korean_ / japan_ /
// ta_ / te_ / ka_ / devanagari_PP-OCRv4_rec_mobile - one graph, ten class counts): MobileNetV1Enhance(scale 0.5, last_conv_stride
// [1, 2], avg pool; backbones/rec_mv1_enhance.py) -> SequenceEncoder(svtr, dims 64, depth 2, hidden_dims 120, use_guide; necks/rnn.py:90-200,
// 382-422) -> CTCHead Linear(64, classes) (heads/rec_ctc_head.py).  Externals, flags and stages as build_ppocrv6_rec, per-line widths
// (REC_LINE_WIDTHS) included; tokens are [.][512].
// Every backbone layer is Conv -> BatchNorm -> hardswish, without branches.  At load time every layer of the blocks becomes weight + bias
// (derive_ppocr_rec_mv1e_weights: in double, rounded once).  The activation is placed as in PPLCNetV3 with identity affines: a depthwise
// layer applies its own hardswish in its epilogue; conv1 and every pointwise layer write convolution + bias, and their hardswish is applied
// by the consumer on load - the next depthwise kernel (inside the map and inside the line's width only: the padding stays zero) or the
// final pooling kernel - so the matrix kernels' shared epilogue does not change (kernels_lcv3.hip says why).
// Rows go 48 -> 24 (conv1) -> 12 -> 6 -> 3; the width is w2 up to the last block, whose stride (1, 2) makes it w4.  AvgPool2d(2, 2) on the
// 3-row map uses rows 0 and 1 only.  SE: relu between the two FCs, gate relu6(x + 3) / 6 (ACT_HSIG), the mean over all rows inside the
// line's width.
// ---------------------------------------------------------------------------------------------------
struct Mv1eCfg { int k, cin, cout, sh, sw; bool se; };
static const Mv1eCfg kMv1eRec[13] = {
    {3, 16, 32, 1, 1, false},   {3, 32, 64, 1, 1, false},   {3, 64, 64, 1, 1, false},   {3, 64, 128, 2, 1, false},  {3, 128, 128, 1, 1, false},
    {3, 128, 256, 2, 1, false}, {5, 256, 256, 1, 1, false}, {5, 256, 256, 1, 1, false}, {5, 256, 256, 1, 1, false}, {5, 256, 256, 1, 1, false},
    {5, 256, 256, 1, 1, false}, {5, 256, 512, 2, 1, true},  {5, 512, 512, 1, 2, true},
};

// Conv (no bias) `p`<conv>.weight + BatchNorm (eps 1e-5) `p`<bn>.* as p.fold.weight / p.fold.bias: scale and product in double, rounded once
static void fold_conv_bn(WeightStore& ws, const std::string& p, const char* conv = "._conv", const char* bn = "._batch_norm") {
    const HostTensor& w = ws.get(p + conv + ".weight");
    RD_CHECK(w.shape.size() == 4, "Conv + BatchNorm fold: convolution weight shape: " + p);
    const int co = (int)w.shape[0];
    const size_t per = w.numel() / co;
    const std::string q = p + bn;
    RD_CHECK(ws.get(q + ".weight").numel() == (size_t)co, "Conv + BatchNorm fold: channel count: " + p);
    std::vector<float> wf(w.numel()), bf(co);
    for (int o = 0; o < co; ++o) {
        const double g = ws.get(q + ".weight").f32()[o], be = ws.get(q + ".bias").f32()[o], m = ws.get(q + ".running_mean").f32()[o],
                     v = ws.get(q + ".running_var").f32()[o];
        const double sc = g / std::sqrt(v + 1e-5);
        for (size_t t = 0; t < per; ++t) wf[o * per + t] = (float)(sc * w.f32()[o * per + t]);
        bf[o] = (float)(be - m * sc);
    }
    ws.add_derived(p + ".fold.weight", std::vector<int64_t>(w.shape.begin(), w.shape.end()), std::move(wf));
    ws.add_derived(p + ".fold.bias", {co}, std::move(bf));
}

void derive_ppocr_rec_mv1e_weights(WeightStore& ws) {
    for (int i = 0; i < 13; ++i) {      // (conv1 is folded by Builder::stem3x3s2, as every stem here)
        const std::string p = "backbone.block_list." + std::to_string(i);
        fold_conv_bn(ws, p + "._depthwise_conv");
        fold_conv_bn(ws, p + "._pointwise_conv");
    }
}

// x NCHW image -> pooled tokens [B][1][w4 / 2][512] (into *tokens_out when given)
static TView mv1e_rec(Builder& b, const TView& x, const TView* tokens_out) {
    // conv1 writes convolution + BatchNorm; its hardswish is the first depthwise layer's.  Columns >= a line's w2 are ignored by every reader
    TView h = b.stem3x3s2("backbone.conv1._conv.weight", "backbone.conv1._batch_norm", x, ACT_NONE);
    const Builder::Affine one;    // hardswish without an affine
    int lt_col = 1;               // LineTab column of the current map's valid width: w2 up to the last block's input, w4 after it
    for (int i = 0; i < 13; ++i) {
        const Mv1eCfg& c = kMv1eRec[i];
        const std::string p = "backbone.block_list." + std::to_string(i);
        RD_CHECK(h.c == c.cin, "MobileNetV1Enhance: channel chain: " + p);
        const int lt_out = c.sw == 2 ? 2 : lt_col;
        TView t = b.lcv3_dw(p + "._depthwise_conv.fold.weight", p + "._depthwise_conv.fold.bias", h, c.k, c.sh, c.sw, &one, one, lt_col, lt_out,
                            c.k == 5 ? 2 : 0);
        b.release(h);
        lt_col = lt_out;
        if (c.se) {
            Builder::GapOut gap = b.lcv3_gap(t, lt_col);
            TView gate = b.se_gate(p + "._se.conv1.weight", p + "._se.conv1.bias", p + "._se.conv2.weight", p + "._se.conv2.bias", t, ACT_HSIG, &gap, lt_col);
            b.scale(t, gate, 0.f, t);
            b.release(gate);
        }
        h = b.conv(p + "._pointwise_conv.fold.weight", p + "._pointwise_conv.fold.bias", "", t, geom(1), ACT_NONE);    // hardswish: the consumer's
        b.release(t);
        RD_CHECK(h.c == c.cout, "MobileNetV1Enhance: channel chain: " + p);
    }
    TView tok = b.mv1e_pool(h, tokens_out);
    b.release(h);
    return tok;
}

void build_ppocr_rec_mv1e(Builder& b, int B, int H, int W, int flags) { build_ppocrv5_rec(b, B, H, W, flags, kRecMv1e); }

// ---------------------------------------------------------------------------------------------------
// PP-OCRv5 mobile det (arch_config.yaml ch_PP-OCRv5_det_mobile): PPLCNetV3(scale 0.75, det=True) -> RSEFPN(96, shortcut) -> DBHead(k 50).
// ext[0] = x NCHW [B,3,H,W]; ext[1] = maps [B,1,H,W]; DET_WANT_NECK: ext[2] = fuse NCHW [B,96,H/4,W/4].
// The backbone is the mobile recogniser's with integer strides.  The reference activates a LearnableRepLayer `if self.stride != 2`, and
// here the stride IS the integer 2: a stride-2 depthwise layer is lab(branches) and nothing else - `lab` is in the folded weights, and
// the `act.lab` tensors the file carries for those layers are never asked for.  Everything else follows the recogniser: a pointwise layer
// writes convolution + bias, its hardswish + act.lab run in its consumer.  The four stage outputs feed matrix kernels, which cannot
// activate on load: their activated form is written once by lcv3_act.
// layer_list[i] (1x1, bias) -> ins_conv[i].in_conv (1x1, no bias) has nothing nonlinear in between: ONE 1x1 convolution + bias, derived
// in double at load time; the widths 12 / 18 / 42 / 360 never exist.  head.thresh.* is in the file and unused in eval mode.
// ---------------------------------------------------------------------------------------------------
// The part of RSEFPN + DBHead that the PP-OCRv5 mobile detector and the PP-OCRv3 multilingual detector share.
// y <- y + y * gate(y): an RSELayer's squeeze-excite with the paddle hard-sigmoid slope and the shortcut, in place
static void rse_gate_shortcut(Builder& b, const std::string& p, const TView& y) {
    const std::string s = p + ".se_block.";
    TView gate = b.se_gate(s + "conv1.weight", s + "conv1.bias", s + "conv2.weight", s + "conv2.bias", y, ACT_HSIG_PADDLE);
    b.scale(y, gate, 1.f, y);  // y + y*s (shortcut)
    b.release(gate);
}
// in[0..3]: the gated ins_conv outputs [B,96,H/4 .. H/32,.] (released here) -> top-down adds, inp_conv 3x3 + gate, concat (`fuse`; under
// DET_WANT_NECK also ext[2]), DBHead -> out.  ACT_SIGMOID maps NaN to 0 (the v5 head's fix_nan); on finite input that is the identity, so a
// head without fix_nan (PP-OCRv3) runs the same tail
static void rsefpn_db_tail(Builder& b, TView (&in)[4], int B, int H, int W, int flags, const TView& out) {
    // RSEFPN
    for (int i = 2; i >= 0; --i) b.upsample(in[i + 1], in[i], 2, true);          // out4, out3, out2 in place
    TView cat = b.alloc(B, H / 4, W / 4, 96);
    for (int i = 0; i < 4; ++i) {
        const std::string p = "neck.inp_conv." + std::to_string(i);
        TView z = b.conv(p + ".in_conv.weight", "", "", in[i], geom(3), ACT_NONE);
        b.release(in[i]);
        const std::string s = p + ".se_block.";
        TView gate = b.se_gate(s + "conv1.weight", s + "conv1.bias", s + "conv2.weight", s + "conv2.bias", z, ACT_HSIG_PADDLE);
        TView slot = b.slice(cat, 24 * (3 - i), 24);                             // cat([p5, p4, p3, p2])
        if (i == 0) {
            b.scale(z, gate, 1.f, slot);
        } else {
            b.scale(z, gate, 1.f, z);
            b.upsample(z, slot, 1 << i, false);
        }
        b.release(gate);
        b.release(z);
    }
    if (flags & DET_WANT_NECK) {
        TView o = b.external(2, B, cat.h, cat.w, cat.c);
        b.to_nchw(cat, o);
    }
    // DBHead: binarize = 3x3 + BN + ReLU -> transposed 2x2 + BN + ReLU -> transposed 2x2 to one channel -> sigmoid
    TView c = b.conv("head.binarize.conv1.weight", "", "head.binarize.conv_bn1", cat, geom(3), ACT_RELU);
    b.release(cat);
    if (b.deconv_pair_to_prob("head.binarize.conv2.weight", "head.binarize.conv2.bias", "head.binarize.conv_bn2", "head.binarize.conv3.weight",
                              "head.binarize.conv3.bias", c, out)) {
        b.release(c);
    } else {
        TView u = b.deconv2x2("head.binarize.conv2.weight", "head.binarize.conv2.bias", "head.binarize.conv_bn2", c, ACT_RELU);
        b.release(c);
        b.deconv2x2("head.binarize.conv3.weight", "head.binarize.conv3.bias", "", u, ACT_SIGMOID, &out);
        b.release(u);
    }
}

static const Lcv3Cfg kLcv3Det[] = {
    {"blocks2.0", 3, 16, 32, 1, 1, false},
    {"blocks3.0", 3, 32, 48, 2, 2, false},   {"blocks3.1", 3, 48, 48, 1, 1, false},
    {"blocks4.0", 3, 48, 96, 2, 2, false},   {"blocks4.1", 3, 96, 96, 1, 1, false},
    {"blocks5.0", 3, 96, 192, 2, 2, false},  {"blocks5.1", 5, 192, 192, 1, 1, false}, {"blocks5.2", 5, 192, 192, 1, 1, false},
    {"blocks5.3", 5, 192, 192, 1, 1, false}, {"blocks5.4", 5, 192, 192, 1, 1, false},
    {"blocks6.0", 5, 192, 384, 2, 2, true},  {"blocks6.1", 5, 384, 384, 1, 1, true},  {"blocks6.2", 5, 384, 384, 1, 1, false},
    {"blocks6.3", 5, 384, 384, 1, 1, false},
};
static const char* const kLcv3DetTaps[4] = {"blocks3.1", "blocks4.1", "blocks5.4", "blocks6.3"};
static std::string ins_fold_name(int i) { return "neck.ins_conv." + std::to_string(i) + ".fold"; }

void derive_ppocrv5_det_mobile_weights(WeightStore& ws) {
    fold_lcv3_blocks(ws, kLcv3Det);
    for (int i = 0; i < 4; ++i) {
        const HostTensor& wl = ws.get("backbone.layer_list." + std::to_string(i) + ".weight");     // [m][k][1][1]
        const HostTensor& bl = ws.get("backbone.layer_list." + std::to_string(i) + ".bias");
        const HostTensor& wi = ws.get("neck.ins_conv." + std::to_string(i) + ".in_conv.weight");    // [co][m][1][1]
        const int m = (int)wl.shape[0], k = (int)wl.shape[1], co = (int)wi.shape[0];
        RD_CHECK(wl.numel() == (size_t)m * k && wi.numel() == (size_t)co * m && (int)wi.shape[1] == m && bl.numel() == (size_t)m,
                 "layer_list / ins_conv shapes of level " + std::to_string(i));
        std::vector<float> w((size_t)co * k), bias(co);
        for (int o = 0; o < co; ++o) {
            for (int c = 0; c < k; ++c) {
                double a = 0.0;
                for (int j = 0; j < m; ++j) a += (double)wi.f32()[(size_t)o * m + j] * wl.f32()[(size_t)j * k + c];
                w[(size_t)o * k + c] = (float)a;
            }
            double a = 0.0;
            for (int j = 0; j < m; ++j) a += (double)wi.f32()[(size_t)o * m + j] * bl.f32()[j];
            bias[o] = (float)a;
        }
        ws.add_derived(ins_fold_name(i) + ".weight", {co, k, 1, 1}, std::move(w));
        ws.add_derived(ins_fold_name(i) + ".bias", {co}, std::move(bias));
    }
}

void build_ppocrv5_det_mobile(Builder& b, int B, int H, int W, int flags) {
    RD_CHECK(H % 32 == 0 && W % 32 == 0 && H >= 32 && W >= 32, "det mobile input H, W must be multiples of 32");
    RD_CHECK((flags & ~DET_WANT_NECK) == 0, "det mobile: unknown flag");
    TView x = b.external(0, B, H, W, 3);
    TView out = b.external(1, B, H, W, 1);

    // backbone; the folded layer_list + ins_conv 1x1 and its RSE gate run while the stage's buffers are live
    TView h = b.stem3x3s2("backbone.conv1.conv.weight", "backbone.conv1.bn", x, ACT_NONE);
    Builder::Affine pre;
    bool has_pre = false;     // conv1 has neither activation nor affine
    int level = 1, tap = 0;   // level: log2 of the current map's reduction of the page
    TView in[4];
    for (const Lcv3Cfg& c : kLcv3Det) {
        const std::string p = std::string("backbone.") + c.name;
        RD_CHECK(h.c == c.cin, "PPLCNetV3: channel chain: " + p);
        Builder::Affine post;
        if (c.sh != 2) post = b.affine(p + ".dw_conv.act.lab");             // a stride-2 layer's act.lab is never asked for: a file without it loads
        TView t = b.lcv3_dw_det(p + ".dw_conv.fold.weight", p + ".dw_conv.fold.bias", h, c.k, c.sh, has_pre ? &pre : nullptr, c.sh == 2 ? nullptr : &post,
                                level);
        b.release(h);
        if (c.sh == 2) ++level;
        if (c.se) {
            Builder::GapOut gap = b.lcv3_gap(t, 0);
            TView gate = b.se_gate(p + ".se.conv1.weight", p + ".se.conv1.bias", p + ".se.conv2.weight", p + ".se.conv2.bias", t, ACT_HSIG, &gap);
            b.scale(t, gate, 0.f, t);
            b.release(gate);
        }
        h = b.conv(p + ".pw_conv.fold.weight", p + ".pw_conv.fold.bias", "", t, geom(1), ACT_NONE);    // hardswish + act.lab: the consumer's
        b.release(t);
        pre = b.affine(p + ".pw_conv.act.lab");
        has_pre = true;
        RD_CHECK(h.c == c.cout, "PPLCNetV3: channel chain: " + p);
        if (tap < 4 && std::string(c.name) == kLcv3DetTaps[tap]) {
            TView a = b.lcv3_act(h, pre);
            TView y = b.conv(ins_fold_name(tap) + ".weight", ins_fold_name(tap) + ".bias", "", a, geom(1), ACT_NONE);
            b.release(a);
            rse_gate_shortcut(b, "neck.ins_conv." + std::to_string(tap), y);
            in[tap++] = y;
        }
    }
    b.release(h);
    RD_CHECK(tap == 4 && level == 5, "PPLCNetV3 det: four taps down to 1/32");

    rsefpn_db_tail(b, in, B, H, W, flags, out);
}

// ---------------------------------------------------------------------------------------------------
// PP-OCRv3 multilingual det (arch_config.yaml multi_PP-OCRv3_det_mobile = en_PP-OCRv3_det_mobile): MobileNetV3(scale 0.5, large,
// disable_se; backbones/det_mobilenet_v3.py) -> RSEFPN(96, shortcut) -> DBHead(k 50, no fix_nan).  Externals as build_ppocrv5_det_mobile;
// DET_WANT_STAGES (developer): ext[3..6] = the four stage features NCHW [B,16,H/4,.], [B,24,H/8,.], [B,56,H/16,.], [B,480,H/32,.].
// conv1 (3x3 / 2, 3 -> 8) is folded by the stem kernel's builder and writes convolution + bias; its hardswish runs in its consumer - on
// load in mbv3_block_kernel, or once through lcv3_act where block 0 is unfused (its consumer is then a matrix kernel).
// A block = expand 1x1 + act -> depthwise k x k / s + act -> linear 1x1 (+ input where s == 1 and cin == cout), every Conv + BatchNorm
// folded at load time.  Unfused: a ReLU block's expand applies ReLU in the matrix kernel's epilogue (ACT_RELU exists there); a hardswish
// block's expand writes convolution + bias and the depthwise kernel activates on load, inside the map only (hardswish is not in the
// shared epilogue: kernels_lcv3.hip says why); the linear layer adds the shortcut in its epilogue.  Fused: mbv3_block_kernel
// (kernels_mbv3.hip), per block by mbv3_fused_default / RD_MBV3_FUSED.  Every 1x1 route serves these channel counts (K % 4 == 0): no
// weight is padded.  The four stage outputs are linear (or conv_last + hardswish through lcv3_act) and feed ins_conv[i].in_conv, a plain
// 1x1 of K = 16 / 24 / 56 / 480 without bias.  head.thresh.* is in the file and unused in eval mode.
// ---------------------------------------------------------------------------------------------------
struct Mbv3Cfg { int stage, idx, k, cin, mid, cout, s, act; };
static const Mbv3Cfg kMbv3Det[15] = {
    {0, 0, 3, 8, 8, 8, 1, MBV3_RELU},       {0, 1, 3, 8, 32, 16, 2, MBV3_RELU},      {0, 2, 3, 16, 40, 16, 1, MBV3_RELU},
    {1, 0, 5, 16, 40, 24, 2, MBV3_RELU},    {1, 1, 5, 24, 64, 24, 1, MBV3_RELU},     {1, 2, 5, 24, 64, 24, 1, MBV3_RELU},
    {2, 0, 3, 24, 120, 40, 2, MBV3_HSWISH}, {2, 1, 3, 40, 104, 40, 1, MBV3_HSWISH},  {2, 2, 3, 40, 96, 40, 1, MBV3_HSWISH},
    {2, 3, 3, 40, 96, 40, 1, MBV3_HSWISH},  {2, 4, 3, 40, 240, 56, 1, MBV3_HSWISH},  {2, 5, 3, 56, 336, 56, 1, MBV3_HSWISH},
    {3, 0, 5, 56, 336, 80, 2, MBV3_HSWISH}, {3, 1, 5, 80, 480, 80, 1, MBV3_HSWISH},  {3, 2, 5, 80, 480, 80, 1, MBV3_HSWISH},
};
static const char* const kMbv3ConvLast = "backbone.stages.3.3";
static std::string mbv3_name(const Mbv3Cfg& c) { return "backbone.stages." + std::to_string(c.stage) + "." + std::to_string(c.idx); }

void derive_ppocrv3_det_mobile_weights(WeightStore& ws) {
    for (const Mbv3Cfg& c : kMbv3Det)       // (conv1 is folded by Builder::stem3x3s2, as every stem here)
        for (const char* layer : {".expand_conv", ".bottleneck_conv", ".linear_conv"}) fold_conv_bn(ws, mbv3_name(c) + layer, ".conv", ".bn");
    fold_conv_bn(ws, kMbv3ConvLast, ".conv", ".bn");
}

void build_ppocrv3_det_mobile(Builder& b, int B, int H, int W, int flags) {
    RD_CHECK(H % 32 == 0 && W % 32 == 0 && H >= 32 && W >= 32, "det v3 mobile input H, W must be multiples of 32");
    RD_CHECK((flags & ~(DET_WANT_NECK | DET_WANT_STAGES)) == 0, "det v3 mobile: unknown flag");
    TView x = b.external(0, B, H, W, 3);
    TView out = b.external(1, B, H, W, 1);

    TView h = b.stem3x3s2("backbone.conv.conv.weight", "backbone.conv.bn", x, ACT_NONE);
    bool raw = true;          // h is conv1's convolution + bias: its hardswish is still to come
    int level = 1, tap = 0;   // level: log2 of the current map's reduction of the page
    TView in[4];
    auto ins = [&](const TView& f) {        // a stage output -> ins_conv[tap] + RSE gate, while the stage's buffer is live
        const std::string p = "neck.ins_conv." + std::to_string(tap);
        if (flags & DET_WANT_STAGES) b.to_nchw(f, b.external(3 + tap, f.n, f.h, f.w, f.c));
        TView y = b.conv(p + ".in_conv.weight", "", "", f, geom(1), ACT_NONE);
        rse_gate_shortcut(b, p, y);
        in[tap++] = y;
    };
    for (int i = 0; i < 15; ++i) {
        const Mbv3Cfg& c = kMbv3Det[i];
        const std::string p = mbv3_name(c);
        RD_CHECK(h.c == c.cin, "MobileNetV3: channel chain: " + p);
        if (c.s == 2 && i > 2) ins(h);      // (det_mobilenet_v3.py: a stage ends in front of every stride-2 block past the third)
        const bool shortcut = c.s == 1 && c.cin == c.cout;
        TView y;
        if (!b.mbv3_block(p, h, c.k, c.s, c.act, raw, shortcut, level, &y)) {
            if (raw) {
                TView a = b.lcv3_act(h, Builder::Affine{});
                b.release(h);
                h = a;
            }
            const bool relu = c.act == MBV3_RELU;
            TView e = b.conv(p + ".expand_conv.fold.weight", p + ".expand_conv.fold.bias", "", h, geom(1), relu ? ACT_RELU : ACT_NONE);
            TView d = b.mbv3_dw(p + ".bottleneck_conv.fold.weight", p + ".bottleneck_conv.fold.bias", e, c.k, c.s, relu ? MBV3_NONE : MBV3_HSWISH, c.act, level);
            b.release(e);
            y = b.conv(p + ".linear_conv.fold.weight", p + ".linear_conv.fold.bias", "", d, geom(1), ACT_NONE, nullptr, shortcut ? &h : nullptr);
            b.release(d);
        }
        raw = false;
        b.release(h);
        h = y;
        if (c.s == 2) ++level;
        RD_CHECK(h.c == c.cout, "MobileNetV3: channel chain: " + p);
    }
    TView t = b.conv(std::string(kMbv3ConvLast) + ".fold.weight", std::string(kMbv3ConvLast) + ".fold.bias", "", h, geom(1), ACT_NONE);
    b.release(h);
    TView last = b.lcv3_act(t, Builder::Affine{});
    b.release(t);
    ins(last);
    b.release(last);
    RD_CHECK(tap == 4 && level == 5, "MobileNetV3 det: four stages down to 1/32");
    rsefpn_db_tail(b, in, B, H, W, flags, out);
}

// ---------------------------------------------------------------------------------------------------
// Text-line direction classifier (arch_config.yaml ch_ptocr_mobile_v2.0_cls_mobile): MobileNetV3(small, scale 0.35;
// backbones/rec_mobilenet_v3.py) -> no neck -> ClsHead(class_dim 2).  248 tensors.  conv1 (3x3 / (2,2), 3 -> 8) writes convolution + bias;
// its hardswish runs once through lcv3_act (block 0's expand is a matrix kernel).  Every block strides the height only.
// A block = expand 1x1 + act -> depthwise k x k / (s, 1) + act -> [SE over the ACTIVATED depthwise output: GAP -> 1x1 mid -> mid / 4 + ReLU ->
// 1x1 back -> paddle hard-sigmoid clamp(0.2 x + 0.5, 0, 1) -> scale] -> linear 1x1 (+ input where s == 1 and cin == cout); every
// Conv + BatchNorm folded in double at load time.  Activations as in build_ppocrv3_det_mobile: a ReLU expand activates in the matrix
// kernel's epilogue, a hardswish expand writes convolution + bias and mbv3s_dw_kernel activates on load, inside the map only.
// conv2 (1x1, 32 -> 200) writes convolution + bias; cls_tail_kernel does hardswish, MaxPool2d(2, 2), the average, the FC and the softmax,
// so the activated 200-channel map is never written.
// ---------------------------------------------------------------------------------------------------
struct Mbv3sCfg { int k, cin, mid, cout, s; bool se; int act; };
static const Mbv3sCfg kMbv3sCls[11] = {
    {3, 8, 8, 8, 2, true, MBV3_RELU},        {3, 8, 24, 8, 2, false, MBV3_RELU},      {3, 8, 32, 8, 1, false, MBV3_RELU},
    {5, 8, 32, 16, 2, true, MBV3_HSWISH},    {5, 16, 88, 16, 1, true, MBV3_HSWISH},   {5, 16, 88, 16, 1, true, MBV3_HSWISH},
    {5, 16, 40, 16, 1, true, MBV3_HSWISH},   {5, 16, 48, 16, 1, true, MBV3_HSWISH},   {5, 16, 104, 32, 2, true, MBV3_HSWISH},
    {5, 32, 200, 32, 1, true, MBV3_HSWISH},  {5, 32, 200, 32, 1, true, MBV3_HSWISH},
};
static const int kClsStageBlock[4] = {0, 3, 8, 10};

void derive_ppocr_cls_mobile_weights(WeightStore& ws) {
    for (int i = 0; i < 11; ++i)            // (conv1 is folded by Builder::stem3x3s2, as every stem here)
        for (const char* layer : {".expand_conv", ".bottleneck_conv", ".linear_conv"}) fold_conv_bn(ws, "backbone.blocks." + std::to_string(i) + layer, ".conv", ".bn");
    fold_conv_bn(ws, "backbone.conv2", ".conv", ".bn");
}

bool cls_mobile_geometry(int H, int W, int rows[4], int* cols) {
    if (H < 1 || W < 1) return false;
    int h = (H - 1) / 2 + 1;
    const int w = (W - 1) / 2 + 1;
    int tap = 0;
    for (int i = 0; i < 11; ++i) {
        h = (h - 1) / kMbv3sCls[i].s + 1;
        if (tap < 4 && i == kClsStageBlock[tap]) rows[tap++] = h;
    }
    *cols = w;
    return h >= 2 && w >= 2;       // MaxPool2d(2, 2) needs one whole window
}

void build_ppocr_cls_mobile(Builder& b, int B, int H, int W, int flags) {
    RD_CHECK((flags & ~(CLS_WANT_AUX | CLS_WANT_STAGES)) == 0, "text-line classifier: unknown flag");
    int rows[4], cols = 0;
    RD_CHECK(B >= 1 && cls_mobile_geometry(H, W, rows, &cols),
             "text-line classifier: input " + std::to_string(H) + " x " + std::to_string(W) + " leaves an empty map in front of the 2 x 2 max-pool (H >= 33 and W >= 3 are needed)");
    TView x = b.external(0, B, H, W, 3);
    TView prob = b.external(1, B, 1, 1, 2);
    // the fused route: the whole network in one launch, where cls_line_kernel holds the shape and RD_CLS_FUSED / the measured default say so
    {
        std::vector<Builder::ClsBlockDesc> blocks;
        for (int i = 0; i < 11; ++i) {
            const Mbv3sCfg& c = kMbv3sCls[i];
            blocks.push_back({"backbone.blocks." + std::to_string(i), c.k, c.cin, c.mid, c.cout, c.s, c.se, c.act});
        }
        TView aux{}, st[4];
        if (flags & CLS_WANT_AUX) aux = b.external(2, B, 1, 1, 2 + 200);
        if (flags & CLS_WANT_STAGES)
            for (int i = 0; i < 4; ++i) st[i] = b.external(3 + i, B, rows[i], cols, kMbv3sCls[kClsStageBlock[i]].cout);
        if (b.cls_line("backbone.conv1.conv.weight", "backbone.conv1.bn", blocks, "backbone.conv2.fold", "head.fc", x, prob, (flags & CLS_WANT_AUX) ? &aux : nullptr,
                       (flags & CLS_WANT_STAGES) ? st : nullptr, kClsStageBlock))
            return;
    }
    TView raw = b.stem3x3s2("backbone.conv1.conv.weight", "backbone.conv1.bn", x, ACT_NONE);
    TView h = b.lcv3_act(raw, Builder::Affine{});
    b.release(raw);
    int tap = 0;
    for (int i = 0; i < 11; ++i) {
        const Mbv3sCfg& c = kMbv3sCls[i];
        const std::string p = "backbone.blocks." + std::to_string(i);
        RD_CHECK(h.c == c.cin, "MobileNetV3 small: channel chain: " + p);
        const bool shortcut = c.s == 1 && c.cin == c.cout;
        const bool relu = c.act == MBV3_RELU;
        TView e = b.conv(p + ".expand_conv.fold.weight", p + ".expand_conv.fold.bias", "", h, geom(1), relu ? ACT_RELU : ACT_NONE);
        RD_CHECK(e.c == c.mid, "MobileNetV3 small: expanded width: " + p);
        TView d = b.mbv3s_dw(p + ".bottleneck_conv.fold.weight", p + ".bottleneck_conv.fold.bias", e, c.k, c.s, 1, relu ? MBV3_NONE : MBV3_HSWISH, c.act);
        b.release(e);
        if (c.se) {
            const std::string s = p + ".mid_se.";
            TView gate = b.se_gate(s + "conv1.weight", s + "conv1.bias", s + "conv2.weight", s + "conv2.bias", d, ACT_HSIG_PADDLE);
            b.scale(d, gate, 0.f, d);      // d * gate, in place
            b.release(gate);
        }
        TView y = b.conv(p + ".linear_conv.fold.weight", p + ".linear_conv.fold.bias", "", d, geom(1), ACT_NONE, nullptr, shortcut ? &h : nullptr);
        b.release(d);
        b.release(h);
        h = y;
        RD_CHECK(h.c == c.cout, "MobileNetV3 small: channel chain: " + p);
        if ((flags & CLS_WANT_STAGES) && tap < 4 && i == kClsStageBlock[tap]) {
            b.to_nchw(h, b.external(3 + tap, h.n, h.h, h.w, h.c));
            ++tap;
        }
    }
    TView t = b.conv("backbone.conv2.fold.weight", "backbone.conv2.fold.bias", "", h, geom(1), ACT_NONE);
    b.release(h);
    if (flags & CLS_WANT_AUX) {
        TView aux = b.external(2, B, 1, 1, 2 + t.c);
        b.cls_tail("head.fc", t, prob, &aux);
    } else {
        b.cls_tail("head.fc", t, prob, nullptr);
    }
    b.release(t);
}

// =================================================================================================
// UniTable table-structure encoder (unitable_modules.py Encoder): ImgLinearBackbone (Conv2d(3, 768, 16, stride 16), flattened to token
// rows) + PositionEmbedding + 12 nn.TransformerEncoderLayer (norm_first, erf GELU, eps 1e-5) + LayerNorm (eps 1e-6)
// =================================================================================================
static const int kVitD = 768, kVitHeads = 12, kVitLayers = 12, kVitPatch = 16, kVitMaxT = 1024;

void derive_unitable_encoder_weights(WeightStore& ws) {
    // conv_proj [768][3][16][16] read as the [768][768] matrix of the patch GEMM: Builder::vit_patchify gathers a patch in (c, ky, kx) order,
    // the order of the weight's rows as they are stored
    const HostTensor& w = ws.get("backbone.conv_proj.weight");
    RD_CHECK(w.shape.size() == 4 && w.shape[0] == kVitD && w.shape[1] == 3 && w.shape[2] == kVitPatch && w.shape[3] == kVitPatch,
             "unitable encoder: backbone.conv_proj.weight must be [768,3,16,16]");
    ws.add_derived("backbone.conv_proj.patch.weight", {kVitD, 3 * kVitPatch * kVitPatch}, std::vector<float>(w.f32(), w.f32() + w.numel()));
}

void build_unitable_encoder(Builder& b, int B, int H, int W, int flags) {
    RD_CHECK((flags & ~VIT_WANT_TAPS) == 0, "unitable encoder: unknown flag");
    RD_CHECK(B >= 1 && H >= kVitPatch && W >= kVitPatch && H % kVitPatch == 0 && W % kVitPatch == 0,
             "unitable encoder: input " + std::to_string(H) + " x " + std::to_string(W) + ": H and W must be multiples of 16");
    const int T = (H / kVitPatch) * (W / kVitPatch);
    RD_CHECK(T <= kVitMaxT, "unitable encoder: " + std::to_string(T) + " patches, the position table holds 1024");
    const bool taps = (flags & VIT_WANT_TAPS) != 0;
    TView x = b.external(0, B, H, W, 3);
    TView memory = b.external(1, B, 1, T, kVitD);
    TView patches = b.vit_patchify(x);
    TView t = b.conv("backbone.conv_proj.patch.weight", "backbone.conv_proj.bias", "", patches, geom(1), ACT_NONE);
    b.release(patches);
    if (taps) b.copy(t, b.external(2, B, 1, T, kVitD));
    b.add_pos("pos_embed.embedding.weight", t, B, T);
    for (int i = 0; i < kVitLayers; ++i) {
        const std::string p = "encoder.layers." + std::to_string(i);
        TView y = b.layernorm(p + ".norm1", t, 1e-5f);
        TView qkv = b.conv(p + ".self_attn.in_proj_weight", p + ".self_attn.in_proj_bias", "", y, geom(1), ACT_NONE);
        b.release(y);
        TView a = b.vit_attention(qkv, B, T, kVitHeads);
        b.release(qkv);
        TView t2 = b.linear(p + ".self_attn.out_proj", a, ACT_NONE, nullptr, &t);
        b.release(a);
        b.release(t);
        TView y2 = b.layernorm(p + ".norm2", t2, 1e-5f);
        TView m = b.linear(p + ".linear1", y2, ACT_GELU);
        b.release(y2);
        t = b.linear(p + ".linear2", m, ACT_NONE, nullptr, &t2);
        b.release(m);
        b.release(t2);
        if (taps && (i == 0 || i == kVitLayers - 1)) b.copy(t, b.external(i == 0 ? 3 : 4, B, 1, T, kVitD));
    }
    // the final LayerNorm writes into a workspace buffer; the result leaves through one copy (a [B,T,768] tensor is NHWC [B,1,T,768] as it is)
    TView n = b.layernorm("norm", t, 1e-6f);
    b.release(t);
    b.copy(n, memory);
    b.release(n);
}

// =================================================================================================
// The model table: one row per engine kind (ModelDesc, engine.h).  A new kind is a builder above and a row here.
// =================================================================================================
const std::vector<ModelDesc>& model_table() {
    using F = ModelFamily;
    static const std::vector<ModelDesc::Geom> page = {{1, 64, 64, 0}}, line = {{1, 48, 64, 0}, {1, 48, 64, REC_UNFUSED_CTC}};
    // kind, family, build, derive, PREPARE geometries, (n_classes, rec_token_dim) tensors, REC_LINE_WIDTHS, DET_WANT_NECK, derived tensors
    static const std::vector<ModelDesc> table = {
        {"ppocrv6_det", F::Detector, build_ppocrv6_det, nullptr, page, nullptr, nullptr, false, false, false},
        {"ppocrv5_det_server", F::Detector, build_ppocrv5_det_server, derive_ppocrv5_det_server_weights, page, nullptr, nullptr, false, true, false},
        {"ppocrv5_det_mobile", F::Detector, build_ppocrv5_det_mobile, derive_ppocrv5_det_mobile_weights, page, nullptr, nullptr, false, true, true},
        {"ppocrv3_det_mobile", F::Detector, build_ppocrv3_det_mobile, derive_ppocrv3_det_mobile_weights, page, nullptr, nullptr, false, true, true},
        {"ppocrv6_rec", F::Recogniser, build_ppocrv6_rec, nullptr, line, "head.head.weight" /* torch.py:112-116 */,
         "head.encoder.conv_block.0.convolution.weight", true, false, false},
        {"ppocrv5_rec_server", F::Recogniser, build_ppocrv5_rec_server, nullptr, line, "head.ctc_head.fc.weight",
         "head.ctc_encoder.encoder.conv1.conv.weight", false, false, false},
        {"ppocrv5_rec_mobile", F::Recogniser, build_ppocrv5_rec_mobile, derive_ppocrv5_rec_mobile_weights, line, "head.ctc_head.fc.weight",
         "head.ctc_encoder.encoder.conv1.conv.weight", true, false, false},
        {"ppocr_rec_mv1e", F::Recogniser, build_ppocr_rec_mv1e, derive_ppocr_rec_mv1e_weights, line, "head.fc.weight", "neck.encoder.conv1.conv.weight", true,
         false, false},
        {"ppocr_cls_mobile", F::Classifier, build_ppocr_cls_mobile, derive_ppocr_cls_mobile_weights, {{1, 48, 192, 0}}, nullptr, nullptr, false, false, false},
        {"unitable_encoder", F::TableEncoder, build_unitable_encoder, derive_unitable_encoder_weights, {{1, 16, 16, 0}}, nullptr, nullptr, false, false, false},
        {"pphgnetv2_b4", F::Backbone, build_pphgnetv2_b4, nullptr, page, nullptr, nullptr, false, false, false},
        {"pphgnetv2_b6_formula", F::FormulaEncoder, build_pphgnetv2_b6_formula, nullptr, page, nullptr, nullptr, false, false, false},
    };
    return table;
}

const ModelDesc* find_model(const std::string& kind) {
    for (const ModelDesc& m : model_table())
        if (kind == m.kind) return &m;
    return nullptr;
}

}  // namespace rd
