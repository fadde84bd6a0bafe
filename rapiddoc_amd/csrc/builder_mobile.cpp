// The Builder operators of the mobile backbones - PPLCNetV3 (kernels_lcv3*.hip), MobileNetV1Enhance (kernels_mv1e.hip), MobileNetV3
// (kernels_mbv3.hip) and MobileNetV3 small (kernels_mbv3s.hip) - with their per-layer default route tables (`*_default`) and the
// measurements that set them.
#include <cstdlib>
#include <cstring>

#include "builder_util.h"
#include "engine.h"

namespace rd {

Builder::Affine Builder::affine(const std::string& prefix) const {
    const HostTensor& sc = ws_->get(prefix + ".scale");
    const HostTensor& bi = ws_->get(prefix + ".bias");
    RD_CHECK(sc.numel() == 1 && bi.numel() == 1, "scalar affine expected: " + prefix);
    return Affine{sc.f32()[0], bi.f32()[0]};
}

// Shared by both PPLCNetV3 depthwise builders: checks, the output view, in PREPARE mode the [k*k][C] weight image + bias, in PLAN mode
// the kernel parameters (pointers of x / y are filled in at run time) and the op's record without its `run`
bool Builder::lcv3_dw_common(const std::string& wname, const std::string& bname, const TView& x, int k, int sh, int sw, const Affine* pre,
                             const Affine* post, TView* y_out, Lcv3DwParams* p_out, OpRecord* r_out) {
    const HostTensor& w = ws_->get(wname);
    RD_CHECK(w.shape.size() == 4 && w.shape[1] == 1 && w.shape[2] == k && w.shape[3] == k, "lcv3 depthwise weight shape: " + wname);
    const int c = (int)w.shape[0];
    RD_CHECK(c == x.c && lcv3_dw_shape_ok(k, sh, sw, c), "lcv3 depthwise geometry: " + wname);
    const int oh = out_dim(x.h, k, sh, k / 2, k / 2), ow = out_dim(x.w, k, sw, k / 2, k / 2);
    TView y = alloc(x.n, oh, ow, c);
    *y_out = y;
    const std::string key = wname + "|lcv3dw";
    if (!planning()) {
        if (!pb_->has(key + "#w")) {
            pb_->add(key + "#w", fold_dw_taps(w.f32(), c, k * k));
            pb_->add(key + "#b", std::vector<float>(ws_->get(bname).f32(), ws_->get(bname).f32() + c));
        }
        return false;
    }
    Lcv3DwParams p{};
    p.xld = plan_->ld(x);
    p.N = x.n; p.H = x.h; p.W = x.w; p.C = c;
    p.w = pb_->ptr(key + "#w");
    p.bias = pb_->ptr(key + "#b");
    p.yld = plan_->ld(y);
    p.OH = oh; p.OW = ow; p.K = k; p.SH = sh; p.SW = sw;
    p.pre_act = pre != nullptr;
    p.pre_s = pre ? pre->s : 1.f; p.pre_b = pre ? pre->b : 0.f;
    p.post_act = post != nullptr;
    p.post_s = post ? post->s : 1.f; p.post_b = post ? post->b : 0.f;
    RD_CHECK(p.xld % 4 == 0 && x.coff % 4 == 0, "lcv3 depthwise: 16-byte aligned pixels");
    *p_out = p;
    r_out->name = wname;
    r_out->kind = "lcv3_dw" + std::to_string(k) + "x" + std::to_string(k);
    r_out->shape = shape_str(x, {c});
    r_out->flops = 2.0 * x.n * oh * ow * (double)c * k * k;
    r_out->bytes = 4.0 * ((double)x.pixels() * c + (double)y.pixels() * c);
    return true;
}

// Per-geometry default of MobileNetV1Enhance's 5x5 depthwise route, from the same-run alternating A/B of tools/mb_rec_mv1e.py on the same
// operands, 64 lines at w2 = 544 (profiles/mb_rec_mv1e.txt; docs/notebook/rec_mv1e.md).  Direct / strip ms (median of 7 rounds of 20 launches;
// every round of the strip kernel below every round of the direct one):
//   C 256, 6 rows, s (1,1)   0.236 / 0.148      C 256, 6 rows, s (2,1)   0.133 / 0.113      C 512, 3 rows, s (1,2)   0.160 / 0.131
// A (stride, C) that was not measured stays on the direct kernel.
bool mv1e_dw_strip_default(int sh, int sw, int c) {
    return (sh == 1 && sw == 1 && c == 256) || (sh == 2 && sw == 1 && c == 256) || (sh == 1 && sw == 2 && c == 512);
}

TView Builder::lcv3_dw(const std::string& wname, const std::string& bname, const TView& x, int k, int sh, int sw, const Affine* pre, Affine post,
                       int lt_in, int lt_out, int strip) {
    TView y{};
    Lcv3DwParams p{};
    OpRecord r;
    if (!lcv3_dw_common(wname, bname, x, k, sh, sw, pre, &post, &y, &p, &r)) return y;
    bool staged = false;      // the route is a property of the layer's geometry, never of the batch or the line widths
    if (strip && dw5_strip_launch_ok(p))
        staged = route_switch(strip == 1 ? "RD_LCV3_DW_STRIP" : "RD_MV1E_DW_STRIP", strip == 2 && mv1e_dw_strip_default(sh, sw, p.C));
    r.cfg = "s" + std::to_string(sh) + std::to_string(sw) + (staged ? "/strip" : "") + (has_lt_ ? "/lines" : "");
    const TView xv = x, yv = y, ltv = lt_;
    const bool has_lt = has_lt_;
    r.run = [p, xv, yv, ltv, has_lt, lt_in, lt_out, staged](const Plan& pl, const RunCtx& cx) {
        Lcv3DwParams q = p;
        q.x = pl.vptr(xv, cx);
        q.y = pl.vptr(yv, cx);
        if (has_lt) {
            const int32_t* lt = reinterpret_cast<const int32_t*>(pl.vptr(ltv, cx));
            q.line_in = lt + lt_in;
            q.line_out = lt + lt_out;
            q.line_stride = kLineTabStride;
        }
        if (staged) (void)launch_dw5_strip(q, cx.stream);      // (servable: checked above)
        else launch_lcv3_dw(q, cx.stream);
    };
    emit(std::move(r));
    return y;
}

TView Builder::mv1e_pool(const TView& x, const TView* out) {
    RD_CHECK(x.h == 3 && x.w >= 2 && x.c % 4 == 0, "mv1e pool: a 3-row map");
    const int ow = x.w / 2;
    TView y = out ? *out : alloc(x.n, 1, ow, x.c);
    RD_CHECK(y.n == x.n && y.h == 1 && y.w == ow && y.c == x.c, "mv1e pool: output view mismatch");
    if (!planning()) return y;
    RD_CHECK(plan_->ld(x) % 4 == 0 && x.coff % 4 == 0 && plan_->ld(y) % 4 == 0 && y.coff % 4 == 0, "mv1e pool: 16-byte aligned pixels");
    OpRecord r;
    r.name = "hswish+avgpool2x2";
    r.kind = "pool";
    r.bytes = 4.0 * (2.0 * x.n * x.w * x.c + y.pixels() * y.c);
    const TView xv = x, yv = y, ltv = lt_;
    const bool has_lt = has_lt_;
    r.run = [xv, yv, ltv, has_lt](const Plan& pl, const RunCtx& c) {
        launch_mv1e_pool(pl.vptr(xv, c), pl.ld(xv), pl.vptr(yv, c), pl.ld(yv), xv.n, xv.h, xv.w, xv.c, c.stream,
                         has_lt ? reinterpret_cast<const int32_t*>(pl.vptr(ltv, c)) : nullptr);
    };
    emit(std::move(r));
    return y;
}

// Per-layer default of the detector's depthwise route, from the same-run alternating A/B of tools/mb_det_mobile.py at [32, 3, 960, 704]
// (profiles/mb_det_mobile.txt): the LDS-staged kernel where its median was below the direct kernel's by more than either route's own
// repeat spread, the direct kernel everywhere else (it is the simpler one).  Direct / staged ms of the measured layers:
//   k 3 s 1  C 16 @ 1/2   0.229 / 0.154    k 3 s 2  C 32 @ 1/2   0.208 / 0.259 (direct stays)    k 5 s 1  C 192 @ 1/16  0.083 / 0.050
//   k 3 s 1  C 48 @ 1/4   0.183 / 0.146    k 3 s 2  C 48 @ 1/4   0.087 / 0.103 (direct stays)    k 5 s 2  C 192 @ 1/16  0.051 / 0.044
//   k 3 s 1  C 96 @ 1/8   0.087 / 0.074    k 3 s 2  C 96 @ 1/8   0.037 / 0.056 (direct stays)    k 5 s 1  C 384 @ 1/32  0.046 / 0.026
// A (k, stride, C, level) that was not measured stays on the direct kernel.
bool lcv3_dw2d_default(int k, int stride, int c, int level) {
    if (k == 3 && stride == 1) return (c == 16 && level == 1) || (c == 48 && level == 2) || (c == 96 && level == 3);
    if (k == 5 && stride == 1) return (c == 192 && level == 4) || (c == 384 && level == 5);
    if (k == 5 && stride == 2) return c == 192 && level == 4;
    return false;
}

TView Builder::lcv3_dw_det(const std::string& wname, const std::string& bname, const TView& x, int k, int stride, const Affine* pre, const Affine* post,
                           int level) {
    RD_CHECK(stride == 1 || stride == 2, "lcv3 depthwise (detector geometry): stride 1 or 2: " + wname);
    RD_CHECK(!has_lt_, "lcv3 depthwise (detector geometry): no line table");
    TView y{};
    Lcv3DwParams p{};
    OpRecord r;
    if (!lcv3_dw_common(wname, bname, x, k, stride, stride, pre, post, &y, &p, &r)) return y;
    // the route is a property of the layer (k, stride, C, pyramid level), never of the batch or the page size; A/B switch read per plan
    const bool staged = lcv3_dw2d_shape_ok(k, stride, stride, p.C) && route_switch("RD_LCV3_DW2D", lcv3_dw2d_default(k, stride, p.C, level));
    RD_CHECK(!staged || lcv3_dw2d_launch_ok(p), "lcv3 depthwise: the staged kernel's grid does not fit: " + wname);
    r.cfg = "s" + std::to_string(stride) + std::to_string(stride) + (staged ? "/lds2d" : "/direct") + (post ? "" : "/noact");
    r.run = staged ? run_xy(p, x, y, launch_lcv3_dw2d) : run_xy(p, x, y, launch_lcv3_dw);      // (the staged kernel: servable, checked above)
    emit(std::move(r));
    return y;
}

TView Builder::lcv3_act(const TView& x, Affine a) {
    RD_CHECK(x.c % 4 == 0, "lcv3 act: channels % 4");
    TView y = alloc(x.n, x.h, x.w, x.c);
    if (!planning()) return y;
    RD_CHECK(plan_->ld(x) % 4 == 0 && x.coff % 4 == 0, "lcv3 act: 16-byte aligned pixels");
    OpRecord r;
    r.name = "hswish+affine";
    r.kind = "lcv3_act";
    r.bytes = 8.0 * x.pixels() * x.c;
    const TView xv = x, yv = y;
    r.run = [xv, yv, a](const Plan& pl, const RunCtx& cx) {
        launch_lcv3_act(pl.vptr(xv, cx), pl.ld(xv), pl.vptr(yv, cx), pl.ld(yv), (long)xv.pixels(), xv.c, a.s, a.b, cx.stream);
    };
    emit(std::move(r));
    return y;
}

// ---- MobileNetV3 (kernels_mbv3.hip)
// Per-layer default of the hardswish depthwise layers with C % 16 == 0: true = lcv3_dw2d_kernel (kernels_lcv3_det.hip), by the same rule, from
// the per-layer A/B of tools/mb_det_v3_mobile.py --routes (docs/notebook/v3_mobile_det.md); a layer that was not measured stays direct.
//   direct / staged ms at 32 pages (median of 7 repeats of 40 launches, alternating; spreads 0.5 - 9.5 %):
//   k 3 s 1  C 96 @ 1/16   0.0290 / 0.0235      k 3 s 1  C 240 @ 1/16  0.0622 / 0.0501      k 3 s 1  C 336 @ 1/16  0.0865 / 0.0679
//   k 5 s 1  C 480 @ 1/32  0.0759 / 0.0353      k 5 s 2  C 336 @ 1/16  0.0700 / 0.0739 (direct stays)
bool mbv3_dw2d_default(int k, int stride, int c, int level) {
    if (k == 3 && stride == 1) return (c == 96 || c == 240 || c == 336) && level == 4;
    if (k == 5 && stride == 1) return c == 480 && level == 5;
    return false;
}

// What differs between the parameter structs of the two MobileNetV3 depthwise kernels (mbv3_dw_kernel: one stride; mbv3s_dw_kernel: row and
// column strides): the rest of mbv3_dw_common is the same for both
static bool mbv3_shape_ok(const Mbv3DwParams&, int k, int sh, int, int c) { return mbv3_dw_shape_ok(k, sh, c); }
static bool mbv3_shape_ok(const Mbv3sDwParams&, int k, int sh, int sw, int c) { return mbv3s_dw_shape_ok(k, sh, sw, c); }
static void mbv3_set_strides(Mbv3DwParams& p, int sh, int) { p.S = sh; }
static void mbv3_set_strides(Mbv3sDwParams& p, int sh, int sw) { p.SH = sh; p.SW = sw; }
static bool mbv3_launch_ok(const Mbv3DwParams& p) { return mbv3_dw_launch_ok(p); }
static bool mbv3_launch_ok(const Mbv3sDwParams& p) { return mbv3s_dw_launch_ok(p); }
static const char* const kMbv3ActName[3] = {"none", "relu", "hswish"};

// Shared by mbv3_dw and mbv3s_dw (`net` = "mbv3" / "mbv3s": error texts, the parameter-block key `wname|<net>dw` and the op kind): checks,
// the output view, in PREPARE mode the [k*k][C] weight image + bias, in PLAN mode the kernel parameters (pointers of x / y are filled in
// at run time) and the op's record without its `cfg` and `run`; false in PREPARE mode
template <typename P>
bool Builder::mbv3_dw_common(const std::string& net, const std::string& wname, const std::string& bname, const TView& x, int k, int sh, int sw, int pre_act,
                             int post_act, TView* y_out, P* p_out, OpRecord* r_out) {
    const HostTensor& w = ws_->get(wname);
    RD_CHECK(w.shape.size() == 4 && w.shape[1] == 1 && w.shape[2] == k && w.shape[3] == k, net + " depthwise weight shape: " + wname);
    const int c = (int)w.shape[0];
    RD_CHECK(c == x.c && mbv3_shape_ok(*p_out, k, sh, sw, c), net + " depthwise geometry: " + wname);
    RD_CHECK(!has_lt_, net + " depthwise: no line table");
    const int oh = (x.h - 1) / sh + 1, ow = (x.w - 1) / sw + 1;
    TView y = alloc(x.n, oh, ow, c);
    *y_out = y;
    const std::string key = wname + "|" + net + "dw";
    if (!planning()) {
        if (!pb_->has(key + "#w")) {
            pb_->add(key + "#w", fold_dw_taps(w.f32(), c, k * k));
            pb_->add(key + "#b", std::vector<float>(ws_->get(bname).f32(), ws_->get(bname).f32() + c));
        }
        return false;
    }
    P p{};
    p.xld = plan_->ld(x);
    p.N = x.n; p.H = x.h; p.W = x.w; p.C = c;
    p.w = pb_->ptr(key + "#w");
    p.bias = pb_->ptr(key + "#b");
    p.yld = plan_->ld(y);
    p.OH = oh; p.OW = ow; p.K = k;
    mbv3_set_strides(p, sh, sw);
    p.pre_act = pre_act; p.post_act = post_act;
    RD_CHECK(mbv3_launch_ok(p) && x.coff % 4 == 0 && y.coff % 4 == 0, net + " depthwise: 16-byte aligned pixels: " + wname);
    *p_out = p;
    r_out->name = wname;
    r_out->kind = net + "_dw" + std::to_string(k) + "x" + std::to_string(k);
    r_out->shape = shape_str(x, {c});
    r_out->flops = 2.0 * x.n * oh * ow * (double)c * k * k;
    r_out->bytes = 4.0 * ((double)x.pixels() * c + (double)y.pixels() * c);
    return true;
}

TView Builder::mbv3_dw(const std::string& wname, const std::string& bname, const TView& x, int k, int stride, int pre_act, int post_act, int level) {
    TView y{};
    Mbv3DwParams p{};
    OpRecord r;
    if (!mbv3_dw_common("mbv3", wname, bname, x, k, stride, stride, pre_act, post_act, &y, &p, &r)) return y;
    // hardswish on load AND in the epilogue, C % 16 == 0: the v5 mobile detector's LDS-staged kernel computes the same layer (identity affines)
    Lcv3DwParams sp{};
    sp.xld = p.xld; sp.N = p.N; sp.H = p.H; sp.W = p.W; sp.C = p.C; sp.w = p.w; sp.bias = p.bias; sp.yld = p.yld;
    sp.OH = p.OH; sp.OW = p.OW; sp.K = k; sp.SH = sp.SW = stride;
    sp.pre_act = 1; sp.pre_s = 1.f; sp.pre_b = 0.f; sp.post_act = 1; sp.post_s = 1.f; sp.post_b = 0.f;
    // A/B switch, read per plan; the route goes by the layer, never by batch or page size
    const bool staged = pre_act == MBV3_HSWISH && post_act == MBV3_HSWISH && lcv3_dw2d_launch_ok(sp) &&
                        route_switch("RD_MBV3_DW2D", mbv3_dw2d_default(k, stride, p.C, level));
    r.cfg = "s" + std::to_string(stride) + "/" + kMbv3ActName[pre_act] + ">" + kMbv3ActName[post_act] + (staged ? "/lds2d" : "");
    r.run = staged ? run_xy(sp, x, y, launch_lcv3_dw2d) : run_xy(p, x, y, launch_mbv3_dw);      // (servable: checked above)
    emit(std::move(r));
    return y;
}

// Per-block default of the MobileNetV3 route.  A block becomes fused only by the rule of docs/notebook/v5_mobile_det.md: routes alternating
// on the same operands at [32, 3, 960, 704] (tools/mb_det_v3_mobile.py --routes), the fused median below the unfused one by more than the
// larger of the two spreads.  The table and what it decided are in docs/notebook/v3_mobile_det.md; a (k, stride, cin, mid, level) that was
// not measured stays unfused.
//   block (k / s, cin-mid-cout @ level)   unfused / fused ms (median of 7 alternating profiled launches; spreads 0.6 - 7.2 %)
//   3 / 1   8-8-8   @ 1/2   0.787 / 0.313      3 / 2   8-32-16 @ 1/2   0.473 / 0.379      3 / 1  16-40-16 @ 1/4   0.451 / 0.248
//   5 / 2  16-40-24 @ 1/4   0.377 / 0.261      5 / 1  24-64-24 @ 1/8   0.234 / 0.191 and 0.230 / 0.190
// All five measured geometries win by more than either route's spread; the forward went from 6.11 to 5.20 ms.
bool mbv3_fused_default(int k, int stride, int cin, int mid, int level) {
    if (k == 3 && stride == 1) return (cin == 8 && mid == 8 && level == 1) || (cin == 16 && mid == 40 && level == 2);
    if (k == 3 && stride == 2) return cin == 8 && mid == 32 && level == 1;
    if (k == 5 && stride == 2) return cin == 16 && mid == 40 && level == 2;
    if (k == 5 && stride == 1) return cin == 24 && mid == 64 && level == 3;
    return false;
}

bool Builder::mbv3_block(const std::string& prefix, const TView& x, int k, int stride, int act, bool in_hswish, bool shortcut, int level, TView* y_out) {
    if (!planning()) return false;
    const std::string we = prefix + ".expand_conv.fold.weight", wd = prefix + ".bottleneck_conv.fold.weight", wl = prefix + ".linear_conv.fold.weight";
    const std::string ke = we + "|", kd = wd + "|mbv3dw", kl = wl + "|";
    if (!pb_->has(ke + "#w") || !pb_->has(ke + "#b") || !pb_->has(kd + "#w") || !pb_->has(kl + "#w") || !pb_->has(kl + "#b")) return false;
    Mbv3BlockParams p{};
    p.xld = plan_->ld(x);
    p.N = x.n; p.H = x.h; p.W = x.w; p.cin = x.c;
    p.mid = weight_dim(we, 0); p.cout = weight_dim(wl, 0);
    p.we = pb_->ptr(ke + "#w"); p.be = pb_->ptr(ke + "#b");
    p.wd = pb_->ptr(kd + "#w"); p.bd = pb_->ptr(kd + "#b");
    p.wl = pb_->ptr(kl + "#w"); p.bl = pb_->ptr(kl + "#b");
    p.OH = (x.h - 1) / stride + 1; p.OW = (x.w - 1) / stride + 1; p.K = k; p.S = stride;
    p.act = act; p.in_hswish = in_hswish; p.shortcut = shortcut;
    p.yld = p.cout;      // (the output is a fresh full-width buffer)
    if (weight_dim(we, 1) != x.c || weight_dim(wl, 1) != p.mid || has_lt_ || x.coff % 4 != 0 || !mbv3_block_launch_ok(p)) return false;
    // the route is a property of the layer (k, stride, cin, mid, pyramid level), never of the batch or the page size; A/B switch read per plan
    if (!route_switch("RD_MBV3_FUSED", mbv3_fused_default(k, stride, p.cin, p.mid, level))) return false;
    TView y = alloc(x.n, p.OH, p.OW, p.cout);
    RD_CHECK(plan_->ld(y) == p.yld, "mbv3 block: output row stride");
    OpRecord r;
    r.name = prefix;
    r.kind = "mbv3_block";
    r.cfg = "k" + std::to_string(k) + "s" + std::to_string(stride) + (act == MBV3_RELU ? "/relu" : "/hswish") + (in_hswish ? "/inact" : "") + (shortcut ? "/res" : "");
    r.shape = shape_str(x, {p.cin, p.mid, p.cout});
    r.flops = 2.0 * ((double)x.pixels() * p.cin * p.mid + (double)y.pixels() * p.mid * (k * k + p.cout));
    r.bytes = 4.0 * ((double)x.pixels() * p.cin + (double)y.pixels() * p.cout);
    r.run = run_xy(p, x, y, launch_mbv3_block);   // (servable: checked above)
    emit(std::move(r));
    *y_out = y;
    return true;
}

// ---- MobileNetV3 small in the text-line geometry (kernels_mbv3s.hip)
TView Builder::mbv3s_dw(const std::string& wname, const std::string& bname, const TView& x, int k, int sh, int sw, int pre_act, int post_act) {
    TView y{};
    Mbv3sDwParams p{};
    OpRecord r;
    if (!mbv3_dw_common("mbv3s", wname, bname, x, k, sh, sw, pre_act, post_act, &y, &p, &r)) return y;
    r.cfg = "s" + std::to_string(sh) + std::to_string(sw) + "/" + kMbv3ActName[pre_act] + ">" + kMbv3ActName[post_act];
    r.run = run_xy(p, x, y, launch_mbv3s_dw);      // (servable: checked in mbv3_dw_common)
    emit(std::move(r));
    return y;
}

void Builder::cls_tail(const std::string& prefix, const TView& x, const TView& prob_ext, const TView* aux_ext) {
    const HostTensor& w = ws_->get(prefix + ".weight");
    RD_CHECK(w.shape.size() == 2 && w.shape[0] == 2 && (int)w.shape[1] == x.c, "classifier head: Linear C -> 2: " + prefix);
    RD_CHECK(prob_ext.pixels() * prob_ext.c == (long)x.n * 2, "classifier head: probability view");
    if (aux_ext) RD_CHECK(aux_ext->pixels() * aux_ext->c == (long)x.n * (2 + x.c), "classifier head: aux view");
    const std::string key = prefix + "|clstail";
    if (!planning()) {
        if (!pb_->has(key + "#w")) {
            pb_->add(key + "#w", std::vector<float>(w.f32(), w.f32() + w.numel()));
            pb_->add(key + "#b", std::vector<float>(ws_->get(prefix + ".bias").f32(), ws_->get(prefix + ".bias").f32() + 2));
        }
        return;
    }
    ClsTailParams p{};
    p.xld = plan_->ld(x);
    p.N = x.n; p.H = x.h; p.W = x.w; p.C = x.c;
    p.w = pb_->ptr(key + "#w");
    p.bias = pb_->ptr(key + "#b");
    RD_CHECK(cls_tail_launch_ok(p), "classifier head: the map behind the backbone has no 2 x 2 window (or more than 1024 channels)");
    OpRecord r;
    r.name = prefix;
    r.kind = "cls_tail";
    r.cfg = "hswish>maxpool2>gap>fc2>softmax";
    r.shape = shape_str(x, {x.c});
    r.flops = (double)x.n * (4.0 * x.c + 5.0 * x.h * x.w * x.c);
    r.bytes = 4.0 * (double)x.pixels() * x.c;
    const TView xv = x, pv = prob_ext, av = aux_ext ? *aux_ext : TView{};
    const bool has_aux = aux_ext != nullptr;
    r.run = [p, xv, pv, av, has_aux](const Plan& pl, const RunCtx& cx) {
        ClsTailParams q = p;
        q.x = pl.vptr(xv, cx);
        q.prob = pl.vptr(pv, cx);
        q.aux = has_aux ? pl.vptr(av, cx) : nullptr;
        (void)launch_cls_tail(q, cx.stream);      // (servable: checked above)
    };
    emit(std::move(r));
}

// Default route of the text-line classifier, by the project's rule (docs/notebook/v5_mobile_det.md): the fused kernel only where its median
// lies below the unfused chain's by more than the larger of the two spreads, alternating in one run (tools/mb_cls_mobile.py,
// profiles/mb_cls_mobile.txt).  Measured, unfused / fused ms per forward at [B, 3, 48, 192] (median of 7 alternating rounds, spreads 0.1 - 1.4 %):
//   B = 6      0.584 / 1.527 (auto)   0.600 / 1.529 (fp32)        B = 1440   3.814 / 8.225 (auto)   3.766 / 8.228 (fp32)
// cls_line_kernel loses at both sizes (one line is 1.5 ms of dependent phases on eight wavefronts, its weights read from global memory per
// FMA quad; docs/notebook/cls_mobile.md), so the chain of separate operators - replayed as one hipGraph - is the default.
bool cls_fused_default() { return false; }

bool Builder::cls_line(const std::string& stem_w, const std::string& stem_bn, const std::vector<ClsBlockDesc>& blocks, const std::string& conv2,
                       const std::string& head, const TView& x, const TView& prob_ext, const TView* aux_ext, const TView* stages, const int* stage_block) {
    if (!planning() || has_lt_ || blocks.size() > 11) return false;
    if (!route_switch("RD_CLS_FUSED", cls_fused_default())) return false;
    const std::string ks = stem_w + "|" + stem_bn + "|stem", k2 = conv2 + ".weight|", kh = head + "|clstail";
    if (!pb_->has(ks + "#w") || !pb_->has(k2 + "#w") || !pb_->has(k2 + "#b") || !pb_->has(kh + "#w")) return false;
    ClsLineParams p{};
    p.B = x.n; p.H = x.h; p.W = x.w;
    p.w1c = pb_->ptr(ks + "#w"); p.b1c = pb_->ptr(ks + "#b"); p.c1 = weight_dim(stem_w, 0);
    p.n_blocks = (int)blocks.size();
    for (size_t i = 0; i < blocks.size(); ++i) {
        const ClsBlockDesc& d = blocks[i];
        const std::string ke = d.prefix + ".expand_conv.fold.weight|", kd = d.prefix + ".bottleneck_conv.fold.weight|mbv3sdw",
                          kl = d.prefix + ".linear_conv.fold.weight|", se = d.prefix + ".mid_se.";
        if (!pb_->has(ke + "#w") || !pb_->has(ke + "#b") || !pb_->has(kd + "#w") || !pb_->has(kl + "#w") || !pb_->has(kl + "#b")) return false;
        if (d.se && !pb_->has(se + "conv1.weight")) return false;
        ClsBlockParams& L = p.blk[i];
        L.we = pb_->ptr(ke + "#w"); L.be = pb_->ptr(ke + "#b");
        L.wd = pb_->ptr(kd + "#w"); L.bd = pb_->ptr(kd + "#b");
        L.wl = pb_->ptr(kl + "#w"); L.bl = pb_->ptr(kl + "#b");
        if (d.se) {
            L.w1 = pb_->ptr(se + "conv1.weight"); L.b1 = pb_->ptr(se + "conv1.bias");
            L.w2 = pb_->ptr(se + "conv2.weight"); L.b2 = pb_->ptr(se + "conv2.bias");
        }
        L.k = d.k; L.cin = d.cin; L.mid = d.mid; L.cout = d.cout; L.sh = d.sh;
        L.se = d.se ? 1 : 0; L.act = d.act; L.shortcut = d.sh == 1 && d.cin == d.cout;
    }
    p.w2c = pb_->ptr(k2 + "#w"); p.b2c = pb_->ptr(k2 + "#b"); p.c2 = weight_dim(conv2 + ".weight", 0);
    p.wf = pb_->ptr(kh + "#w"); p.bf = pb_->ptr(kh + "#b");
    for (int i = 0; i < 4; ++i) p.stage_block[i] = stage_block[i];
    if (weight_dim(conv2 + ".weight", 1) != 32 || !cls_line_plan(p)) return false;      // a shape the kernel cannot hold: the separate operators take it
    TView scratch = alloc_raw(cls_line_scratch_floats(p));
    OpRecord r;
    r.name = "backbone+head";
    r.kind = "cls_line";
    r.cfg = "fused/" + std::to_string(p.n_blocks) + "blocks";
    r.shape = shape_str(x);
    r.bytes = 4.0 * (double)x.n * 3 * x.h * x.w;
    const TView xv = x, pv = prob_ext, av = aux_ext ? *aux_ext : TView{}, sv = scratch;
    const bool has_aux = aux_ext != nullptr, has_st = stages != nullptr;
    TView stv[4];
    for (int i = 0; i < 4; ++i) stv[i] = has_st ? stages[i] : TView{};
    r.run = [p, xv, pv, av, sv, has_aux, has_st, stv](const Plan& pl, const RunCtx& cx) {
        ClsLineParams q = p;
        q.x = pl.vptr(xv, cx);
        q.prob = pl.vptr(pv, cx);
        q.aux = has_aux ? pl.vptr(av, cx) : nullptr;
        for (int i = 0; i < 4; ++i) q.stage_out[i] = has_st ? pl.vptr(stv[i], cx) : nullptr;
        q.scratch = pl.vptr(sv, cx);
        (void)launch_cls_line(q, cx.stream);      // (servable: planned above)
    };
    emit(std::move(r));
    release(scratch);
    return true;
}

// the fused block's own parameters: the pointwise weights [cout][cin] as fp32 (the kernel splits them once per workgroup) + bias, for layers
// whose weights fit the fp16 range.  Prepared for every handle (28 KB over the three blocks): plans pick the route later, per plan
void Builder::prepare_lcv3_block(const std::string& key, const HostTensor& w, const std::string& pw_b) {
    if (pb_->has(key + "#w")) return;
    const int cout = (int)w.shape[0], cin = (int)w.shape[1];
    std::vector<float> wf(w.f32(), w.f32() + (size_t)cout * cin);
    if (!fits_fp16_range(wf)) return;
    pb_->add(key + "#w", wf);
    pb_->add(key + "#b", std::vector<float>(ws_->get(pw_b).f32(), ws_->get(pw_b).f32() + cout));
}

bool Builder::lcv3_block(const std::string& dw_w, const std::string& pw_w, const std::string& pw_b, const TView& x, const Affine* pre, Affine mid,
                         int lt_col, TView* y_out) {
    const HostTensor& w = ws_->get(pw_w);
    const int cout = (int)w.shape[0], cin = (int)w.shape[1];
    if (cin != x.c || !lcv3_block_shape_ok(cin, cout)) return false;
    const std::string key = pw_w + "|lcv3blk", dkey = dw_w + "|lcv3dw";
    if (!planning()) {          // PREPARE: the parameters only; the caller goes on to prepare the separate operators, whose depthwise
        prepare_lcv3_block(key, w, pw_b);   // parameters this kernel shares
        return false;
    }
    const bool on = rd_env_on("RD_LCV3_FUSED");   // A/B switch, read per plan
    if (!on || !(h3_ || mixer_h3_) || !pb_->has(key + "#w") || !pb_->has(dkey + "#w") || plan_->ld(x) % 4 != 0 || x.coff % 4 != 0) return false;
    TView y = alloc(x.n, x.h, x.w, cout);
    Lcv3BlockParams p{};
    p.xld = plan_->ld(x);
    p.N = x.n; p.H = x.h; p.W = x.w; p.cin = cin; p.cout = cout;
    p.dw_w = pb_->ptr(dkey + "#w"); p.dw_b = pb_->ptr(dkey + "#b");
    p.pw_w = pb_->ptr(key + "#w"); p.pw_b = pb_->ptr(key + "#b");
    p.yld = plan_->ld(y);
    p.pre_act = pre != nullptr;
    p.pre_s = pre ? pre->s : 1.f; p.pre_b = pre ? pre->b : 0.f; p.mid_s = mid.s; p.mid_b = mid.b;
    p.out_act = 0; p.out_s = 1.f; p.out_b = 0.f;
    p.split = 1; p.range_flag = range_flag_;
    OpRecord r;
    r.name = pw_w;
    r.kind = "lcv3_block";
    r.cfg = has_lt_ ? "h3/lines" : "h3";
    r.shape = shape_str(x, {cin, cout});
    r.flops = 2.0 * x.pixels() * (double)cin * (9 + cout);
    r.bytes = 4.0 * (double)x.pixels() * (cin + cout);
    const TView xv = x, yv = y, ltv = lt_;
    const bool has_lt = has_lt_;
    r.run = [p, xv, yv, ltv, has_lt, lt_col](const Plan& pl, const RunCtx& cx) {
        Lcv3BlockParams q = p;
        q.x = pl.vptr(xv, cx);
        q.y = pl.vptr(yv, cx);
        if (has_lt) {
            q.line_w = reinterpret_cast<const int32_t*>(pl.vptr(ltv, cx)) + lt_col;
            q.line_stride = kLineTabStride;
        }
        launch_lcv3_block(q, cx.stream);
    };
    emit(std::move(r));
    *y_out = y;
    return true;
}

Builder::GapOut Builder::lcv3_gap(const TView& x, int lt_col) {
    RD_CHECK(lcv3_gap_shape_ok(x.c), "lcv3 gap: channels % 4, at most 4096");
    GapOut g;
    g.chunks = x.h;
    g.partial = alloc_raw((size_t)x.n * x.h * x.c);
    if (!planning()) return g;
    OpRecord r;
    r.name = "lcv3_gap";
    r.kind = "gap";
    r.cfg = has_lt_ ? "rows/lines" : "rows";
    r.bytes = 4.0 * x.pixels() * x.c;
    const TView xv = x, pv = g.partial, ltv = lt_;
    const bool has_lt = has_lt_;
    r.run = [xv, pv, ltv, has_lt, lt_col](const Plan& pl, const RunCtx& cx) {
        launch_lcv3_gap_rows(pl.vptr(xv, cx), pl.ld(xv), xv.n, xv.h, xv.w, xv.c, pl.vptr(pv, cx),
                             has_lt ? reinterpret_cast<const int32_t*>(pl.vptr(ltv, cx)) + lt_col : nullptr, kLineTabStride, cx.stream);
    };
    emit(std::move(r));
    return g;
}

TView Builder::lcv3_pool(const TView& x, Affine post, const TView* out) {
    RD_CHECK(x.h == 3 && x.w >= 2 && x.c % 4 == 0, "lcv3 pool: a 3-row map");
    const int ow = (x.w - 2) / 2 + 1;
    TView y = out ? *out : alloc(x.n, 1, ow, x.c);
    RD_CHECK(y.n == x.n && y.h == 1 && y.w == ow && y.c == x.c, "lcv3 pool: output view mismatch");
    if (!planning()) return y;
    OpRecord r;
    r.name = "hswish+avgpool3x2+affine";
    r.kind = "pool";
    r.bytes = 4.0 * (x.pixels() * x.c + y.pixels() * y.c);
    const TView xv = x, yv = y, ltv = lt_;
    const bool has_lt = has_lt_;
    r.run = [xv, yv, ltv, has_lt, post](const Plan& pl, const RunCtx& c) {
        launch_lcv3_pool(pl.vptr(xv, c), pl.ld(xv), pl.vptr(yv, c), pl.ld(yv), xv.n, xv.h, xv.w, xv.c, post.s, post.b, c.stream,
                         has_lt ? reinterpret_cast<const int32_t*>(pl.vptr(ltv, c)) : nullptr);
    };
    emit(std::move(r));
    return y;
}

}  // namespace rd
