// Helpers shared by builder.cpp, builder_mobile.cpp and the developer entries of api_debug.cpp (everything here is file-local to the
// including source).
#pragma once
#include <cmath>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "engine.h"

namespace rd {

// weights beyond the fp16 range cannot be split: such a layer stays on the fp32 MFMA kernel in every precision mode
static inline bool fits_fp16_range(const std::vector<float>& w) {
    for (float v : w)
        if (!(std::fabs(v) < 65504.f)) return false;
    return true;
}
static inline int out_dim(int in, int k, int s, int p0, int p1) { return (in + p0 + p1 - k) / s + 1; }

// depthwise weight [C][1][taps] -> the kernels' tap-major image [taps][C], each channel times scale[ch] when given (a folded BatchNorm)
static inline std::vector<float> fold_dw_taps(const float* w, int c, int taps, const float* scale = nullptr) {
    std::vector<float> wf((size_t)taps * c);
    for (int ch = 0; ch < c; ++ch)
        for (int t = 0; t < taps; ++t) wf[(size_t)t * c + ch] = w[(size_t)ch * taps + t] * (scale ? scale[ch] : 1.f);
    return wf;
}

// the geometry of a depthwise convolution as launch_dwconv, dw_route and the planner's dwconv_gap_chunks read it (pointers, leading
// dimensions, epilogue and line tables stay with the caller): Builder::dwconv and the developer entries fill DwParams here only
static inline DwParams dw_geometry(int n, int h, int w, int c, int kh, int kw, int sh, int sw, int pt, int pl, int pb, int pr) {
    DwParams p{};
    p.N = n; p.H = h; p.W = w; p.C = c;
    p.OH = out_dim(h, kh, sh, pt, pb); p.OW = out_dim(w, kw, sw, pl, pr);
    p.KH = kh; p.KW = kw; p.SH = sh; p.SW = sw; p.PT = pt; p.PL = pl;
    return p;
}

// The DB head's two ConvTranspose2d(.., 2, stride 2) weights in their checkpoint layouts - w1 [cin][cmid][2][2], b1 [cmid] or null,
// w2 [cmid][1][2][2] - as det_head_tail_kernel reads them: tap = 2 dy + dx major, wa [4][cmid][cin] and ba [cmid] with the middle
// channel's affine (a folded BatchNorm: scale, shift per channel) applied, wb [4][cmid]
static inline void pack_det_head_tail(const float* w1, const float* b1, const float* w2, int cin, int cmid, const float* scale, const float* shift,
                                      std::vector<float>& wa, std::vector<float>& ba, std::vector<float>& wb) {
    wa.assign((size_t)4 * cmid * cin, 0.f);
    ba.assign(cmid, 0.f);
    wb.assign((size_t)4 * cmid, 0.f);
    for (int tap = 0; tap < 4; ++tap) {
        const int dy = tap >> 1, dx = tap & 1;
        for (int co = 0; co < cmid; ++co) {
            for (int ci = 0; ci < cin; ++ci) wa[((size_t)tap * cmid + co) * cin + ci] = w1[(((size_t)ci * cmid + co) * 2 + dy) * 2 + dx] * scale[co];
            wb[(size_t)tap * cmid + co] = w2[((size_t)co * 2 + dy) * 2 + dx];
        }
    }
    if (b1)
        for (int co = 0; co < cmid; ++co) ba[co] = b1[co] * scale[co];
    for (int co = 0; co < cmid; ++co) ba[co] += shift[co];
}

// A ConvTranspose2d(.., 2, stride 2) weight in its checkpoint layout - w [cin][cout][2][2], b [cout] or null - as the OUT_DECONV2X2
// epilogue of the implicit-GEMM kernels reads it: wf [4 cout][cin], row = tap * cout + co with tap = 2 dy + dx, and bias [cout], both with
// the output channel's affine (a folded BatchNorm: scale, shift per channel) applied
static inline void pack_deconv2x2(const float* w, const float* b, int cin, int cout, const float* scale, const float* shift, std::vector<float>& wf,
                                  std::vector<float>& bias) {
    wf.assign((size_t)4 * cout * cin, 0.f);
    bias.assign(cout, 0.f);
    for (int ci = 0; ci < cin; ++ci)
        for (int co = 0; co < cout; ++co)
            for (int dy = 0; dy < 2; ++dy)
                for (int dx = 0; dx < 2; ++dx)
                    wf[((size_t)(dy * 2 + dx) * cout + co) * cin + ci] = w[(((size_t)ci * cout + co) * 2 + dy) * 2 + dx] * scale[co];
    if (b)
        for (int co = 0; co < cout; ++co) bias[co] = b[co] * scale[co];
    for (int co = 0; co < cout; ++co) bias[co] += shift[co];
}

// OpRecord::shape of a layer over the map x: "N<n>_<h>x<w>", then "_C<c>" per channel count given
static inline std::string shape_str(const TView& x, std::initializer_list<int> channels = {}) {
    std::string s = "N" + std::to_string(x.n) + "_" + std::to_string(x.h) + "x" + std::to_string(x.w);
    const char* sep = "_C";
    for (int c : channels) {
        s += sep + std::to_string(c);
        sep = "_";
    }
    return s;
}

// A/B switch of a route, read per plan: the variable's first character '0' / '1' forces the route off / on for every layer the kernel
// serves; unset or anything else leaves the per-layer default
static inline bool route_switch(const char* env, bool dflt) {
    return rd_env_on(env) || (dflt && !rd_env_off(env));
}

// OpRecord::run of a one-input one-output kernel: the plan-time parameters with x / y taken from the plan's buffers at run time
template <typename P, typename R>
static inline std::function<void(const Plan&, const RunCtx&)> run_xy(const P& p, const TView& x, const TView& y, R (*launch)(const P&, hipStream_t)) {
    return [p, x, y, launch](const Plan& pl, const RunCtx& cx) {
        P q = p;
        q.x = pl.vptr(x, cx);
        q.y = pl.vptr(y, cx);
        (void)launch(q, cx.stream);
    };
}

}  // namespace rd
