// Helpers shared by builder.cpp and builder_mobile.cpp only (everything here is file-local to the including source).
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
