// Argument checks of rd_preproc_resize_norm_sources (include/rapiddoc_mi355.h) as host-only code without a HIP call: the launcher in
// kernels_resize_sources.hip runs them on the HOST copy of the descriptors before anything is launched, and a plain C++ program can
// include this header alone.  Returns 0, or 1 with the message in `err`; on success `max_pixels` is the largest OW * OH of the launch.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rapiddoc_mi355.h"

namespace rd {

constexpr int kResizeSourcesMax = 65535;      // sources of one launch: gridDim.y
constexpr int kResizeSourcesMaxSide = 32768;  // W, H, OW, OH: a plane stays below 2^31 pixels, 3 planes far below 2^63 floats

inline int check_resize_sources(const rd_resize_source_desc* host, const void* dev, int n, int interp, const void* out, int64_t out_floats,
                                int64_t& max_pixels, std::string& err) {
    const std::string who = "rd_preproc_resize_norm_sources: ";
    max_pixels = 0;
    if (!host || !dev) { err = who + "descriptors are NULL"; return 1; }
    if (!out || out_floats < 0) { err = who + "out_dev is NULL or out_floats negative"; return 1; }
    if (n < 1 || n > kResizeSourcesMax) { err = who + "n outside 1 .. " + std::to_string(kResizeSourcesMax); return 1; }
    if (interp != 1 && interp != 2) { err = who + "interp " + std::to_string(interp) + " is neither 1 (linear) nor 2 (cubic)"; return 1; }
    auto side_ok = [](int32_t v) { return v >= 1 && v <= kResizeSourcesMaxSide; };
    std::vector<std::pair<int64_t, int64_t>> slots((size_t)n);      // (first float, floats)
    for (int k = 0; k < n; ++k) {
        const rd_resize_source_desc& d = host[k];
        const std::string src = who + "source " + std::to_string(k) + ": ";
        if (!d.src) { err = src + "src is NULL"; return 1; }
        if (!side_ok(d.W) || !side_ok(d.H)) {
            err = src + "source size " + std::to_string(d.H) + " x " + std::to_string(d.W) + " outside 1 .. " + std::to_string(kResizeSourcesMaxSide);
            return 1;
        }
        if (!side_ok(d.OW) || !side_ok(d.OH)) {
            err = src + "output size " + std::to_string(d.OH) + " x " + std::to_string(d.OW) + " outside 1 .. " + std::to_string(kResizeSourcesMaxSide);
            return 1;
        }
        if (d.pitch < 3 * (int64_t)d.W) { err = src + "pitch " + std::to_string(d.pitch) + " is below 3 * W"; return 1; }
        const int64_t px = (int64_t)d.OW * d.OH, floats = 3 * px;                                    // <= 3 * 2^30
        if (d.out_off < 0) { err = src + "out_off " + std::to_string(d.out_off) + " is negative"; return 1; }
        if (d.out_off > out_floats || floats > out_floats - d.out_off) {                             // (no sum that can overflow)
            err = src + "slot of " + std::to_string(floats) + " floats at offset " + std::to_string(d.out_off) + " overruns out_floats = " +
                  std::to_string(out_floats);
            return 1;
        }
        slots[(size_t)k] = {d.out_off, floats};
        if (px > max_pixels) max_pixels = px;
    }
    std::sort(slots.begin(), slots.end());
    for (int k = 1; k < n; ++k)
        if (slots[(size_t)k].first - slots[(size_t)k - 1].first < slots[(size_t)k - 1].second) {     // both inside out_floats: no overflow
            err = who + "the slots at offsets " + std::to_string(slots[(size_t)k - 1].first) + " and " + std::to_string(slots[(size_t)k].first) +
                  " overlap";
            return 1;
        }
    return 0;
}

}  // namespace rd
