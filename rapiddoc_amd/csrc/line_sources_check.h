// Argument checks of rd_line_warp_sources (include/rapiddoc_mi355.h) as host-only code without a HIP call: the launcher in
// kernels_image.hip runs them on the HOST copy of the descriptors before anything is launched, and a plain C++ program can include
// this header alone.  Returns 0, or 1 with the message in `err`; on success `max_pixels` is the largest crop_w * crop_h of the launch.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/rapiddoc_mi355.h"

namespace rd {

constexpr int kLineSourcesMax = 65535;     // lines of one launch: gridDim.y

inline int check_line_sources(const rd_line_source_desc* host, const void* dev, int n, const void* scratch, int64_t scratch_bytes,
                              int64_t& max_pixels, std::string& err) {
    const std::string who = "rd_line_warp_sources: ";
    max_pixels = 0;
    if (!host || !dev) { err = who + "descriptors are NULL"; return 1; }
    if (!scratch || scratch_bytes < 0) { err = who + "scratch is NULL or scratch_bytes negative"; return 1; }
    if (n < 1 || n > kLineSourcesMax) { err = who + "n outside 1 .. " + std::to_string(kLineSourcesMax); return 1; }
    for (int k = 0; k < n; ++k) {
        const rd_line_source_desc& d = host[k];
        const std::string line = who + "line " + std::to_string(k) + ": ";
        if (!d.src) { err = line + "src is NULL"; return 1; }
        if (d.W < 1 || d.H < 1) { err = line + "source size " + std::to_string(d.H) + " x " + std::to_string(d.W) + " is not positive"; return 1; }
        if (d.pitch < 3 * (int64_t)d.W) { err = line + "pitch " + std::to_string(d.pitch) + " is below 3 * W"; return 1; }
        if (d.crop_w < 1 || d.crop_h < 1) {
            err = line + "crop size " + std::to_string(d.crop_h) + " x " + std::to_string(d.crop_w) + " is not positive";
            return 1;
        }
        const int64_t px = (int64_t)d.crop_w * d.crop_h;
        if (d.scratch_off < 0 || d.scratch_off > scratch_bytes || px > (scratch_bytes - d.scratch_off) / 3) {      // (no product that can overflow)
            err = line + "crop of " + std::to_string(px) + " pixels at offset " + std::to_string(d.scratch_off) + " overruns scratch_bytes = " +
                  std::to_string(scratch_bytes);
            return 1;
        }
        if (px > max_pixels) max_pixels = px;
    }
    return 0;
}

}  // namespace rd
