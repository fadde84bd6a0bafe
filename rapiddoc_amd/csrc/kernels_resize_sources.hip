// rd_preproc_resize_norm_sources (include/rapiddoc_mi355.h): cv2.resize on uint8 + normalise -> CHW fp32, the work of
// resize_u8_norm_kernel (kernels_image.hip), for n source images of ANY sizes, each to its own output size, in ONE launch: the pages
// of a batch whose sizes differ (A4 next to Letter, a landscape sheet in a portrait report), the tables of a page.  Every source
// carries a descriptor - device address, row pitch, sizes, where its [3][OH][OW] planes go - as the lines of rd_line_warp_sources do.
// The arithmetic is resize_u8_norm_kernel's, expression for expression (a copy on purpose, in a file of its own: the two kernels share
// no body and no translation unit, so this one cannot move the other's generated code): 11-bit coefficients rounded half-to-even from
// float32, int32 rows, the two vertical rounding rules, the source position from 1.0 / ((double)OW / (double)W).  Only the addressing
// differs: rows are `pitch` bytes apart (a source may be a window of a larger image) and start at any byte address - every load is a
// single byte.  tests/test_gpu_mixed_pages.py demands bit-equality with rd_preproc_resize_norm on a contiguous copy of each source.
// OpenCV's scalar code rounds every float operation separately: no FMA contraction in this file.
#pragma clang fp contract(off)
#include <cmath>
#include <string>

#include "rd_device.h"
#include "resize_sources_check.h"

namespace rd {

static_assert(sizeof(rd_resize_source_desc) == 48, "rd_resize_source_desc layout");

struct ResizeSourcesParams {
    const rd_resize_source_desc* descs;   // device copy
    float* out;
    float mean[3], inv_std[3], scale;
    int interp, swap_rb;
};

__device__ __forceinline__ void rs_cubic_coeffs(float x, float* c) {   // interpolateCubic, A = -0.75, float32
    const float A = -0.75f;
    c[0] = ((A * (x + 1.f) - 5.f * A) * (x + 1.f) + 8.f * A) * (x + 1.f) - 4.f * A;
    c[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
    c[2] = ((A + 2.f) * (1.f - x) - (A + 3.f)) * (1.f - x) * (1.f - x) + 1.f;
    c[3] = 1.f - c[0] - c[1] - c[2];
}
// saturate_cast<short>(v): round half to even, clamp
__device__ __forceinline__ int rs_round_short(float v) {
    const int r = __float2int_rn(v);
    return min(max(r, -32768), 32767);
}
// source position of destination index d: fx = (float)((d + 0.5) * scale - 0.5) with scale = 1 / (dst / src) in double
__device__ __forceinline__ void rs_src_pos(int d, double scale, int& s, float& f) {
    const float fx = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(fx);
    f = fx - (float)s;
}

// grid = (blocks along the largest output, sources): blockIdx.y names the source, its descriptor is wave-uniform (scalar loads); the
// blocks of a row of the grid stride over the output's pixels, blocks past a smaller output's end leave at once.  Stores are plain
// float stores, one plane after the other.
__global__ void __launch_bounds__(256) resize_u8_norm_sources_kernel(ResizeSourcesParams p) {
    const rd_resize_source_desc d = p.descs[blockIdx.y];
    const long total = (long)d.OH * d.OW;
    const uint8_t* src = d.src;
    const size_t pitch = (size_t)d.pitch;
    float* dst = p.out + d.out_off;
    const double scale_x = 1.0 / ((double)d.OW / (double)d.W), scale_y = 1.0 / ((double)d.OH / (double)d.H);
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int ox = (int)(idx % d.OW), oy = (int)(idx / d.OW);
        int sx, sy;
        float fx, fy;
        rs_src_pos(ox, scale_x, sx, fx);
        rs_src_pos(oy, scale_y, sy, fy);
        int out[3];
        if (p.interp == 2) {
            float cx[4], cy[4];
            rs_cubic_coeffs(fx, cx);
            rs_cubic_coeffs(fy, cy);
            int ax[4], ay[4], xi[4], yi[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ax[k] = rs_round_short(cx[k] * 2048.f);
                ay[k] = rs_round_short(cy[k] * 2048.f);
                xi[k] = min(max(sx - 1 + k, 0), d.W - 1);
                yi[k] = min(max(sy - 1 + k, 0), d.H - 1);
            }
            long acc[3] = {0, 0, 0};
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const uint8_t* row = src + (size_t)yi[a] * pitch;
                int h[3] = {0, 0, 0};
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uint8_t* px = row + (size_t)xi[b] * 3;
                    h[0] += (int)px[0] * ax[b];
                    h[1] += (int)px[1] * ax[b];
                    h[2] += (int)px[2] * ax[b];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += (long)h[c] * ay[a];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] = (int)min(max((acc[c] + (1L << 21)) >> 22, 0L), 255L);
        } else {
            if (sx < 0) { fx = 0.f; sx = 0; }
            if (sx >= d.W - 1) { fx = 0.f; sx = d.W - 1; }
            if (sy < 0) { fy = 0.f; sy = 0; }
            if (sy >= d.H - 1) { fy = 0.f; sy = d.H - 1; }
            const int x1 = min(sx + 1, d.W - 1), y1 = min(sy + 1, d.H - 1);
            const int a0 = rs_round_short((1.f - fx) * 2048.f), a1 = rs_round_short(fx * 2048.f);
            const int b0 = rs_round_short((1.f - fy) * 2048.f), b1 = rs_round_short(fy * 2048.f);
            const uint8_t* r0 = src + (size_t)sy * pitch;
            const uint8_t* r1 = src + (size_t)y1 * pitch;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int s0 = (int)r0[sx * 3 + c] * a0 + (int)r0[x1 * 3 + c] * a1;
                const int s1 = (int)r1[sx * 3 + c] * a0 + (int)r1[x1 * 3 + c] * a1;
                out[c] = min(max((((b0 * (s0 >> 4)) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2, 0), 255);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int sc = p.swap_rb ? 2 - c : c;
            dst[(size_t)c * total + idx] = ((float)out[sc] * p.scale - p.mean[c]) * p.inv_std[c];
        }
    }
}

int launch_preproc_resize_norm_sources(int device, const rd_resize_source_desc* host, const rd_resize_source_desc* dev, int n, const float mean[3],
                                       const float std[3], float scale, int interp, int swap_rb, float* out, int64_t out_floats, hipStream_t s,
                                       std::string& err) {
    const std::string who = "rd_preproc_resize_norm_sources: ";
    int64_t max_pixels = 0;
    if (check_resize_sources(host, dev, n, interp, out, out_floats, max_pixels, err) != 0) return 1;
    hipError_t rc = hipSetDevice(device);
    if (rc != hipSuccess) { err = who + "hipSetDevice: " + hipGetErrorString(rc); return 1; }
    ResizeSourcesParams p{};
    p.descs = dev; p.out = out;
    for (int i = 0; i < 3; ++i) { p.mean[i] = mean ? mean[i] : 0.f; p.inv_std[i] = 1.f / (std ? std[i] : 1.f); }
    p.scale = scale; p.interp = interp; p.swap_rb = swap_rb;
    const long blocks = ((long)max_pixels + 255) / 256;
    hipLaunchKernelGGL(resize_u8_norm_sources_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks), n), dim3(256), 0, s, p);
    rc = hipGetLastError();
    if (rc != hipSuccess) { err = who + "kernel launch: " + hipGetErrorString(rc); return 1; }
    return 0;
}

}  // namespace rd
