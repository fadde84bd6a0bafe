// Canvases from uploaded host crops (include/rapiddoc_mi355.h rd_stage_canvases): what analyze.RegionTextModel composes for the detector -
// a white [gh][gw][3] canvas per crop, the crop at (0, 0), BGR turned into RGB - for ALL size groups of a call in one launch.  No weights;
// a byte copy, written for the memory system:
//   stores   a lane owns 4 pixels = 12 bytes of one canvas row (gw % 4 == 0 and a 4-byte aligned canvas make that three aligned dwords);
//            consecutive lanes own consecutive groups, so a wavefront's store instruction covers 768 contiguous bytes, and every canvas byte
//            is written exactly once - white and crop in the same pass;
//   loads    a group that lies wholly inside the crop's row reads its 12 bytes with one unaligned 12-byte copy (crop rows start at any byte
//            address; the compiler is free to use dword loads, which gfx950 serves at any alignment) - lanes read consecutive 12-byte pieces
//            of a row; the one group per row that straddles the crop's right edge reads its 3, 6 or 9 bytes one by one, so no byte past
//            3 * w of a row is ever touched; groups outside the crop load nothing;
//   swap     bytes 0 and 2 of every pixel are exchanged in registers, between load and store.
// grid = (blocks along the largest canvas, crops): blockIdx.y names the crop (its descriptor is wave-uniform: scalar loads), the blocks of
// a row of the grid stride over the canvas's groups; blocks past a smaller canvas's end leave at once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "rd_kernels.h"

namespace {

static_assert(sizeof(rd_stage_desc) == 48, "rd_stage_desc layout");

constexpr int kThreads = 256, kMaxGridX = 1024, kMaxSide = 16384, kMaxCrops = 65535;

struct alignas(4) Group { uint32_t d[3]; };                          // 4 pixels of a canvas row
struct __attribute__((packed)) LooseGroup { uint8_t b[12]; };       // 4 pixels of a crop row: any byte address
// the descriptors' addresses are device memory: saying so keeps the accesses global_* (a pointer read from memory is a flat one otherwise)
#define RD_GLOBAL __attribute__((address_space(1)))

__global__ __launch_bounds__(kThreads) void stage_canvases_kernel(const rd_stage_desc* __restrict__ descs) {
#if defined(__HIP_DEVICE_COMPILE__)                                  // (address-space struct copies have no host form)
    const rd_stage_desc d = descs[blockIdx.y];
    const int per_row = d.gw >> 2, groups = d.gh * per_row;          // gh * gw / 4 <= 2^26
    const bool swap = (d.flags & RD_STAGE_SWAP_RB) != 0;
    for (int g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += gridDim.x * kThreads) {
        const int y = g / per_row, x = (g - y * per_row) << 2;
        uint8_t b[12];
#pragma unroll
        for (int t = 0; t < 12; ++t) b[t] = 255;
        if (y < d.h && x < d.w) {
            const RD_GLOBAL uint8_t* s = (const RD_GLOBAL uint8_t*)d.src + ((size_t)y * (size_t)d.pitch + (size_t)x * 3);
            if (x + 4 <= d.w) {
                const LooseGroup in = *reinterpret_cast<const RD_GLOBAL LooseGroup*>(s);
#pragma unroll
                for (int t = 0; t < 12; ++t) b[t] = in.b[t];
            } else {                                                     // the group on the crop's right edge: 1 .. 3 pixels of it
                const int nb = (d.w - x) * 3;
#pragma unroll
                for (int t = 0; t < 9; ++t)
                    if (t < nb) b[t] = s[t];
            }
            if (swap) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {                            // (white stays white)
                    const uint8_t r = b[3 * p];
                    b[3 * p] = b[3 * p + 2];
                    b[3 * p + 2] = r;
                }
            }
        }
        Group out;
        __builtin_memcpy(&out, b, 12);
        *reinterpret_cast<RD_GLOBAL Group*>((RD_GLOBAL uint8_t*)d.canvas + ((size_t)y * (size_t)d.gw + (size_t)x) * 3) = out;
    }
#endif
}

}  // namespace

namespace rd {

int launch_stage_canvases(int device, const rd_stage_desc* host, const rd_stage_desc* dev, int n, hipStream_t s, std::string& err) {
    const std::string who = "rd_stage_canvases: ";
    if (!host || !dev) { err = who + "descriptors are NULL"; return 1; }
    if (n < 1 || n > kMaxCrops) { err = who + "n outside 1 .. " + std::to_string(kMaxCrops); return 1; }
    int max_groups = 0;
    for (int k = 0; k < n; ++k) {
        const rd_stage_desc& d = host[k];
        const std::string crop = who + "crop " + std::to_string(k) + ": ";
        if (d.gh < 1 || d.gw < 1 || d.gh > kMaxSide || d.gw > kMaxSide) { err = crop + "gh, gw outside 1 .. " + std::to_string(kMaxSide); return 1; }
        if (d.gw % 4 != 0) { err = crop + "gw = " + std::to_string(d.gw) + " is no multiple of 4"; return 1; }
        if (!d.canvas || reinterpret_cast<uintptr_t>(d.canvas) % 4 != 0) { err = crop + "canvas is NULL or not 4-byte aligned"; return 1; }
        if (d.w < 0 || d.h < 0) { err = crop + "negative size"; return 1; }
        if (d.w > d.gw || d.h > d.gh) {
            err = crop + std::to_string(d.h) + " x " + std::to_string(d.w) + " does not fit its " + std::to_string(d.gh) + " x " + std::to_string(d.gw) + " canvas";
            return 1;
        }
        if (d.w > 0 && d.h > 0 && (!d.src || (d.h > 1 && d.pitch < 3 * (int64_t)d.w))) { err = crop + "src is NULL or its pitch is below 3 * w"; return 1; }
        max_groups = std::max(max_groups, d.gh * (d.gw / 4));
    }
    hipError_t rc = hipSetDevice(device);
    if (rc != hipSuccess) { err = who + "hipSetDevice: " + hipGetErrorString(rc); return 1; }
    const int gx = std::min(kMaxGridX, (max_groups + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(stage_canvases_kernel, dim3((unsigned)gx, (unsigned)n), dim3(kThreads), 0, s, dev);
    rc = hipGetLastError();
    if (rc != hipSuccess) { err = who + "kernel launch: " + hipGetErrorString(rc); return 1; }
    return 0;
}

}  // namespace rd
