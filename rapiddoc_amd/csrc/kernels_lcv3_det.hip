// PPLCNetV3 in its DETECTOR geometry (PP-OCRv5 mobile detector, build_ppocrv5_det_mobile): the LDS-staged 2-D depthwise layer and the
// elementwise activation of the four stage outputs.
//
// lcv3_dw2d_kernel<K, S> computes the same layer as lcv3_dw_kernel (kernels_lcv3.hip):
//   y = post_act ? post_s * hardswish(dw_kxk(x') + bias) + post_b : dw_kxk(x') + bias,   x' = pre_act ? pre_s * hardswish(x) + pre_b : x
// with zero padding around x' (activation and affine touch the elements INSIDE the map only).  The direct kernel loads every input
// element K (K + 3) / 4 times from global memory and activates it each time, and at the detector's big maps (C = 16 / 32 / 48 at 1/2 and
// 1/4 of the page) its 16-byte loads are C * 4-byte segments 4 * C * 4 bytes apart.  Here a workgroup owns TH x TW output pixels x 16
// channels, stages the (TH - 1) S + K by (TW - 1) S + K input patch once - consecutive lanes walk a patch row: 64 contiguous bytes per
// pixel, the whole row segment contiguous where C = 16 - activates each staged element once, and computes from LDS.
//
// Thread t: channel quad t & 3, output column (t >> 2) & 31, row group t >> 7; it owns TR vertically adjacent outputs, so that the
// (TR - 1) S + K patch elements of one kernel column are read once for all of them.  A wavefront's 16-byte LDS reads are then S * 64 bytes
// apart: conflict-free at stride 1, two-way at stride 2.  The sum runs over kw (outer) and kh (inner) from the bias: its order does not
// depend on the position of the pixel, the tile or the image, so a page's result does not depend on the batch it rides in.
//
//   <K, S>    tile (rows x cols x ch)   patch     LDS bytes   VGPRs   workgroups / CU (a workgroup = one wavefront per SIMD; LDS 160 KB)
//   <3, 1>    8 x 32 x 16               10 x 34   21760       60      7   (LDS-bound)
//   <5, 1>    8 x 32 x 16               12 x 36   27648       76      5   (LDS-bound)
//   <3, 2>    4 x 32 x 16                9 x 65   37440       48      4   (LDS-bound)
//   <5, 2>    4 x 32 x 16               11 x 67   47168       64      3   (LDS-bound)
// No spills (tests/test_isa_resources.py::test_no_hot_kernel_spills).  The kw loop is NOT unrolled on purpose: unrolled, the compiler
// keeps all K * K weight quads and every patch column live, 256 VGPRs and one wavefront per SIMD at K = 5.
// Ragged tiles, maps smaller than a tile or than the halo, odd H / W under stride 2: every global load is guarded by the map's bounds and
// every store by (OH, OW); a workgroup exists only for tiles that hold at least one output.
#include "rd_device.h"

namespace rd {

constexpr int DW2D_CS = 16, DW2D_TW = 32;

template <int K, int S>
__global__ void __launch_bounds__(256) lcv3_dw2d_kernel(Lcv3DwParams p, int tiles_h, int tiles_w, int nslices) {
    constexpr int P = K / 2, TR = S == 1 ? 4 : 2, TH = 2 * TR, TW = DW2D_TW;
    constexpr int PH = (TH - 1) * S + K, PW = (TW - 1) * S + K, NV = (TR - 1) * S + K;
    __shared__ f32x4 patch[PH * PW * 4];
    int bid = blockIdx.x;
    const int c0 = (bid % nslices) * DW2D_CS;
    bid /= nslices;
    const int ow0 = (bid % tiles_w) * TW;
    bid /= tiles_w;
    const int oh0 = (bid % tiles_h) * TH;
    const int n = bid / tiles_h;
    const int t = threadIdx.x;
    const int ih0 = oh0 * S - P, iw0 = ow0 * S - P;
    const float* xn = p.x + (size_t)n * p.H * p.W * p.xld + c0;
#pragma unroll 4
    for (int i = t; i < PH * PW * 4; i += 256) {
        const int pix = i >> 2;
        const int ih = ih0 + pix / PW, iw = iw0 + pix % PW;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ih >= 0 && ih < p.H && iw >= 0 && iw < p.W) {
            v = *reinterpret_cast<const f32x4*>(xn + ((size_t)ih * p.W + iw) * p.xld + ((i & 3) << 2));
            if (p.pre_act) v = lcv3_hswish_aff(v, p.pre_s, p.pre_b);
        }
        patch[i] = v;
    }
    __syncthreads();
    const int q = t & 3, col = (t >> 2) & (TW - 1), rg = t >> 7;
    const int c = c0 + (q << 2);
    const f32x4 bias = *reinterpret_cast<const f32x4*>(p.bias + c);
    f32x4 acc[TR];
#pragma unroll
    for (int j = 0; j < TR; ++j) acc[j] = bias;
    const f32x4* base = patch + ((rg * TR * S) * PW + col * S) * 4 + q;
#pragma unroll 1
    for (int kw = 0; kw < K; ++kw) {
        f32x4 in[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) in[i] = base[(i * PW + kw) * 4];
#pragma unroll
        for (int kh = 0; kh < K; ++kh) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(p.w + (size_t)(kh * K + kw) * p.C + c);
#pragma unroll
            for (int j = 0; j < TR; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(in[j * S + kh][e], wv[e], acc[j][e]);
        }
    }
    const int ow = ow0 + col;
    if (ow >= p.OW) return;
#pragma unroll
    for (int j = 0; j < TR; ++j) {
        const int oh = oh0 + rg * TR + j;
        if (oh >= p.OH) break;
        const f32x4 o = p.post_act ? lcv3_hswish_aff(acc[j], p.post_s, p.post_b) : acc[j];
        *reinterpret_cast<f32x4*>(p.y + (((size_t)n * p.OH + oh) * p.OW + ow) * p.yld + c) = o;
    }
}

bool lcv3_dw2d_shape_ok(int k, int sh, int sw, int c) { return (k == 3 || k == 5) && sh == sw && (sh == 1 || sh == 2) && c >= DW2D_CS && c % DW2D_CS == 0; }

static long lcv3_dw2d_grid(const Lcv3DwParams& p, int* tiles_h, int* tiles_w, int* nslices) {
    const int th = p.SH == 1 ? 8 : 4;
    *tiles_h = (p.OH + th - 1) / th;
    *tiles_w = (p.OW + DW2D_TW - 1) / DW2D_TW;
    *nslices = p.C / DW2D_CS;
    return (long)p.N * *tiles_h * *tiles_w * *nslices;
}

bool lcv3_dw2d_launch_ok(const Lcv3DwParams& p) {
    if (!lcv3_dw2d_shape_ok(p.K, p.SH, p.SW, p.C) || p.line_in || p.line_out || p.N < 1 || p.OH < 1 || p.OW < 1) return false;
    int a, b, c;
    return lcv3_dw2d_grid(p, &a, &b, &c) <= 0x7fffffffL;
}

bool launch_lcv3_dw2d(const Lcv3DwParams& p, hipStream_t s) {
    if (!lcv3_dw2d_launch_ok(p)) return false;
    int tiles_h, tiles_w, nslices;
    const long total = lcv3_dw2d_grid(p, &tiles_h, &tiles_w, &nslices);
    const dim3 g((unsigned)total), b(256);
    if (p.K == 3 && p.SH == 1) hipLaunchKernelGGL((lcv3_dw2d_kernel<3, 1>), g, b, 0, s, p, tiles_h, tiles_w, nslices);
    else if (p.K == 5 && p.SH == 1) hipLaunchKernelGGL((lcv3_dw2d_kernel<5, 1>), g, b, 0, s, p, tiles_h, tiles_w, nslices);
    else if (p.K == 3 && p.SH == 2) hipLaunchKernelGGL((lcv3_dw2d_kernel<3, 2>), g, b, 0, s, p, tiles_h, tiles_w, nslices);
    else hipLaunchKernelGGL((lcv3_dw2d_kernel<5, 2>), g, b, 0, s, p, tiles_h, tiles_w, nslices);
    return true;
}

// y = s hardswish(x) + b: a pointwise layer of this backbone writes convolution + bias and leaves its activation to its consumer; the
// four stage outputs feed the neck's matrix kernels, which cannot activate on load, so their activated form is written once, here
__global__ void __launch_bounds__(256) lcv3_act_kernel(const float* x, int xld, float* y, int yld, long pixels, int C, float s, float b) {
    const int c4n = C >> 2;
    const long total = pixels * c4n;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int c = (int)(idx % c4n) << 2;
        const long pix = idx / c4n;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)pix * xld + c);
        *reinterpret_cast<f32x4*>(y + (size_t)pix * yld + c) = lcv3_hswish_aff(v, s, b);
    }
}
void launch_lcv3_act(const float* x, int xld, float* y, int yld, long pixels, int C, float s, float b, hipStream_t st) {
    const long blocks = (pixels * (C >> 2) + 255) / 256;
    hipLaunchKernelGGL(lcv3_act_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks > 65536 ? 65536 : blocks)), dim3(256), 0, st, x, xld, y, yld, pixels, C,
                       s, b);
}

}  // namespace rd
