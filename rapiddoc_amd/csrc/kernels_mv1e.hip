// MobileNetV1Enhance (the multilingual PP-OCRv3 / v4 mobile recognisers, build_ppocr_rec_mv1e): the LDS-staged 5x5 depthwise layer of the
// recogniser geometry and the backbone's final pooling.
//
// dw5_strip_kernel<SH, SW> computes the same layer as lcv3_dw_kernel<5, SW, 4> (kernels_lcv3.hip):
//   y = post_act ? post_s * hardswish(dw_5x5(x') + bias) + post_b : dw_5x5(x') + bias,   x' = pre_act ? pre_s * hardswish(x) + pre_b : x
// with zero padding around x' (activation and affine touch the elements INSIDE the map only), under the recogniser's line table: input
// columns >= line_in[n] are padding too, output columns >= line_out[n] are written as zeros, and a tile wholly beyond a line's output
// width writes zeros and loads nothing.  Strides (1,1), (2,1) and (1,2).
//
// The direct kernel loads every input element 5 * (5 + 3) / 4 = 10 times from global memory and activates it each time.  A recogniser map
// is at most 6 rows high from the first 5x5 layer on, so here ONE workgroup owns one line x one strip of TW output columns x 16 channels x
// ALL rows: the H x ((TW - 1) SW + 5) input patch is staged once - through registers, because the activation is applied on the way;
// consecutive lanes walk a patch row, 64 contiguous bytes per pixel - each element is activated once, and all 25 taps read it from LDS.
// A strip re-reads only its 4-column halo.
//
// Thread t: channel quad t & 3, output column t >> 2; it owns every output row of its column (6 at SH = 1, 3 at SH = 2), so the <= 6 patch
// elements of one kernel column are read once for all of them.  A wavefront's 16-byte LDS reads are SW * 64 bytes apart: conflict-free at
// SW = 1, two-way at SW = 2.  The sum starts from the bias and runs over kw (outer) and kh (inner); taps above / below the map are left
// out by row index alone.  The order depends on the row and on H only - never on the column, the tile, the line's index or the batch - so
// a line's result does not depend on the launch it rides in, bit for bit.
//
//   <SH, SW>   tile (rows x cols x ch)   patch      LDS bytes   threads   VGPRs   workgroups / CU (LDS 160 KB; a workgroup = 1 wavefront per SIMD
//                                                                                at 256 threads, 1 per 2 SIMDs at 128)
//   <1, 1>     6 x 64 x 16               6 x 68     26112       256       74      6   (LDS-bound; 74 VGPRs allow 6 waves per SIMD)
//   <2, 1>     3 x 64 x 16               6 x 68     26112       256       62      6   (LDS-bound)
//   <1, 2>     6 x 32 x 16               6 x 67     25728       128       74      6   (LDS-bound)
// No scratch.  The kw loop is NOT unrolled on purpose (as in lcv3_dw2d_kernel): unrolled, all 25 weight quads and every patch column stay
// live.  Every global load is guarded by (H, the line's input width), every store by (OH, OW).
#include "rd_device.h"

namespace rd {

constexpr int DW5_CS = 16, DW5_MAXH = 6;
constexpr int dw5_tw(int sw) { return sw == 1 ? 64 : 32; }

template <int SH, int SW>
__global__ void __launch_bounds__(4 * dw5_tw(SW)) dw5_strip_kernel(Lcv3DwParams p, int tiles_w, int nslices) {
    constexpr int K = 5, P = 2, TW = dw5_tw(SW), NT = 4 * TW, PW = (TW - 1) * SW + K;
    constexpr int MAXOH = (DW5_MAXH + 2 * P - K) / SH + 1;
    __shared__ f32x4 patch[DW5_MAXH * PW * 4];
    int bid = blockIdx.x;
    const int c0 = (bid % nslices) * DW5_CS;
    bid /= nslices;
    const int ow0 = (bid % tiles_w) * TW;
    const int n = bid / tiles_w;
    const int t = threadIdx.x;
    const int q = t & 3, col = t >> 2;
    const int c = c0 + (q << 2);
    const int ow = ow0 + col;
    const int lw_in = p.line_in ? min(p.line_in[n * p.line_stride], p.W) : p.W;
    const int lw_out = p.line_out ? min(p.line_out[n * p.line_stride], p.OW) : p.OW;
    float* yn = p.y + (size_t)n * p.OH * p.OW * p.yld + c;
    if (ow0 >= lw_out) {          // (uniform over the workgroup) wholly beyond the line: zeros, nothing loaded
        if (ow < p.OW)
            for (int j = 0; j < p.OH; ++j) *reinterpret_cast<f32x4*>(yn + ((size_t)j * p.OW + ow) * p.yld) = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const int iw0 = ow0 * SW - P;
    const float* xn = p.x + (size_t)n * p.H * p.W * p.xld + c0;
    const int nstage = p.H * PW * 4;
#pragma unroll 4
    for (int i = t; i < nstage; i += NT) {
        const int pix = i >> 2;
        const int ih = pix / PW, iw = iw0 + pix % PW;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (iw >= 0 && iw < lw_in) {
            v = *reinterpret_cast<const f32x4*>(xn + ((size_t)ih * p.W + iw) * p.xld + ((i & 3) << 2));
            if (p.pre_act) v = lcv3_hswish_aff(v, p.pre_s, p.pre_b);
        }
        patch[i] = v;
    }
    __syncthreads();
    const f32x4 bias = *reinterpret_cast<const f32x4*>(p.bias + c);
    f32x4 acc[MAXOH];
#pragma unroll
    for (int j = 0; j < MAXOH; ++j) acc[j] = bias;
    const f32x4* base = patch + (col * SW) * 4 + q;
#pragma unroll 1
    for (int kw = 0; kw < K; ++kw) {
        f32x4 in[DW5_MAXH];
#pragma unroll
        for (int i = 0; i < DW5_MAXH; ++i) in[i] = i < p.H ? base[(i * PW + kw) * 4] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kh = 0; kh < K; ++kh) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(p.w + (size_t)(kh * K + kw) * p.C + c);
#pragma unroll
            for (int j = 0; j < MAXOH; ++j) {
                const int i = j * SH - P + kh;       // (compile-time after unrolling)
                if (i < 0 || i >= DW5_MAXH) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(in[i][e], wv[e], acc[j][e]);
            }
        }
    }
    if (ow >= p.OW) return;
    const bool dead = ow >= lw_out;
#pragma unroll
    for (int j = 0; j < MAXOH; ++j) {
        if (j >= p.OH) break;
        const f32x4 o = dead ? f32x4{0.f, 0.f, 0.f, 0.f} : p.post_act ? lcv3_hswish_aff(acc[j], p.post_s, p.post_b) : acc[j];
        *reinterpret_cast<f32x4*>(yn + ((size_t)j * p.OW + ow) * p.yld) = o;
    }
}

static long dw5_strip_grid(const Lcv3DwParams& p, int* tiles_w, int* nslices) {
    *tiles_w = (p.OW + dw5_tw(p.SW) - 1) / dw5_tw(p.SW);
    *nslices = p.C / DW5_CS;
    return (long)p.N * *tiles_w * *nslices;
}

bool dw5_strip_launch_ok(const Lcv3DwParams& p) {
    const bool stride_ok = (p.SH == 1 && p.SW == 1) || (p.SH == 2 && p.SW == 1) || (p.SH == 1 && p.SW == 2);
    if (p.K != 5 || !stride_ok || p.C < DW5_CS || p.C % DW5_CS != 0 || p.H < 1 || p.H > DW5_MAXH || p.N < 1 || p.W < 1) return false;
    if (p.OH != (p.H - 1) / p.SH + 1 || p.OW != (p.W - 1) / p.SW + 1 || p.xld % 4 != 0 || p.yld % 4 != 0 || p.xld < p.C || p.yld < p.C) return false;
    int a, b;
    return dw5_strip_grid(p, &a, &b) <= 0x7fffffffL;
}

bool launch_dw5_strip(const Lcv3DwParams& p, hipStream_t s) {
    if (!dw5_strip_launch_ok(p)) return false;
    int tiles_w, nslices;
    const dim3 g((unsigned)dw5_strip_grid(p, &tiles_w, &nslices));
    if (p.SH == 1 && p.SW == 1) hipLaunchKernelGGL((dw5_strip_kernel<1, 1>), g, dim3(4 * dw5_tw(1)), 0, s, p, tiles_w, nslices);
    else if (p.SH == 2) hipLaunchKernelGGL((dw5_strip_kernel<2, 1>), g, dim3(4 * dw5_tw(1)), 0, s, p, tiles_w, nslices);
    else hipLaunchKernelGGL((dw5_strip_kernel<1, 2>), g, dim3(4 * dw5_tw(2)), 0, s, p, tiles_w, nslices);
    return true;
}

// The backbone's end: the last pointwise layer's deferred hardswish on load, then AvgPool2d(2, 2) of the 3-row map - rows 0 and 1 only,
// row 2 is never read - giving one row of floor(W / 2) tokens.  line_tab as launch_avgpool3x2: line n writes its floor(w4 / 2) tokens at
// row line_tab[4 n + 3].
__global__ void __launch_bounds__(256) mv1e_pool_kernel(const float* x, int xld, float* y, int yld, int N, int H, int W, int C, int OW,
                                                        const int32_t* line_tab) {
    const int c4n = C >> 2;
    const long total = (long)N * OW * c4n;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int c = (int)(idx % c4n) << 2;
        const long pix = idx / c4n;
        const int ow = (int)(pix % OW);
        const int n = (int)(pix / OW);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int kw = 0; kw < 2; ++kw)
                acc += lcv3_hswish_aff(*reinterpret_cast<const f32x4*>(x + (((size_t)n * H + kh) * W + ow * 2 + kw) * xld + c), 1.f, 0.f);
        const f32x4 o = acc * 0.25f;
        if (line_tab) {
            const int t_n = min(line_tab[n * kLineTabStride + 2], W) >> 1;
            if (ow < t_n) *reinterpret_cast<f32x4*>(y + (size_t)(line_tab[n * kLineTabStride + 3] + ow) * yld + c) = o;
        } else {
            *reinterpret_cast<f32x4*>(y + (size_t)pix * yld + c) = o;
        }
    }
}
void launch_mv1e_pool(const float* x, int xld, float* y, int yld, int N, int H, int W, int C, hipStream_t s, const int32_t* line_tab) {
    const int OW = W / 2;
    if (OW < 1 || H < 2) return;
    const long blocks = ((long)N * OW * (C >> 2) + 255) / 256;
    hipLaunchKernelGGL(mv1e_pool_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks > 65536 ? 65536 : blocks)), dim3(256), 0, s, x, xld, y, yld, N, H, W, C, OW,
                       line_tab);
}

}  // namespace rd
