// PPLCNetV3 (PP-OCRv5 mobile recogniser) depthwise layer and its helpers.  A LearnableRepLayer is, after the load-time fold
// (derive_ppocrv5_rec_mobile_weights), one convolution + bias, then hardswish, then the scalar affine `act.lab`:
//   y = post_s * hardswish(dw_kxk(x') + bias) + post_b
// The PRODUCER of x is a pointwise layer that wrote its convolution + bias only: the matrix kernels' shared epilogue (rd_act) stays as it
// is - one more case in it costs conv_igemm_h3_kernel<256,128> two spilled registers (tests/test_isa_resources.py) - so that layer's
// hardswish and `act.lab` are applied here, on load, to the elements INSIDE the map - x' = pre_s hardswish(x) + pre_b (pre_act) - while the
// convolution's padding stays zero, as in the reference, where activation and affine precede the padding.
// Per-line widths (rd_kernels.h LineTab): input columns >= line_in[n] are that padding too (whatever the shared tensor holds there),
// output columns >= line_out[n] are written as zeros.  Strides (1,1), (2,1) and (1,2); 3x3 and 5x5 (5x5 at (1,2): MobileNetV1Enhance's last
// block, build_ppocr_rec_mv1e, whose LDS-staged alternative to this kernel is kernels_mv1e.hip).
// The mobile DETECTOR (build_ppocrv5_det_mobile) adds stride (2,2) for both kernel sizes and post_act = 0: the reference skips the
// activation of a layer whose stride is the integer 2, so such a layer writes dw_kxk(x') + bias and nothing else.  The detector's
// LDS-staged alternative to this kernel is kernels_lcv3_det.hip.
// One thread = 4 channels x TW adjacent output columns of one row: the (TW - 1) SW + K input columns of a kernel row are loaded once
// and feed all TW outputs.  Channel quads are the fastest thread index: every load is a coalesced 16-byte access.
#include "rd_device.h"

namespace rd {

template <int K, int SW, int TW>
__global__ void __launch_bounds__(256) lcv3_dw_kernel(Lcv3DwParams p) {
    constexpr int P = K / 2, NIN = (TW - 1) * SW + K;
    const int c4n = p.C >> 2;
    const int owt = (p.OW + TW - 1) / TW;
    const long total = (long)p.N * p.OH * owt * c4n;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int c = (int)(idx % c4n) << 2;
        long t = idx / c4n;
        const int ow0 = (int)(t % owt) * TW;
        t /= owt;
        const int oh = (int)(t % p.OH);
        const int n = (int)(t / p.OH);
        const int lw_in = p.line_in ? min(p.line_in[n * p.line_stride], p.W) : p.W;
        const int lw_out = p.line_out ? min(p.line_out[n * p.line_stride], p.OW) : p.OW;
        const f32x4 bias = *reinterpret_cast<const f32x4*>(p.bias + c);
        f32x4 acc[TW];
#pragma unroll
        for (int j = 0; j < TW; ++j) acc[j] = bias;
        const int iw0 = ow0 * SW - P;
#pragma unroll
        for (int kh = 0; kh < K; ++kh) {
            const int ih = oh * p.SH - P + kh;
            if (ih < 0 || ih >= p.H) continue;
            const float* row = p.x + ((size_t)n * p.H + ih) * p.W * p.xld + c;
            f32x4 in[NIN];
#pragma unroll
            for (int i = 0; i < NIN; ++i) {
                const int iw = iw0 + i;
                if (iw >= 0 && iw < lw_in) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(row + (size_t)iw * p.xld);
                    in[i] = p.pre_act ? lcv3_hswish_aff(v, p.pre_s, p.pre_b) : v;
                } else {
                    in[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
#pragma unroll
            for (int kw = 0; kw < K; ++kw) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(p.w + (size_t)(kh * K + kw) * p.C + c);
#pragma unroll
                for (int j = 0; j < TW; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(in[j * SW + kw][e], wv[e], acc[j][e]);
            }
        }
        float* yrow = p.y + ((size_t)n * p.OH + oh) * p.OW * p.yld + c;
#pragma unroll
        for (int j = 0; j < TW; ++j) {
            const int ow = ow0 + j;
            if (ow >= p.OW) break;
            const f32x4 o = ow >= lw_out ? f32x4{0.f, 0.f, 0.f, 0.f} : p.post_act ? lcv3_hswish_aff(acc[j], p.post_s, p.post_b) : acc[j];
            *reinterpret_cast<f32x4*>(yrow + (size_t)ow * p.yld) = o;
        }
    }
}

static inline int lcv3_grid(long total) {
    long g = (total + 255) / 256;
    return (int)(g < 1 ? 1 : g > 65536 ? 65536 : g);
}

bool lcv3_dw_shape_ok(int k, int sh, int sw, int c) {
    return (k == 3 || k == 5) && c % 4 == 0 && ((sh == 1 && sw == 1) || (sh == 2 && sw == 1) || (sh == 1 && sw == 2) || (sh == 2 && sw == 2));
}

void launch_lcv3_dw(const Lcv3DwParams& p, hipStream_t s) {
    constexpr int TW = 4;
    const long total = (long)p.N * p.OH * ((p.OW + TW - 1) / TW) * (p.C >> 2);
    const dim3 g(lcv3_grid(total)), b(256);
    if (p.K == 3 && p.SW == 1) hipLaunchKernelGGL((lcv3_dw_kernel<3, 1, TW>), g, b, 0, s, p);
    else if (p.K == 3 && p.SW == 2) hipLaunchKernelGGL((lcv3_dw_kernel<3, 2, TW>), g, b, 0, s, p);
    else if (p.K == 5 && p.SW == 1) hipLaunchKernelGGL((lcv3_dw_kernel<5, 1, TW>), g, b, 0, s, p);
    else if (p.K == 5 && p.SW == 2) hipLaunchKernelGGL((lcv3_dw_kernel<5, 2, TW>), g, b, 0, s, p);
}

// SE pooling partial sums of a depthwise output under per-line widths: partial[n][h][c] = sum over w < line_w[n] of x[n][h][w][c], one
// chunk per map row (SeFcParams::chunks = H).  One workgroup of 1024 threads per (n, h): S = 1024 / (C / 4) threads share a channel quad.
// Columns are cut into chunks of 16 at ABSOLUTE positions; thread s of a quad adds chunks s, s + S, ... in column order, and the S partial
// sums are added in the order of s.  The order depends on the line's width and on C only: the sum of a line does not depend on the
// launch it rides in.
constexpr int LCV3_GAP_THREADS = 1024, LCV3_GAP_CHUNK = 16;
__global__ void __launch_bounds__(LCV3_GAP_THREADS) lcv3_gap_rows_kernel(const float* x, int xld, int H, int W, int C, float* partial,
                                                                         const int32_t* line_w, int stride) {
    __shared__ f32x4 part[LCV3_GAP_THREADS];
    const int n = blockIdx.y, h = blockIdx.x;
    const int lw = line_w ? min(line_w[n * stride], W) : W;
    const int nq = C >> 2, S = LCV3_GAP_THREADS / nq;            // (the launcher checks nq <= 1024)
    const int t = threadIdx.x, q = t % nq, s = t / nq;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (s < S) {
        const float* row = x + ((size_t)n * H + h) * W * xld + (q << 2);
        for (int w0 = s * LCV3_GAP_CHUNK; w0 < lw; w0 += S * LCV3_GAP_CHUNK) {
            const int w1 = min(w0 + LCV3_GAP_CHUNK, lw);
            for (int w = w0; w < w1; ++w) acc += *reinterpret_cast<const f32x4*>(row + (size_t)w * xld);
        }
    }
    part[t] = acc;
    __syncthreads();
    if (t < nq) {
        f32x4 r = part[t];
        for (int k = 1; k < S; ++k) r += part[k * nq + t];
        *reinterpret_cast<f32x4*>(partial + ((size_t)n * H + h) * C + (t << 2)) = r;
    }
}
bool lcv3_gap_shape_ok(int c) { return c % 4 == 0 && c >= 4 && (c >> 2) <= LCV3_GAP_THREADS; }
void launch_lcv3_gap_rows(const float* x, int xld, int N, int H, int W, int C, float* partial, const int32_t* line_w, int stride, hipStream_t s) {
    if (!lcv3_gap_shape_ok(C)) return;
    hipLaunchKernelGGL(lcv3_gap_rows_kernel, dim3(H, N), dim3(LCV3_GAP_THREADS), 0, s, x, xld, H, W, C, partial, line_w, stride);
}

// The backbone's end: the last pointwise layer's deferred hardswish on load, avg_pool2d([3, 2]), then its `act.lab` (the mean of an
// affine map is the affine map of the mean).  line_tab as launch_avgpool3x2: line n writes its w4 / 2 tokens at row line_tab[4 n + 3].
__global__ void __launch_bounds__(256) lcv3_pool_kernel(const float* x, int xld, float* y, int yld, int N, int H, int W, int C, int OW, float post_s,
                                                        float post_b, const int32_t* line_tab) {
    const int c4n = C >> 2;
    const long total = (long)N * OW * c4n;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int c = (int)(idx % c4n) << 2;
        const long pix = idx / c4n;
        const int ow = (int)(pix % OW);
        const int n = (int)(pix / OW);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 2; ++kw)
                acc += lcv3_hswish_aff(*reinterpret_cast<const f32x4*>(x + (((size_t)n * H + kh) * W + ow * 2 + kw) * xld + c), 1.f, 0.f);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaf(acc[e] * (1.f / 6.f), post_s, post_b);
        if (line_tab) {
            const int t_n = min(line_tab[n * kLineTabStride + 2], W) >> 1;
            if (ow < t_n) *reinterpret_cast<f32x4*>(y + (size_t)(line_tab[n * kLineTabStride + 3] + ow) * yld + c) = o;
        } else {
            *reinterpret_cast<f32x4*>(y + (size_t)pix * yld + c) = o;
        }
    }
}
void launch_lcv3_pool(const float* x, int xld, float* y, int yld, int N, int H, int W, int C, float post_s, float post_b, hipStream_t s,
                      const int32_t* line_tab) {
    const int OW = (W - 2) / 2 + 1;
    hipLaunchKernelGGL(lcv3_pool_kernel, dim3(lcv3_grid((long)N * OW * (C >> 2))), dim3(256), 0, s, x, xld, y, yld, N, H, W, C, OW, post_s, post_b,
                       line_tab);
}

}  // namespace rd
