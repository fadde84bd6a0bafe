// The small kernels of PPHGNet_small (PP-OCRv4 server models, rec_hgnet.py) besides its convolutions:
//   * the ESE gate of an HG_Block (rec_hgnet.py:34-52): s[n][c] = sigmoid(b[c] + sum_k W[c][k] mean_hw(x)[n][k]), y = x s (+ identity),
//     C = 256 .. 1024.  One FC with bias: se_fc_kernel (kernels_misc.hip) is the two-FC hard-sigmoid gate for C <= 512 and does not serve it.
//     The pooled sums come from launch_gap_partial (deterministic, chunk count from H x W alone: ese_gap_chunks);
//   * the detector stem's MaxPool2d(3, stride 2, padding 1) (rec_hgnet.py:205-206), padding = -inf as torch's.
// Plain fp32 in every precision mode; every sum has a fixed order, and nothing depends on the batch size.
#include <algorithm>
#include <cmath>

#include "rd_device.h"

namespace rd {

bool ese_shape_ok(int c) { return c % 4 == 0 && c >= 4 && c <= 1024; }
int ese_gap_chunks(int hw) { return std::max(1, std::min(64, hw / 256)); }

// grid (C / 16, N), 256 threads: the workgroup first adds the partial sums of image n into mean[C] in LDS (chunk order), then each of
// its four wavefronts computes four rows of W: lanes stride over k (a row is read coalesced), a fixed butterfly adds the 64 lane sums.
__global__ void __launch_bounds__(256) ese_gate_kernel(const float* __restrict__ partial, int chunks, int C, float inv_hw, const float* __restrict__ w,
                                                       const float* __restrict__ b, float* __restrict__ s) {
    __shared__ float mean[1024];
    const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int c = tid; c < C; c += 256) {
        float a = 0.f;
        for (int k = 0; k < chunks; ++k) a += partial[((size_t)n * chunks + k) * C + c];
        mean[c] = a * inv_hw;
    }
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
        const int c = blockIdx.x * 16 + wave * 4 + j;
        if (c >= C) break;
        const float* row = w + (size_t)c * C;
        float a = 0.f;
        for (int k = lane; k < C; k += 64) a = fmaf(row[k], mean[k], a);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) s[(size_t)n * C + c] = 1.f / (1.f + __expf(-(a + b[c])));
    }
}

void launch_ese_gate(const float* partial, int chunks, int N, int C, float inv_hw, const float* w, const float* b, float* s, hipStream_t st) {
    if (N <= 0) return;
    hipLaunchKernelGGL(ese_gate_kernel, dim3((C + 15) / 16, N), dim3(256), 0, st, partial, chunks, C, inv_hw, w, b, s);
}

// y = x s (+ identity), 16 bytes per thread; in place (y == x) or into a channel slot
__global__ void __launch_bounds__(256) ese_apply_kernel(const float* x, int xld, const float* __restrict__ s, const float* idn, int ild, float* y, int yld,
                                                        int HW, int C, long total) {
    const int c4n = C >> 2;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int c = (int)(idx % c4n) << 2;
        const long pix = idx / c4n;
        const long n = pix / HW;
        f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)pix * xld + c);
        v *= *reinterpret_cast<const f32x4*>(s + (size_t)n * C + c);
        if (idn) v += *reinterpret_cast<const f32x4*>(idn + (size_t)pix * ild + c);
        *reinterpret_cast<f32x4*>(y + (size_t)pix * yld + c) = v;
    }
}

static inline unsigned ese_grid(long total) { return (unsigned)std::max(1L, std::min((total + 255) / 256, 256L * 64)); }

void launch_ese_apply(const float* x, int xld, const float* s, const float* idn, int ild, float* y, int yld, int N, int HW, int C, hipStream_t st) {
    const long total = (long)N * HW * (C >> 2);
    if (total <= 0) return;
    hipLaunchKernelGGL(ese_apply_kernel, dim3(ese_grid(total)), dim3(256), 0, st, x, xld, s, idn, ild, y, yld, HW, C, total);
}

// MaxPool2d(3, stride 2, padding 1): OH = (H - 1) / 2 + 1; the window's taps outside the map do not take part (torch pads with -inf)
__global__ void __launch_bounds__(256) maxpool3x3s2_kernel(const float* __restrict__ x, int xld, float* __restrict__ y, int yld, int H, int W, int C, int OH,
                                                           int OW, long total) {
    const int c4n = C >> 2;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int c = (int)(idx % c4n) << 2;
        const long pix = idx / c4n;
        const int ow = (int)(pix % OW);
        const int oh = (int)((pix / OW) % OH);
        const long n = pix / ((long)OW * OH);
        f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int ih = 2 * oh - 1 + a;
            if ((unsigned)ih >= (unsigned)H) continue;
#pragma unroll
            for (int bb = 0; bb < 3; ++bb) {
                const int iw = 2 * ow - 1 + bb;
                if ((unsigned)iw >= (unsigned)W) continue;
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + (((size_t)n * H + ih) * W + iw) * xld + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) m[e] = (v[e] != v[e]) ? v[e] : (m[e] != m[e] ? m[e] : fmaxf(m[e], v[e]));   // NaN propagates, as torch's
            }
        }
        *reinterpret_cast<f32x4*>(y + (size_t)pix * yld + c) = m;
    }
}

void launch_maxpool3x3s2(const float* x, int xld, float* y, int yld, int N, int H, int W, int C, hipStream_t st) {
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const long total = (long)N * OH * OW * (C >> 2);
    if (total <= 0) return;
    hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3(ese_grid(total)), dim3(256), 0, st, x, xld, y, yld, H, W, C, OH, OW, total);
}

}  // namespace rd
