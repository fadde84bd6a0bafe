// MobileNetV3 (small, scale 0.35, WITH squeeze-excite) in the text-line geometry: the backbone of the 0 / 180 degree text-line direction
// classifier ch_ptocr_mobile_v2.0_cls_mobile (build_ppocr_cls_mobile).  Every block strides the HEIGHT only - (2, 1) or (1, 1) - so the
// maps are 24 ... 2 rows by 96 columns at 8 ... 200 channels: launch-latency territory, one line costs 32.6 MFLOP.
//
// mbv3s_dw_kernel<K, SH, SW>: the depthwise layer with separate row and column strides, C % 8 == 0.  The idiom is mbv3_dw_kernel's
// (kernels_mbv3.hip, which knows one stride for both axes and is left as it is): one thread = 4 channels x TW adjacent output columns of one
// row, channel quads fastest, every access a coalesced 16 bytes, every load guarded by the map's bounds, a grid-stride loop whose grid
// `max_blocks` caps.  pre_act is the PRODUCER's activation, applied on load to the elements inside the map only - the padding is zeros of
// the ACTIVATED tensor, not act(bias); post_act is the layer's own, applied in the epilogue.  The sum runs from the bias over kh, kw upwards:
// a property of the layer, whatever the thread, the grid or the image index.
//
// cls_tail_kernel: the classifier's end behind conv2's convolution + bias t [N][H2][W2][C]: hardswish -> MaxPool2d(2, 2) -> global
// average -> Linear C -> 2 -> softmax(dim 1), one workgroup per line.  Thread c owns channel c: the maximum of the four ACTIVATED values of
// a window (hardswish is not monotonic, so the activation comes first), windows summed row-major from zero, divided once; the two logits
// run from their bias over the channel index upwards in one thread each.  No atomics: a line's bits depend on nothing but the line.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): docs/notebook/cls_mobile.md.  No scratch, nothing spilled
// (tests/test_isa_resources.py::test_no_hot_kernel_spills).
#include "rd_device.h"

#include <algorithm>

namespace rd {

__device__ __forceinline__ float mbv3s_act1(float v, int act) {
    if (act == MBV3_RELU) return fmaxf(v, 0.f);
    if (act == MBV3_HSWISH) return v * fminf(fmaxf(v + 3.f, 0.f), 6.f) * (1.f / 6.f);
    return v;
}
__device__ __forceinline__ f32x4 mbv3s_act4(f32x4 v, int act) {
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = mbv3s_act1(v[e], act);
    return r;
}

// ---------------------------------------------------------------------------------------------------------------- depthwise layer
template <int K, int SH, int SW, int TW>
__global__ void __launch_bounds__(256) mbv3s_dw_kernel(Mbv3sDwParams p) {
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
        const f32x4 bias = *reinterpret_cast<const f32x4*>(p.bias + c);
        f32x4 acc[TW];
#pragma unroll
        for (int j = 0; j < TW; ++j) acc[j] = bias;
        const int iw0 = ow0 * SW - P;
#pragma unroll
        for (int kh = 0; kh < K; ++kh) {
            const int ih = oh * SH - P + kh;
            if (ih < 0 || ih >= p.H) continue;
            const float* row = p.x + ((size_t)n * p.H + ih) * p.W * p.xld + c;
            f32x4 in[NIN];
#pragma unroll
            for (int i = 0; i < NIN; ++i) {
                const int iw = iw0 + i;
                in[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (iw >= 0 && iw < p.W) in[i] = mbv3s_act4(*reinterpret_cast<const f32x4*>(row + (size_t)iw * p.xld), p.pre_act);
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
            *reinterpret_cast<f32x4*>(yrow + (size_t)ow * p.yld) = mbv3s_act4(acc[j], p.post_act);
        }
    }
}

static inline bool mbv3s_act_ok(int a) { return a == MBV3_NONE || a == MBV3_RELU || a == MBV3_HSWISH; }
static inline bool mbv3s_aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

bool mbv3s_dw_shape_ok(int k, int sh, int sw, int c) { return (k == 3 || k == 5) && (sh == 1 || sh == 2) && sw == 1 && c >= 8 && c % 8 == 0; }

bool mbv3s_dw_launch_ok(const Mbv3sDwParams& p) {
    return mbv3s_dw_shape_ok(p.K, p.SH, p.SW, p.C) && p.N >= 1 && p.H >= 1 && p.W >= 1 && p.OH == (p.H - 1) / p.SH + 1 && p.OW == (p.W - 1) / p.SW + 1 &&
           p.xld >= p.C && p.yld >= p.C && p.xld % 4 == 0 && p.yld % 4 == 0 && mbv3s_act_ok(p.pre_act) && mbv3s_act_ok(p.post_act) &&
           (size_t)p.N * p.H * p.W * p.xld < ((size_t)1 << 40) &&
           mbv3s_aligned16(p.x) && mbv3s_aligned16(p.y) && mbv3s_aligned16(p.w) && mbv3s_aligned16(p.bias);   // (a null pointer: filled in later)
}

bool launch_mbv3s_dw(const Mbv3sDwParams& p, hipStream_t s) {
    if (!mbv3s_dw_launch_ok(p) || !p.x || !p.y || !p.w || !p.bias) return false;
    constexpr int TW = 4;
    const long total = (long)p.N * p.OH * ((p.OW + TW - 1) / TW) * (p.C >> 2);
    const long blocks = (total + 255) / 256;
    const long cap = p.max_blocks > 0 ? p.max_blocks : 65536;                 // (grid-stride loop; max_blocks: a test's way to the wrap)
    const dim3 g((unsigned)(blocks > cap ? cap : blocks)), b(256);
    if (p.K == 3 && p.SH == 1) hipLaunchKernelGGL((mbv3s_dw_kernel<3, 1, 1, TW>), g, b, 0, s, p);
    else if (p.K == 3 && p.SH == 2) hipLaunchKernelGGL((mbv3s_dw_kernel<3, 2, 1, TW>), g, b, 0, s, p);
    else if (p.K == 5 && p.SH == 1) hipLaunchKernelGGL((mbv3s_dw_kernel<5, 1, 1, TW>), g, b, 0, s, p);
    else hipLaunchKernelGGL((mbv3s_dw_kernel<5, 2, 1, TW>), g, b, 0, s, p);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- classifier tail
constexpr int CLS_TAIL_MAX_C = 1024;

__global__ void __launch_bounds__(256) cls_tail_kernel(ClsTailParams p) {
    __shared__ float feat[CLS_TAIL_MAX_C];
    __shared__ float logit[2];
    const int n = blockIdx.x;
    const int ph = p.H >> 1, pw = p.W >> 1;
    const float* x = p.x + (size_t)n * p.H * p.W * p.xld;
    for (int c = threadIdx.x; c < p.C; c += 256) {
        float sum = 0.f;
        for (int r = 0; r < ph; ++r)
            for (int q = 0; q < pw; ++q) {
                const float* a = x + ((size_t)(2 * r) * p.W + 2 * q) * p.xld + c;
                const float* b = a + (size_t)p.W * p.xld;
                const float m = fmaxf(fmaxf(mbv3s_act1(a[0], MBV3_HSWISH), mbv3s_act1(a[p.xld], MBV3_HSWISH)),
                                      fmaxf(mbv3s_act1(b[0], MBV3_HSWISH), mbv3s_act1(b[p.xld], MBV3_HSWISH)));
                sum += m;
            }
        feat[c] = sum / (float)(ph * pw);
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const float* w = p.w + (size_t)threadIdx.x * p.C;
        float acc = p.bias[threadIdx.x];
        for (int c = 0; c < p.C; ++c) acc = fmaf(feat[c], w[c], acc);
        logit[threadIdx.x] = acc;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const float m = fmaxf(logit[0], logit[1]);
        const float e0 = expf(logit[0] - m), e1 = expf(logit[1] - m);
        p.prob[(size_t)n * 2 + threadIdx.x] = (threadIdx.x == 0 ? e0 : e1) / (e0 + e1);
    }
    if (p.aux) {
        float* a = p.aux + (size_t)n * (2 + p.C);
        if (threadIdx.x < 2) a[threadIdx.x] = logit[threadIdx.x];
        for (int c = threadIdx.x; c < p.C; c += 256) a[2 + c] = feat[c];
    }
}

bool cls_tail_launch_ok(const ClsTailParams& p) {
    return p.N >= 1 && p.H >= 2 && p.W >= 2 && p.C >= 1 && p.C <= CLS_TAIL_MAX_C && p.xld >= p.C;
}

bool launch_cls_tail(const ClsTailParams& p, hipStream_t s) {
    if (!cls_tail_launch_ok(p) || !p.x || !p.w || !p.bias || !p.prob) return false;
    hipLaunchKernelGGL(cls_tail_kernel, dim3((unsigned)p.N), dim3(256), 0, s, p);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- the whole network in one launch
// cls_line_kernel: one 512-thread workgroup owns one line at a time (a persistent grid walks the batch) and runs conv1, the eleven blocks, conv2,
// both pools, the FC and the softmax; all synchronisation is __syncthreads().  Per workgroup, a region of the workspace holds the block
// input / output ping-pong (NHWC) and the depthwise output d; LDS holds what is re-used: the slice of the expanded map the depthwise taps
// read, the squeeze-excite vectors, the last map under conv2.
//   expand + depthwise  over slices of `ms` mid channels (both are independent per mid channel, so only H x W x ms of the expanded map is
//                       ever live, in LDS; a pixel outside the map contributes nothing: the padding is zeros of the ACTIVATED map)
//   d                   goes to the workgroup's global region and is re-read through L1 / L2 by the pooling and by the linear layer: blocks
//                       9 / 10 would need 153 600 B of LDS for it, which leaves no room for a second workgroup on the CU or for a useful
//                       slice (docs/notebook/cls_mobile.md: the measured choice)
//   squeeze-excite      per-channel sums of the activated d: along each row, then over the rows, both ascending; the two FCs from their
//                       bias over the input index upwards, once per line; gate = clamp(0.2 v + 0.5, 0, 1) (the paddle hard-sigmoid)
//   linear              y = bl + sum over m ascending of (gate[m] d[m]) wl[co][m], + x on a shortcut
//   tail                conv2 + hardswish + MaxPool2d(2, 2) per channel and window, the windows summed row-major in two halves that are
//                       added first + second, / windows; logits from the bias over the channel index upwards; softmax
// Every sum's order is a property of the layer and of the map size: a line's bits do not depend on its index, the batch or the grid.
// All fp32 FMA chains: no precision mode and no range guard applies (as mbv3_block_kernel).  No floating-point atomics.
constexpr int CLS_T = 512;
constexpr int CLS_ES = 18432;                 // floats of LDS for the expanded slice (72 KB): 24 x 96 pixels x 8 channels in one piece
constexpr int CLS_VEC = 256, CLS_HID = 64;        // squeeze-excite vectors: mid <= 256, mid / 4 <= 64
constexpr int CLS_LDS_FLOATS = CLS_ES + 2 * CLS_VEC + CLS_HID;      // 76 032 B: two workgroups per CU
constexpr int CLS_CONV2_CIN = 32;
constexpr int CLS_MAX_GRID = 512;             // two workgroups on each of 256 CUs

__device__ __forceinline__ void cls_block(const ClsBlockParams& L, const float* __restrict__ X, float* __restrict__ Y, float* __restrict__ D, int H, int W,
                                          float* lds) {
    float* es = lds;
    float* rows = lds;                 // the row sums of d: over the slice, which is dead by then
    float* pooled = lds + CLS_ES;
    float* gate = pooled + CLS_VEC;
    float* hid = gate + CLS_VEC;
    const int tid = threadIdx.x;
    const int K = L.k, P = K >> 1, cin = L.cin, mid = L.mid, cout = L.cout, sh = L.sh;
    const int OH = (H - 1) / sh + 1, OW = W, px = H * W, opx = OH * OW;
    for (int m0 = 0; m0 < mid; m0 += L.ms) {
        const int mw = min(L.ms, mid - m0), q4 = mw >> 2;
        // expand: es[p][j] = act(be + x[p] . we[m]) for the slice's channels
        for (int it = tid; it < px * q4; it += CLS_T) {
            const int j = it % q4, p = it / q4, m = m0 + (j << 2);
            f32x4 acc = *reinterpret_cast<const f32x4*>(L.be + m);
            const float* xp = X + (size_t)p * cin;
            for (int k = 0; k < cin; k += 4) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(xp + k);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(L.we + (size_t)(m + e) * cin + k);
                    acc[e] = fmaf(xv[3], wv[3], fmaf(xv[2], wv[2], fmaf(xv[1], wv[1], fmaf(xv[0], wv[0], acc[e]))));
                }
            }
            *reinterpret_cast<f32x4*>(es + (size_t)p * L.es_ld + (j << 2)) = mbv3s_act4(acc, L.act);
        }
        __syncthreads();
        // depthwise over the slice: d[op][m] = act(bd + taps inside the map)
        for (int it = tid; it < opx * q4; it += CLS_T) {
            const int j = it % q4, op = it / q4, m = m0 + (j << 2);
            const int ow = op % OW, oh = op / OW;
            f32x4 acc = *reinterpret_cast<const f32x4*>(L.bd + m);
            for (int kh = 0; kh < K; ++kh) {
                const int ih = oh * sh - P + kh;
                if (ih < 0 || ih >= H) continue;
                for (int kw = 0; kw < K; ++kw) {
                    const int iw = ow - P + kw;
                    if (iw < 0 || iw >= W) continue;
                    const f32x4 ev = *reinterpret_cast<const f32x4*>(es + (size_t)(ih * W + iw) * L.es_ld + (j << 2));
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(L.wd + (size_t)(kh * K + kw) * mid + m);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = fmaf(ev[e], wv[e], acc[e]);
                }
            }
            *reinterpret_cast<f32x4*>(D + (size_t)op * mid + m) = mbv3s_act4(acc, L.act);
        }
        __syncthreads();
    }
    if (L.se) {
        for (int it = tid; it < OH * mid; it += CLS_T) {
            const int c = it % mid, r = it / mid;
            const float* dp = D + (size_t)r * OW * mid + c;
            float sum = 0.f;
            for (int w = 0; w < OW; ++w) sum += dp[(size_t)w * mid];
            rows[it] = sum;
        }
        __syncthreads();
        for (int c = tid; c < mid; c += CLS_T) {
            float sum = 0.f;
            for (int r = 0; r < OH; ++r) sum += rows[r * mid + c];
            pooled[c] = sum / (float)opx;
        }
        __syncthreads();
        const int cr = mid >> 2;
        for (int j = tid; j < cr; j += CLS_T) {
            float a = L.b1[j];
            for (int c = 0; c < mid; ++c) a = fmaf(pooled[c], L.w1[(size_t)j * mid + c], a);
            hid[j] = fmaxf(a, 0.f);
        }
        __syncthreads();
        for (int c = tid; c < mid; c += CLS_T) {
            float a = L.b2[c];
            for (int j = 0; j < cr; ++j) a = fmaf(hid[j], L.w2[(size_t)c * cr + j], a);
            gate[c] = fminf(fmaxf(fmaf(0.2f, a, 0.5f), 0.f), 1.f);
        }
        __syncthreads();
    }
    const int cq = cout >> 2;
    for (int it = tid; it < opx * cq; it += CLS_T) {
        const int q = it % cq, p = it / cq, co = q << 2;
        f32x4 acc = *reinterpret_cast<const f32x4*>(L.bl + co);
        const float* dp = D + (size_t)p * mid;
        for (int m = 0; m < mid; m += 4) {
            f32x4 dv = *reinterpret_cast<const f32x4*>(dp + m);
            if (L.se) {
#pragma unroll
                for (int e = 0; e < 4; ++e) dv[e] *= gate[m + e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(L.wl + (size_t)(co + e) * mid + m);
                acc[e] = fmaf(dv[3], wv[3], fmaf(dv[2], wv[2], fmaf(dv[1], wv[1], fmaf(dv[0], wv[0], acc[e]))));
            }
        }
        if (L.shortcut) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(X + (size_t)p * cin + co);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += xv[e];
        }
        *reinterpret_cast<f32x4*>(Y + (size_t)p * cout + co) = acc;
    }
    __syncthreads();
}

// one block alone, one workgroup per image (rd_debug_mbv3s_block route 1): x / y contiguous NHWC in the caller's buffers with row strides
// xld / yld, copied through the workgroup's region so that the block itself is the code the network runs
__global__ void __launch_bounds__(CLS_T) cls_block_kernel(ClsBlockParams L, const float* __restrict__ x, int xld, float* __restrict__ y, int yld, int N, int H,
                                                          int W, float* __restrict__ scratch, size_t per_wg) {
    extern __shared__ __attribute__((aligned(16))) float cls_lds[];
    const int OH = (H - 1) / L.sh + 1;
    float* X = scratch + (size_t)blockIdx.x * per_wg;
    float* Y = X + (((size_t)H * W * L.cin + 3) & ~(size_t)3);
    float* D = Y + (((size_t)OH * W * L.cout + 3) & ~(size_t)3);
    for (int n = blockIdx.x; n < N; n += gridDim.x) {
        const float* xn = x + (size_t)n * H * W * xld;
        for (int i = threadIdx.x; i < H * W * L.cin; i += CLS_T) X[i] = xn[(size_t)(i / L.cin) * xld + i % L.cin];
        __syncthreads();
        cls_block(L, X, Y, D, H, W, cls_lds);
        float* yn = y + (size_t)n * OH * W * yld;
        for (int i = threadIdx.x; i < OH * W * L.cout; i += CLS_T) yn[(size_t)(i / L.cout) * yld + i % L.cout] = Y[i];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(CLS_T) cls_line_kernel(ClsLineParams p) {
    extern __shared__ __attribute__((aligned(16))) float cls_lds[];
    const int tid = threadIdx.x;
    const int H1 = (p.H - 1) / 2 + 1, W1 = (p.W - 1) / 2 + 1, c1 = p.c1;
    float* A = p.scratch + (size_t)blockIdx.x * p.per_wg;
    float* Bf = A + p.act_floats;
    float* D = Bf + p.act_floats;
    for (int n = blockIdx.x; n < p.B; n += gridDim.x) {
        // conv1: 3x3 / (2,2) / pad 1 from the NCHW image + hardswish -> A [H1][W1][c1]
        const float* xn = p.x + (size_t)n * 3 * p.H * p.W;
        const int c1q = c1 >> 2;
        for (int it = tid; it < H1 * W1 * c1q; it += CLS_T) {
            const int q = it % c1q, pp = it / c1q, co = q << 2;
            const int ow = pp % W1, oh = pp / W1;
            f32x4 acc = *reinterpret_cast<const f32x4*>(p.b1c + co);
            for (int a = 0; a < 3; ++a) {
                const int ih = oh * 2 - 1 + a;
                if (ih < 0 || ih >= p.H) continue;
                for (int b = 0; b < 3; ++b) {
                    const int iw = ow * 2 - 1 + b;
                    if (iw < 0 || iw >= p.W) continue;
#pragma unroll
                    for (int ci = 0; ci < 3; ++ci) {
                        const float xv = xn[((size_t)ci * p.H + ih) * p.W + iw];
                        const f32x4 wv = *reinterpret_cast<const f32x4*>(p.w1c + (size_t)((a * 3 + b) * 3 + ci) * c1 + co);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[e] = fmaf(xv, wv[e], acc[e]);
                    }
                }
            }
            *reinterpret_cast<f32x4*>(A + (size_t)pp * c1 + co) = mbv3s_act4(acc, MBV3_HSWISH);
        }
        __syncthreads();
        float* X = A;
        float* Y = Bf;
        int h = H1;
        int tap = 0;
        for (int i = 0; i < p.n_blocks; ++i) {
            const ClsBlockParams& L = p.blk[i];
            cls_block(L, X, Y, D, h, W1, cls_lds);
            h = (h - 1) / L.sh + 1;
            if (tap < 4 && p.stage_out[tap] && i == p.stage_block[tap]) {       // developer output: the block's result as NCHW
                float* so = p.stage_out[tap] + (size_t)n * L.cout * h * W1;
                for (int j = tid; j < L.cout * h * W1; j += CLS_T) {
                    const int c = j / (h * W1), pp = j % (h * W1);
                    so[j] = Y[(size_t)pp * L.cout + c];
                }
            }
            if (tap < 4 && i == p.stage_block[tap]) ++tap;
            float* t = X; X = Y; Y = t;
        }
        // tail: the last map into LDS, conv2 + hardswish + max-pool per (channel, half of the windows), average, FC, softmax
        const int H2 = h, C2 = p.c2;
        float* xs = cls_lds;
        float* psum = cls_lds + (size_t)H2 * W1 * CLS_CONV2_CIN;       // behind the staged map, inside the slice region (cls_line_plan)
        float* feat = cls_lds + CLS_ES;
        float* logit = feat + CLS_VEC;
        for (int j = tid; j < ((H2 * W1 * CLS_CONV2_CIN) >> 2); j += CLS_T) reinterpret_cast<f32x4*>(xs)[j] = reinterpret_cast<const f32x4*>(X)[j];
        __syncthreads();
        const int PH = H2 >> 1, PW = W1 >> 1, nwin = PH * PW, half = (nwin + 1) >> 1;
        for (int it = tid; it < 2 * C2; it += CLS_T) {
            const int c = it % C2, part = it / C2;
            float wr[CLS_CONV2_CIN];
#pragma unroll
            for (int k = 0; k < CLS_CONV2_CIN; ++k) wr[k] = p.w2c[(size_t)c * CLS_CONV2_CIN + k];
            const float bias = p.b2c[c];
            float sum = 0.f;
            const int w_end = min(nwin, (part + 1) * half);
            for (int win = part * half; win < w_end; ++win) {
                const int r = win / PW, q = win % PW;
                float m = 0.f;
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const float* xp = xs + (size_t)((2 * r + a) * W1 + 2 * q + b) * CLS_CONV2_CIN;
                        float v = bias;
#pragma unroll
                        for (int k = 0; k < CLS_CONV2_CIN; ++k) v = fmaf(xp[k], wr[k], v);
                        v = mbv3s_act1(v, MBV3_HSWISH);
                        m = (a == 0 && b == 0) ? v : fmaxf(m, v);
                    }
                sum += m;
            }
            psum[it] = sum;
        }
        __syncthreads();
        for (int c = tid; c < C2; c += CLS_T) feat[c] = (psum[c] + psum[C2 + c]) / (float)nwin;
        __syncthreads();
        if (tid < 2) {
            float acc = p.bf[tid];
            for (int c = 0; c < C2; ++c) acc = fmaf(feat[c], p.wf[(size_t)tid * C2 + c], acc);
            logit[tid] = acc;
        }
        __syncthreads();
        if (tid < 2) {
            const float m = fmaxf(logit[0], logit[1]);
            const float e0 = expf(logit[0] - m), e1 = expf(logit[1] - m);
            p.prob[(size_t)n * 2 + tid] = (tid == 0 ? e0 : e1) / (e0 + e1);
        }
        if (p.aux) {
            float* a = p.aux + (size_t)n * (2 + C2);
            if (tid < 2) a[tid] = logit[tid];
            for (int c = tid; c < C2; c += CLS_T) a[2 + c] = feat[c];
        }
        __syncthreads();      // the LDS vectors and the region are free for the next line
    }
}

// slice width and LDS row stride of one block at an H x W input map: the widest multiple of 4 channels whose expanded slice fits CLS_ES
// floats; a stride that is a multiple of 32 floats gets 4 more (adjacent pixels would share their banks).  false: no slice fits
bool cls_block_plan(ClsBlockParams& L, int H, int W) {
    const long px = (long)H * W;
    if (px < 1) return false;
    for (int ms = L.mid & ~3; ms >= 4; ms -= 4) {
        const int ld = ms % 32 == 0 ? ms + 4 : ms;
        if (px * ld <= CLS_ES) {
            L.ms = ms; L.es_ld = ld;
            return true;
        }
    }
    return false;
}

static bool cls_block_ok(const ClsBlockParams& L, int H, int W) {
    const int OH = (H - 1) / (L.sh > 0 ? L.sh : 1) + 1;
    return (L.k == 3 || L.k == 5) && (L.sh == 1 || L.sh == 2) && L.cin >= 4 && L.cin % 4 == 0 && L.mid >= 4 && L.mid % 4 == 0 && L.mid <= CLS_VEC &&
           L.cout >= 4 && L.cout % 4 == 0 && (L.act == MBV3_RELU || L.act == MBV3_HSWISH) && (!L.shortcut || (L.sh == 1 && L.cin == L.cout)) &&
           (!L.se || (long)OH * L.mid <= CLS_ES) && H >= 1 && W >= 1 && L.ms >= 4 && L.ms % 4 == 0 && L.es_ld >= L.ms && L.es_ld % 4 == 0 &&
           (long)H * W * L.es_ld <= CLS_ES &&
           mbv3s_aligned16(L.we) && mbv3s_aligned16(L.be) && mbv3s_aligned16(L.wd) && mbv3s_aligned16(L.bd) && mbv3s_aligned16(L.wl) && mbv3s_aligned16(L.bl);
}

size_t cls_block_scratch_floats(const ClsBlockParams& L, int H, int W) {
    const size_t OH = (size_t)(H - 1) / L.sh + 1;
    auto r4 = [](size_t v) { return (v + 3) & ~(size_t)3; };
    return r4((size_t)H * W * L.cin) + r4(OH * W * L.cout) + r4(OH * W * L.mid);
}

bool cls_block_launch_ok(const ClsBlockParams& L, int N, int H, int W, int xld, int yld) {
    return N >= 1 && xld >= L.cin && yld >= L.cout && cls_block_ok(L, H, W);
}

bool launch_cls_block(const ClsBlockParams& L, const float* x, int xld, float* y, int yld, int N, int H, int W, float* scratch, hipStream_t s) {
    if (!cls_block_launch_ok(L, N, H, W, xld, yld) || !x || !y || !scratch || !mbv3s_aligned16(scratch)) return false;
    if (!L.we || !L.be || !L.wd || !L.bd || !L.wl || !L.bl || (L.se && (!L.w1 || !L.b1 || !L.w2 || !L.b2))) return false;
    static unsigned long long opted = 0;
    rd_allow_dynamic_lds(reinterpret_cast<const void*>(cls_block_kernel), CLS_LDS_FLOATS * sizeof(float), opted);
    const int grid = N < CLS_MAX_GRID ? N : CLS_MAX_GRID;
    hipLaunchKernelGGL(cls_block_kernel, dim3(grid), dim3(CLS_T), CLS_LDS_FLOATS * sizeof(float), s, L, x, xld, y, yld, N, H, W, scratch,
                       cls_block_scratch_floats(L, H, W));
    return true;
}

int cls_line_grid(int B, int max_blocks) {
    const int cap = max_blocks > 0 && max_blocks < CLS_MAX_GRID ? max_blocks : CLS_MAX_GRID;
    return B < cap ? B : cap;
}

// fills act_floats / d_floats / per_wg and every block's slice plan for the H x W input; false: a shape the kernel cannot hold (an empty
// map, a map whose narrowest slice overflows LDS, squeeze-excite row sums beyond their LDS vector, conv2 off its 32 -> <= 256 channels)
bool cls_line_plan(ClsLineParams& p) {
    if (p.B < 1 || p.H < 1 || p.W < 1 || p.n_blocks < 1 || p.n_blocks > 11 || p.c1 < 4 || p.c1 % 4 != 0) return false;
    const int H1 = (p.H - 1) / 2 + 1, W1 = (p.W - 1) / 2 + 1;
    if ((long)H1 * W1 * p.c1 > (1l << 24)) return false;
    size_t act = (size_t)H1 * W1 * p.c1, dmax = 0;
    int h = H1, c = p.c1;
    for (int i = 0; i < p.n_blocks; ++i) {
        ClsBlockParams& L = p.blk[i];
        if (L.cin != c || L.sh < 1 || !cls_block_plan(L, h, W1) || !cls_block_ok(L, h, W1)) return false;
        h = (h - 1) / L.sh + 1;
        c = L.cout;
        act = std::max(act, (size_t)h * W1 * c);
        dmax = std::max(dmax, (size_t)h * W1 * L.mid);
    }
    if (c != CLS_CONV2_CIN || p.c2 < 1 || p.c2 > CLS_VEC || h < 2 || W1 < 2 || (long)h * W1 * CLS_CONV2_CIN + 2 * p.c2 > CLS_ES) return false;
    p.act_floats = (act + 3) & ~(size_t)3;
    p.d_floats = (dmax + 3) & ~(size_t)3;
    p.per_wg = 2 * p.act_floats + p.d_floats;
    return true;
}

size_t cls_line_scratch_floats(const ClsLineParams& p) { return (size_t)cls_line_grid(p.B, p.max_blocks) * p.per_wg; }

bool cls_line_launch_ok(const ClsLineParams& p) {
    ClsLineParams q = p;
    if (!cls_line_plan(q) || q.per_wg != p.per_wg || q.act_floats != p.act_floats) return false;
    for (int i = 0; i < p.n_blocks; ++i)
        if (q.blk[i].ms != p.blk[i].ms || q.blk[i].es_ld != p.blk[i].es_ld) return false;
    return mbv3s_aligned16(p.scratch) && mbv3s_aligned16(p.w1c) && mbv3s_aligned16(p.b1c) && (reinterpret_cast<uintptr_t>(p.x) & 3) == 0;
}

bool launch_cls_line(const ClsLineParams& p, hipStream_t s) {
    if (!cls_line_launch_ok(p) || !p.x || !p.prob || !p.scratch || !p.w1c || !p.b1c || !p.w2c || !p.b2c || !p.wf || !p.bf) return false;
    static unsigned long long opted = 0;
    rd_allow_dynamic_lds(reinterpret_cast<const void*>(cls_line_kernel), CLS_LDS_FLOATS * sizeof(float), opted);
    hipLaunchKernelGGL(cls_line_kernel, dim3(cls_line_grid(p.B, p.max_blocks)), dim3(CLS_T), CLS_LDS_FLOATS * sizeof(float), s, p);
    return true;
}

}  // namespace rd
