// Kernels of the UniTable table-structure encoder (a plain ViT-B: d = 768, 12 heads of 64, up to 1024 tokens per image) that the
// convolutional networks never needed: self-attention at head dimension 64, the 16 x 16 patch gather in front of the patch-embedding GEMM,
// the learned position rows, and LayerNorm at C = 768.
//
// vit_attention_kernel: softmax(scale Q K^T) V over packed qkv [B][T][3 * heads * 64] (q | k | v, head-major), fp32 in and out.
//   K and V of one head at T = 784 are 200 KB each, more than the LDS holds: the keys run in tiles of 64 and the softmax is online
//   (running row maximum and sum, flash style).  Both products run on the fp32-input matrix cores (v_mfma_f32_16x16x4_f32: a k-ordered
//   fp32 fma chain, bit for bit), so one kernel serves every precision mode, nothing is converted to fp16 and no range flag is involved.
//   Grid (ceil(T / 64), heads, B), 256 threads; wavefront w of a workgroup owns 16 query rows.  Per key tile and wavefront:
//     S^T [key][query] = K Q^T      A = K rows from LDS, B = Q (registers, loaded once, pre-multiplied by `scale`); the result has the
//                                   query on the lane (lane & 15) and keys 4 (lane >> 4) + r in register r of each 16-key sub-tile
//     online softmax                per lane over its 16 scores, then across the four lane groups that share a query (two shuffles)
//     O^T [d][query] += V^T P^T     B = P^T: register r of a sub-tile IS the operand of the k-step over keys {4 g + r}, no lane movement
//                                   and no LDS round trip; A = V from LDS at those keys
//   A row's sums run over the key tiles in order and over a fixed lane pattern inside a tile: they depend on T alone, never on B or on
//   the workgroup that holds the row.  No atomics.  Keys and query rows >= T are never read (zero-filled in LDS, masked to -inf) and
//   no row >= T is written.
#include <hip/hip_runtime.h>

#include "rd_device.h"
#include "rd_kernels.h"

namespace rd {

namespace {
constexpr int VA_HD = 64;           // head dimension
constexpr int VA_TK = 64;           // keys per tile
constexpr int VA_TQ = 64;           // query rows per workgroup (4 wavefronts x 16)
constexpr int VA_LD = VA_HD + 4;    // LDS row stride in floats: 16 B aligned, and the 16 keys of a sub-tile fall into 16 different bank groups
}  // namespace

__global__ void __launch_bounds__(256) vit_attention_kernel(const float* __restrict__ qkv, float* __restrict__ o, int T, int heads, float scale) {
    __shared__ float Ks[VA_TK * VA_LD];
    __shared__ float Vs[VA_TK * VA_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane & 15, g = lane >> 4;
    const int head = blockIdx.y, b = blockIdx.z;
    const int ld = 3 * heads * VA_HD;
    const float* base = qkv + (size_t)b * T * ld + head * VA_HD;
    const float* kbase = base + heads * VA_HD;
    const float* vbase = base + 2 * heads * VA_HD;

    // Q fragments: query row q, d = 16 g + s for k-step s (the K operand uses the same k order)
    const int q = blockIdx.x * VA_TQ + wave * 16 + lq;
    const bool q_ok = q < T;
    const bool wave_ok = blockIdx.x * VA_TQ + wave * 16 < T;       // wave-uniform: a wavefront without a query row only helps to stage
    float qf[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q_ok) v = *reinterpret_cast<const f32x4*>(base + (size_t)q * ld + 16 * g + 4 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) qf[4 * j + e] = v[e] * scale;
    }

    f32x4 acc[4];                    // O^T: d = 16 i + 4 g + r, query lq
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;      // l_run: this lane's share of the row sum (joined across the lane groups at the end)

    // staging: thread -> (row = tid / 16 + 16 p, float4 column tid % 16) of the K and the V tile
    const int srow = tid >> 4, scol = (tid & 15) * 4;
    f32x4 kpre[4], vpre[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int key = k0 + srow + 16 * p;
            kpre[p] = f32x4{0.f, 0.f, 0.f, 0.f};
            vpre[p] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (key < T) {
                kpre[p] = *reinterpret_cast<const f32x4*>(kbase + (size_t)key * ld + scol);
                vpre[p] = *reinterpret_cast<const f32x4*>(vbase + (size_t)key * ld + scol);
            }
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < T; k0 += VA_TK) {
        __syncthreads();             // every wavefront is done with the previous tile
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            *reinterpret_cast<f32x4*>(&Ks[(srow + 16 * p) * VA_LD + scol]) = kpre[p];
            *reinterpret_cast<f32x4*>(&Vs[(srow + 16 * p) * VA_LD + scol]) = vpre[p];
        }
        __syncthreads();
        if (k0 + VA_TK < T) fetch(k0 + VA_TK);      // the next tile's loads fly under this tile's arithmetic
        if (!wave_ok) continue;

        // S^T = K Q^T: four 16-key sub-tiles, 16 k-steps each
        f32x4 s[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4 kf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) kf[i] = *reinterpret_cast<const f32x4*>(&Ks[(16 * i + lq) * VA_LD + 16 * g + 4 * j]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[i][e], qf[4 * j + e], s[i], 0, 0, 0);
        }
        // online softmax: s[i][r] is the score of key k0 + 16 i + 4 g + r for query lq
        float m_tile = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (k0 + 16 * i + 4 * g + r >= T) s[i][r] = -INFINITY;
                m_tile = fmaxf(m_tile, s[i][r]);
            }
        m_tile = fmaxf(m_tile, __shfl_xor(m_tile, 16, 64));
        m_tile = fmaxf(m_tile, __shfl_xor(m_tile, 32, 64));
        const float m_new = fmaxf(m_run, m_tile);       // finite: key k0 < T is in every tile
        const float alpha = expf(m_run - m_new);        // 0 on the first tile
        m_run = m_new;
        float l_tile = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[i][r] = expf(s[i][r] - m_new);
                l_tile += s[i][r];
            }
        l_run = fmaf(l_run, alpha, l_tile);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] *= alpha;
        // O^T += V^T P^T: k-step (kt, r) sums over keys 16 kt + 4 g + r
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* vrow = &Vs[(16 * kt + 4 * g + r) * VA_LD + lq];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(vrow[16 * i], s[kt][r], acc[i], 0, 0, 0);
            }
    }
    if (!q_ok) return;
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    const float inv = 1.f / l_run;
    float* orow = o + ((size_t)b * T + q) * (heads * VA_HD) + head * VA_HD;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(orow + 16 * i + 4 * g) = acc[i] * inv;
}

bool vit_attention_applies(int T, int hd) { return hd == VA_HD && T >= 1 && T <= 1024; }

void launch_vit_attention(const float* qkv, float* o, int B, int T, int heads, float scale, hipStream_t s) {
    hipLaunchKernelGGL(vit_attention_kernel, dim3((T + VA_TQ - 1) / VA_TQ, heads, B), dim3(256), 0, s, qkv, o, T, heads, scale);
}

// --------------------------------------------------------------------------------------------------
// Patch gather: x NCHW [B][3][H][W] -> rows [B * (H/16) * (W/16)][3 * 16 * 16], column k = (c * 16 + ky) * 16 + kx - the order of a
// Conv2d(3, D, 16, stride 16) weight row, so that the patch embedding is one GEMM on the weight as it is stored.  One float4 per thread.
// --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vit_patchify_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, long total) {
    const int pw = W >> 4, T = (H >> 4) * pw;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int k = (int)(idx % 192) << 2;
        const long m = idx / 192;
        const int t = (int)(m % T), b = (int)(m / T);
        const int c = k >> 8, ky = (k >> 4) & 15, kx = k & 15;
        const int py = t / pw, px = t % pw;
        *reinterpret_cast<f32x4*>(y + m * 768 + k) =
            *reinterpret_cast<const f32x4*>(x + (((size_t)b * 3 + c) * H + py * 16 + ky) * W + px * 16 + kx);
    }
}
void launch_vit_patchify(const float* x, float* y, int B, int H, int W, hipStream_t s) {
    const long total = (long)B * (H >> 4) * (W >> 4) * 192;
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(vit_patchify_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, x, y, H, W, total);
}

// x[b][t][:] += pos[t][:]  (learned position rows; C % 4 == 0), in place
__global__ void __launch_bounds__(256) vit_add_pos_kernel(float* __restrict__ x, const float* __restrict__ pos, int T, int C, long total) {
    const int c4n = C >> 2;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int c = (int)(idx % c4n) << 2;
        const long m = idx / c4n;
        f32x4* p = reinterpret_cast<f32x4*>(x + m * C + c);
        *p = *p + *reinterpret_cast<const f32x4*>(pos + (size_t)(m % T) * C + c);
    }
}
void launch_vit_add_pos(float* x, const float* pos, int B, int T, int C, hipStream_t s) {
    const long total = (long)B * T * (C >> 2);
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(vit_add_pos_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, x, pos, T, C, total);
}

// --------------------------------------------------------------------------------------------------
// LayerNorm at C = 768 (layernorm_kernel of kernels_misc.hip holds C <= 512 in registers): one wavefront per token, three float4 per
// lane, two passes over the registers as there (mean, then the centred squares).
// --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) layernorm768_kernel(const float* __restrict__ x, int xld, float* __restrict__ y, int yld,
                                                           const float* __restrict__ gm, const float* __restrict__ bt, int M, float eps) {
    constexpr int C = 768;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + (size_t)row * xld;
    f32x4 v[3];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v[i] = *reinterpret_cast<const f32x4*>(xr + 256 * i + 4 * lane);
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
#pragma unroll
    for (int of = 32; of > 0; of >>= 1) s += __shfl_xor(s, of, 64);
    const float mean = s * (1.f / C);
    float qs = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v[i] -= mean;
        qs += (v[i][0] * v[i][0] + v[i][1] * v[i][1]) + (v[i][2] * v[i][2] + v[i][3] * v[i][3]);
    }
#pragma unroll
    for (int of = 32; of > 0; of >>= 1) qs += __shfl_xor(qs, of, 64);
    const float rstd = rsqrtf(qs * (1.f / C) + eps);
    float* yr = y + (size_t)row * yld;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(gm + 256 * i + 4 * lane);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(bt + 256 * i + 4 * lane);
        *reinterpret_cast<f32x4*>(yr + 256 * i + 4 * lane) = v[i] * rstd * gv + bv;
    }
}
void launch_layernorm768(const float* x, int xld, float* y, int yld, const float* g, const float* b, int M, float eps, hipStream_t s) {
    hipLaunchKernelGGL(layernorm768_kernel, dim3((M + 3) / 4), dim3(256), 0, s, x, xld, y, yld, g, b, M, eps);
}

}  // namespace rd
