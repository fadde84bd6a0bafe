// One PPLCNetV3 block (no SE, 3x3, stride 1) in one launch: depthwise layer -> pointwise layer, for the blocks at the recogniser's largest
// maps (blocks2.0, blocks3.0, blocks3.1: 24 x w2 pixels per line, cin 16 / 32 / 64, cout 32 / 64).  The depthwise output is never written:
//   a   = mid_s hardswish(dw3x3(x') + dw_b) + mid_b       x' = pre_act ? pre_s hardswish(x) + pre_b : x  (inside the map; padding = zeros)
//   acc = a W^T + pw_b                                     on the matrix cores
//   y   = out_act ? out_s hardswish(acc) + out_b : acc
// A workgroup of 4 waves owns a tile of 4 rows x 32 columns.  Phase 1: a thread computes 4 channels x 4 adjacent columns of `a` (the 6
// input columns of a kernel row are loaded once) and stores them into the LDS tile [128 pixels][CIN] - as the (hi, lo) fp16 pair of the
// split route, or as fp32.  Phase 2: wave r multiplies tile row r (32 pixels = the 32 rows of the A operand) with the weights, which it
// holds in registers as B operands for every tile it walks (grid-stride over tiles).  Split route: hi hi + (lo hi + hi lo) 2^-11 in two
// accumulators, v_mfma_f32_32x32x16_f16; fp32 route: v_mfma_f32_32x32x2_f32.  The arithmetic of an output pixel does not depend on its
// tile's neighbours, its image's index or the launch's size.
// Per-line widths: input columns >= line_w[n] are zero padding, rows of `a` at columns >= line_w[n] are zero (what the separate depthwise
// kernel writes there), so the output there is the pointwise bias as on the separate route.
// Range guard (split route): an input element or an element of `a` that is not a finite |v| <= 65504 raises the handle's flag.
#include "rd_device.h"

namespace rd {

namespace {

constexpr int LB_TH = 4, LB_TW = 32, LB_PIX = LB_TH * LB_TW;

template <int CIN, int COUT, bool SPLIT>
__global__ void __launch_bounds__(256) lcv3_block_kernel(Lcv3BlockParams p) {
    constexpr int NB = COUT / 32;                       // 32-wide blocks of output channels
    constexpr int LDH = CIN + 8;                        // halfs per pixel row of the split tiles: 16-byte reads, rows 16 bytes apart mod 128
    constexpr int LDF = CIN + 1;                        // floats per pixel row of the fp32 tile: odd, the column reads hit 32 banks
    constexpr int CQ = CIN / 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[SPLIT ? 2 * LB_PIX * LDH * 2 : LB_PIX * LDF * 4];
    _Float16* const ah = reinterpret_cast<_Float16*>(smem);
    _Float16* const al = ah + LB_PIX * LDH;
    float* const af = reinterpret_cast<float*>(smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l32 = lane & 31, lg = lane >> 5;

    // the pointwise weights as B operands, resident: column = output channel nb * 32 + l32
    f16x8 wh[SPLIT ? NB : 1][SPLIT ? CIN / 16 : 1], wl[SPLIT ? NB : 1][SPLIT ? CIN / 16 : 1];
    float wf[SPLIT ? 1 : NB][SPLIT ? 1 : CIN / 2];
    float pwb[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int co = nb * 32 + l32;
        pwb[nb] = p.pw_b[co];
        if constexpr (SPLIT) {
#pragma unroll
            for (int ks = 0; ks < CIN / 16; ++ks) {
                const float* src = p.pw_w + (size_t)co * CIN + ks * 16 + lg * 8;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    _Float16 h, l;
                    rd_split(src[e], h, l);
                    wh[nb][ks][e] = h;
                    wl[nb][ks][e] = l;
                }
            }
        } else {
#pragma unroll
            for (int s = 0; s < CIN / 2; ++s) wf[nb][s] = p.pw_w[(size_t)co * CIN + 2 * s + lg];
        }
    }

    const int tiles_w = (p.W + LB_TW - 1) / LB_TW, tiles_h = (p.H + LB_TH - 1) / LB_TH;
    const long ntiles = (long)p.N * tiles_h * tiles_w;
    bool bad = false;
#pragma unroll 1
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int tw = (int)(tile % tiles_w);
        const long tq = tile / tiles_w;
        const int th = (int)(tq % tiles_h), n = (int)(tq / tiles_h);
        const int lw = p.line_w ? min(p.line_w[n * p.line_stride], p.W) : p.W;

        // ---- phase 1: the depthwise layer into the LDS tile
#pragma unroll 1
        for (int item = tid; item < LB_TH * (LB_TW / 4) * CQ; item += 256) {
            const int c = (item % CQ) << 2;
            const int r = item / CQ;
            const int cg = r % (LB_TW / 4), row = r / (LB_TW / 4);
            const int oh = th * LB_TH + row, ow0 = tw * LB_TW + cg * 4;
            const f32x4 bias = *reinterpret_cast<const f32x4*>(p.dw_b + c);
            f32x4 acc[4] = {bias, bias, bias, bias};
            if (oh < p.H && ow0 < lw) {
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    const int ih = oh - 1 + kh;
                    if (ih < 0 || ih >= p.H) continue;
                    const float* xrow = p.x + ((size_t)n * p.H + ih) * p.W * p.xld + c;
                    f32x4 in[6];
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
                        const int iw = ow0 - 1 + i;
                        if (iw >= 0 && iw < lw) {
                            const f32x4 v = *reinterpret_cast<const f32x4*>(xrow + (size_t)iw * p.xld);
                            if constexpr (SPLIT) {
#pragma unroll
                                for (int e = 0; e < 4; ++e) bad |= !(fabsf(v[e]) <= 65504.f);
                            }
                            in[i] = p.pre_act ? lcv3_hswish_aff(v, p.pre_s, p.pre_b) : v;
                        } else {
                            in[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                        }
                    }
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const f32x4 wv = *reinterpret_cast<const f32x4*>(p.dw_w + (size_t)(kh * 3 + kw) * CIN + c);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(in[j + kw][e], wv[e], acc[j][e]);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in_map = oh < p.H && ow0 + j < lw;
                const f32x4 a = in_map ? lcv3_hswish_aff(acc[j], p.mid_s, p.mid_b) : f32x4{0.f, 0.f, 0.f, 0.f};
                const int pix = row * LB_TW + cg * 4 + j;
                if constexpr (SPLIT) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) bad |= !(fabsf(a[e]) <= 65504.f);
                    f16x4 h, l;
                    rd_split4(a, h, l);
                    *reinterpret_cast<f16x4*>(ah + pix * LDH + c) = h;
                    *reinterpret_cast<f16x4*>(al + pix * LDH + c) = l;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) af[pix * LDF + c + e] = a[e];
                }
            }
        }
        __syncthreads();

        // ---- phase 2: wave `wave` owns tile row `wave`: [32 pixels][CIN] x [CIN][COUT]
        const int oh = th * LB_TH + wave;
        if (oh < p.H) {                                  // (uniform per wave)
            const int pix = wave * LB_TW + l32;
            f32x16 out[NB];
            if constexpr (SPLIT) {
                f32x16 am[NB], ac[NB];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) am[nb][i] = ac[nb][i] = 0.f;
#pragma unroll
                for (int ks = 0; ks < CIN / 16; ++ks) {
                    const f16x8 xh = *reinterpret_cast<const f16x8*>(ah + pix * LDH + ks * 16 + lg * 8);
                    const f16x8 xl = *reinterpret_cast<const f16x8*>(al + pix * LDH + ks * 16 + lg * 8);
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        am[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wh[nb][ks], am[nb], 0, 0, 0);
                        ac[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, wh[nb][ks], ac[nb], 0, 0, 0);
                        ac[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wl[nb][ks], ac[nb], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) out[nb][i] = fmaf(ac[nb][i], 1.f / 2048.f, am[nb][i]);
            } else {
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) out[nb][i] = 0.f;
#pragma unroll
                for (int s = 0; s < CIN / 2; ++s) {
                    const float xv = af[pix * LDF + 2 * s + lg];
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) out[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv, wf[nb][s], out[nb], 0, 0, 0);
                }
            }
            // D element i of a lane: pixel row 8 (i / 4) + 4 (lane / 32) + i % 4, output channel lane % 32
            float* yrow = p.y + ((size_t)n * p.H + oh) * p.W * p.yld;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int ow = tw * LB_TW + 8 * (i >> 2) + 4 * lg + (i & 3);
                if (ow >= p.W) continue;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    float v = out[nb][i] + pwb[nb];
                    if (p.out_act) v = fmaf(v * fminf(fmaxf(v + 3.f, 0.f), 6.f) * (1.f / 6.f), p.out_s, p.out_b);
                    yrow[(size_t)ow * p.yld + nb * 32 + l32] = v;
                }
            }
        }
        __syncthreads();                                 // the next tile's phase 1 overwrites the LDS tile
    }
    if constexpr (SPLIT) {
        if (bad && p.range_flag) rd_raise_flag(p.range_flag);
    }
}

template <int CIN, int COUT>
void lb_launch(const Lcv3BlockParams& p, int grid, hipStream_t s) {
    if (p.split) hipLaunchKernelGGL((lcv3_block_kernel<CIN, COUT, true>), dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((lcv3_block_kernel<CIN, COUT, false>), dim3(grid), dim3(256), 0, s, p);
}

}  // namespace

bool lcv3_block_shape_ok(int cin, int cout) { return (cin == 16 && cout == 32) || (cin == 32 && cout == 64) || (cin == 64 && cout == 64); }

void launch_lcv3_block(const Lcv3BlockParams& p, hipStream_t s) {
    const long ntiles = (long)p.N * ((p.H + LB_TH - 1) / LB_TH) * ((p.W + LB_TW - 1) / LB_TW);
    const int grid = (int)(ntiles < 1 ? 1 : ntiles > 1024 ? 1024 : ntiles);       // 256 CUs x 4 resident workgroups; the rest by stride
    if (p.cin == 16 && p.cout == 32) lb_launch<16, 32>(p, grid, s);
    else if (p.cin == 32 && p.cout == 64) lb_launch<32, 64>(p, grid, s);
    else if (p.cin == 64 && p.cout == 64) lb_launch<64, 64>(p, grid, s);
}

}  // namespace rd
