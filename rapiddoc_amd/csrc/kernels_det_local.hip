// Fused local tail of PFHeadLocal (the PP-OCRv5 server detector's head, det_db_head.py:152-180), one kernel per forward:
//
//   maps[y][x] = 0.5 * (shrink[y][x] + sigmoid(b1 + sum_co w1[co] * relu(b3[co] + sum_{dy, dx} ( W3[co][0][dy][dx] * shrink[y + dy][x + dx]
//                                                                        + sum_ci W3[co][1 + ci][dy][dx] * f[(y + dy) >> 1][(x + dx) >> 1][ci] ))))
//
// i.e. last_3 (3x3 over cat[shrink, nearest-2x(f)], 65 -> 64, BN folded, ReLU), last_1 (1x1 to one channel), sigmoid and the mean with the
// shrink map.  It reads f [N][H/2][W/2][64] and shrink [N][H][W] and writes maps [N][H][W]: neither the 65-channel concat nor the
// 64-channel hidden tensor at full resolution exists anywhere (about 350 MB per 960 x 704 page as separate operators).
//
// * The 64 f channels are a nearest-neighbour 2x upsample, so the three rows (columns) of the 3x3 only ever meet TWO rows (columns) of f:
//   for an even output row y = 2Y the taps y - 1, y, y + 1 read f rows Y - 1, Y, Y, for an odd one Y, Y, Y + 1 (H and W are even, so the
//   zero padding of the full-resolution map coincides with the border of f).  Per output parity (py, px) the 3x3 over up2(f) is therefore a
//   2x2 convolution over f with summed weights (prepare_det_local_weights): K = 4 x 64 instead of 9 x 64, the same sum of products in exact
//   arithmetic.  The nine shrink taps ride along as one more 16-wide k-step: K = 272.
// * Matrix cores: D[co][pixel] = W[co][k] X[k][pixel].  A wavefront owns ONE parity class of a tile of 4 x 32 f pixels (4 blocks of 32
//   output pixels x 64 output channels, 128 accumulator registers), the four wavefronts of a workgroup the four classes.  With the output
//   channels in the ROWS of the accumulator a lane holds 32 of the 64 channels of its pixel: the 1x1 is an in-lane dot product plus one
//   exchange with lane ^ 32.
// * Split route: the one-accumulator arithmetic of kernels_conv3x3_h1.hip (x = hi + lo unscaled, weights pre-scaled by a power of two,
//   hi.hi + hi.lo + lo.hi into one fp32 accumulator, range flag).  fp32 route: the same loop on v_mfma_f32_32x32x2_f32.
// * Operands stream from global memory through L1 (f: every value is read by 4 taps x 4 parities of one workgroup; weights: fragment-ordered
//   images of 17 - 35 KB per parity, L2 resident), loads of step s + 1 requested before the MFMAs of step s; no LDS, no barrier.
// * A pixel's value is the sum of its own products in one fixed k order: it does not depend on the launch it rides in.
#include <cmath>
#include <vector>

#include "rd_device.h"

namespace rd {

static constexpr int DL_C = 64;                  // f channels = hidden channels
static constexpr int DL_STEPS = 17;              // 16 k-steps of f (4 taps x 4 x 16 channels) + 1 of shrink taps
static constexpr int DL_PB = 4;                  // f rows (pixel blocks) per wavefront
static constexpr int DL_TW = 32;                 // f columns per tile

typedef _Float16 dl_f16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void dl_split8(const f32x4 v0, const f32x4 v1, float neg1, f16x8& hi, f16x8& lo) {
    const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        const dl_f16x2 h = __builtin_convertvector(f32x2{v[e], v[e + 1]}, dl_f16x2);
        hi[e] = h[0];
        hi[e + 1] = h[1];
        lo[e] = (_Float16)__builtin_fmaf((float)h[0], neg1, v[e]);
        lo[e + 1] = (_Float16)__builtin_fmaf((float)h[1], neg1, v[e + 1]);
    }
}

template <bool SPLIT>
__global__ void __launch_bounds__(256) det_local_kernel(DetLocalParams p, int tiles_y, int tiles_x) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lhi = lane >> 5;
    const int py = wave >> 1, px = wave & 1;
    const int FH = p.H >> 1, FW = p.W >> 1;
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y;
    const int n = t / tiles_y;
    const int fx = tx * DL_TW + l31, fy0 = ty * DL_PB;
    float neg1 = -1.f;
    asm volatile("" : "+s"(neg1));

    const float* fimg = p.f + (size_t)n * FH * FW * p.fld;
    const float* simg = p.shrink + (size_t)n * p.H * p.W;
    // weight image of this parity: [step][channel block][plane][lane][8]
    const size_t wpar = (size_t)wave * DL_STEPS * 2;          // in fragments (SPLIT: of two planes)

    struct Regs {
        f32x4 x[DL_PB][2];
        u32x4 w[2][2];       // SPLIT: [channel block][hi | lo] 8 halfs;  fp32: [channel block][first | second four floats]
    };
    auto load_w = [&](int s, Regs& g) {
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const size_t frag = wpar + (size_t)s * 2 + cb;
            if (SPLIT) {
                const uint16_t* q = p.wimg16 + frag * 1024 + lane * 8;
                g.w[cb][0] = *reinterpret_cast<const u32x4*>(q);
                g.w[cb][1] = *reinterpret_cast<const u32x4*>(q + 512);
            } else {
                const float* q = p.wimg32 + frag * 512 + lane * 8;
                g.w[cb][0] = *reinterpret_cast<const u32x4*>(q);
                g.w[cb][1] = *reinterpret_cast<const u32x4*>(q + 4);
            }
        }
    };
    // ok: bit pb = this step's f pixel of block pb lies inside the map (else it is the convolution's zero padding)
    auto load = [&](int s, Regs& g, unsigned& ok) {
        const int tap = s >> 2, a = tap >> 1, b = tap & 1;
        const int c0 = (s & 3) * 16 + 8 * lhi;
        const int xx = fx + b - 1 + px;
        const bool xin = (unsigned)xx < (unsigned)FW;
        const int xc = min(max(xx, 0), FW - 1);
        ok = 0;
#pragma unroll
        for (int pb = 0; pb < DL_PB; ++pb) {
            const int yy = fy0 + pb + a - 1 + py;
            if (xin && (unsigned)yy < (unsigned)FH) ok |= 1u << pb;
            const int yc = min(max(yy, 0), FH - 1);
            const float* xp = fimg + ((size_t)yc * FW + xc) * p.fld + c0;
            g.x[pb][0] = *reinterpret_cast<const f32x4*>(xp);
            g.x[pb][1] = *reinterpret_cast<const f32x4*>(xp + 4);
        }
        load_w(s, g);
    };
    // the shrink step: k = 8 lhi + e is tap (k / 3 - 1, k % 3 - 1) of the full-resolution shrink map for k < 9, zero beyond
    auto load_shrink = [&](Regs& g) {
        const int X = 2 * fx + px;
#pragma unroll
        for (int pb = 0; pb < DL_PB; ++pb) {
            const int Y = 2 * (fy0 + pb) + py;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = 8 * lhi + e;
                const int dy = k / 3 - 1, dx = k % 3 - 1;
                const int yy = Y + dy, xx = X + dx;
                const bool in = k < 9 && (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W;
                const float sv = simg[(size_t)min(max(yy, 0), p.H - 1) * p.W + min(max(xx, 0), p.W - 1)];
                v[e] = in ? sv : 0.f;
            }
            g.x[pb][0] = f32x4{v[0], v[1], v[2], v[3]};
            g.x[pb][1] = f32x4{v[4], v[5], v[6], v[7]};
        }
        load_w(DL_STEPS - 1, g);
    };

    f32x16 acc[2][DL_PB];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int pb = 0; pb < DL_PB; ++pb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][pb][r] = 0.f;

    float amax = 0.f;
    auto compute = [&](const Regs& g, unsigned ok) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int pb = 0; pb < DL_PB; ++pb) {
            const bool in = (ok >> pb) & 1u;
            const f32x4 x0 = in ? g.x[pb][0] : z, x1 = in ? g.x[pb][1] : z;
            if (SPLIT) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    amax = (x0[e] != x0[e] || x1[e] != x1[e]) ? INFINITY : fmaxf(amax, fmaxf(fabsf(x0[e]), fabsf(x1[e])));
                }
                f16x8 xh, xl;
                dl_split8(x0, x1, neg1, xh, xl);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const f16x8 wh = __builtin_bit_cast(f16x8, g.w[cb][0]);
                    const f16x8 wl = __builtin_bit_cast(f16x8, g.w[cb][1]);
                    acc[cb][pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xh, acc[cb][pb], 0, 0, 0);
                    acc[cb][pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, xh, acc[cb][pb], 0, 0, 0);
                    acc[cb][pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xl, acc[cb][pb], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const f32x4 w0 = __builtin_bit_cast(f32x4, g.w[cb][0]), w1 = __builtin_bit_cast(f32x4, g.w[cb][1]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[cb][pb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[e], x0[e], acc[cb][pb], 0, 0, 0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[cb][pb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[e], x1[e], acc[cb][pb], 0, 0, 0);
                }
            }
        }
    };

    Regs cur, nxt;
    unsigned ok, okn;
    load(0, cur, ok);
#pragma unroll 1
    for (int s = 0; s < DL_STEPS - 1; ++s) {
        if (s + 1 < DL_STEPS - 1) load(s + 1, nxt, okn);
        else { load_shrink(nxt); okn = (1u << DL_PB) - 1u; }
        compute(cur, ok);
        cur = nxt;
        ok = okn;
    }
    compute(cur, ok);

    // ---- epilogue: lane = pixel (l31), registers = 16 of a channel block's 32 hidden channels (4 lhi + (r & 3) + 8 (r >> 2))
    unsigned emax = 0;
    float part[DL_PB];
#pragma unroll
    for (int pb = 0; pb < DL_PB; ++pb) part[pb] = 0.f;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = cb * 32 + 4 * lhi + (r & 3) + 8 * (r >> 2);
            const float bv = p.b3[co], wv = p.w1[co];
#pragma unroll
            for (int pb = 0; pb < DL_PB; ++pb) {
                const float h = SPLIT ? fmaf(acc[cb][pb][r], p.w_inv, bv) : acc[cb][pb][r] + bv;
                emax = max(emax, __float_as_uint(h) & 0x7fffffffu);
                part[pb] = fmaf(fmaxf(h, 0.f), wv, part[pb]);
            }
        }
#pragma unroll
    for (int pb = 0; pb < DL_PB; ++pb) {
        const float tot = part[pb] + __shfl_xor(part[pb], 32);
        const int fy = fy0 + pb;
        if (lhi == 0 && fx < FW && fy < FH) {
            const size_t o = (size_t)(2 * fy + py) * p.W + (2 * fx + px);
            const float sv = simg[o];
            p.y[(size_t)n * p.H * p.W + o] = 0.5f * (sv + rd_act(tot + p.b1, ACT_SIGMOID));
        }
    }
    if (SPLIT && (emax >= 0x7f800000u || !(amax < 65504.f)) && p.range_flag) rd_raise_flag(p.range_flag);
}

void launch_det_local(const DetLocalParams& p, hipStream_t s) {
    if (p.N <= 0 || p.H <= 0 || p.W <= 0) return;
    const int FH = p.H / 2, FW = p.W / 2;
    const int tiles_y = (FH + DL_PB - 1) / DL_PB, tiles_x = (FW + DL_TW - 1) / DL_TW;
    const dim3 grid((unsigned)((size_t)p.N * tiles_y * tiles_x)), block(256);
    if (p.wimg16) hipLaunchKernelGGL(det_local_kernel<true>, grid, block, 0, s, p, tiles_y, tiles_x);
    else hipLaunchKernelGGL(det_local_kernel<false>, grid, block, 0, s, p, tiles_y, tiles_x);
}

// Host: w3 = last_3's folded weights in the state dict's order [64][65][3][3] (input channel 0 = the shrink map, 1 .. 64 = f).
// Builds, per output parity (py, px), the matrix [64][272]: k = (a * 2 + b) * 64 + ci for the 2x2 over f (row Y + a - 1 + py, column
// X + b - 1 + px; the 3x3's rows dy that fall on the same f row are summed, in double), k = 256 + t the nine shrink taps, zeros beyond -
// and from it the two fragment-ordered images: img32 [parity][step][block][lane][8] fp32, img16 the same with (hi, lo) fp16 planes of the
// weights scaled by 2^ex (max |w| in [2^13, 2^14)); returns 2^-ex.
float prepare_det_local_weights(const float* w3, std::vector<float>& img32, std::vector<uint16_t>& img16) {
    const int KP = 16 * DL_STEPS;
    std::vector<float> m((size_t)4 * DL_C * KP, 0.f);
    // which 2x2 tap a 3x3 offset d = -1, 0, 1 lands on: even parity: (y - 1) >> 1 = Y - 1 (a = 0), y >> 1 = (y + 1) >> 1 = Y (a = 1);
    // odd parity: (y - 1) >> 1 = y >> 1 = Y (a = 0), (y + 1) >> 1 = Y + 1 (a = 1)
    auto tap_of = [](int par, int d) { return par == 0 ? (d < 0 ? 0 : 1) : (d > 0 ? 1 : 0); };
    for (int par = 0; par < 4; ++par) {
        const int py = par >> 1, px = par & 1;
        for (int co = 0; co < DL_C; ++co) {
            float* row = m.data() + ((size_t)par * DL_C + co) * KP;
            for (int ci = 0; ci < DL_C; ++ci) {
                double sum[4] = {0, 0, 0, 0};
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx)
                        sum[tap_of(py, dy) * 2 + tap_of(px, dx)] += (double)w3[(((size_t)co * 65 + 1 + ci) * 3 + dy + 1) * 3 + dx + 1];
                for (int tp = 0; tp < 4; ++tp) row[tp * DL_C + ci] = (float)sum[tp];
            }
            for (int tp = 0; tp < 9; ++tp) row[4 * DL_C + tp] = w3[((size_t)co * 65) * 9 + tp];
        }
    }
    const int ex = rd_pow2_exp(m.data(), m.size(), RD_EXP_CLAMP);
    const size_t nfrag = (size_t)4 * DL_STEPS * 2;
    img32.assign(nfrag * 512, 0.f);
    img16.assign(nfrag * 1024, 0);
    for (int par = 0; par < 4; ++par)
        for (int s = 0; s < DL_STEPS; ++s)
            for (int cb = 0; cb < 2; ++cb)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const int co = cb * 32 + (lane & 31), k = s * 16 + 8 * (lane >> 5) + e;
                        const float v = m[((size_t)par * DL_C + co) * KP + k];
                        const size_t frag = ((size_t)par * DL_STEPS + s) * 2 + cb;
                        img32[frag * 512 + (size_t)lane * 8 + e] = v;
                        rd_split_scaled(v, ex, img16[frag * 1024 + (size_t)lane * 8 + e], img16[frag * 1024 + 512 + (size_t)lane * 8 + e]);
                    }
    return std::ldexp(1.f, -ex);
}

}  // namespace rd
