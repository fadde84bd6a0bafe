// 1x3 sequence convolution over token rows (the SVTR neck's conv1 / conv4 of the PP-OCRv5 server recogniser) as a GEMM with
// K = 3 taps x Cin on the fp16 matrix cores with (hi, lo) split operands - arithmetic as in kernels_conv_h3.hip / kernels_gemm_h1.hip:
// x = hi + lo 2^-11, products hi.hi into one fp32 accumulator and hi.lo + lo.hi into a second, fp32 accumulate, range flag for operands
// outside the fp16 range (the caller re-runs in fp32) - and a native fp32-MFMA instance of the same loop for RD_PRECISION=fp32.
//
//   Y[m][n] = act( sum_{d in -1,0,+1} sum_c X[m + d][c] W[n][(d + 1) Cin + c] + bias[n] ),   X[m + d] = 0 where m + d leaves m's LINE
//
// * Token rows of many text lines lie one behind the other ("ragged token buffer"): tokinfo[m] = position in the line | tokens of the
//   line << 16 says where a row's line begins and ends.  The uniform form ([B][T] rows) derives the same two numbers from m and T;
//   from there on both forms are one code path.
// * Two K segments from two sources: Cin = C0 + C1, channels [0, C0) come from x0, [C0, Cin) from x1 - the neck's cat(backbone tokens,
//   conv3 output) is never written.
// * A wavefront owns 64 token rows x 64 output channels (2 x 2 MFMA 32x32 blocks, one accumulator pair each); the four wavefronts of a
//   workgroup share the rows and split 256 output channels.  Both operands stream from global memory (A: fp32 rows, split in registers,
//   the four wavefronts' reads of the same rows hit in L1; B: the pre-split weight planes, 12.6 MB for conv4, L2 / MALL resident), the
//   loads of step s + 1 are requested before the MFMAs of step s, and there is no LDS and no barrier: the layer is 2/3 of the tail's
//   arithmetic but ~3 % of the network's, so the kernel is kept simple rather than tiled through LDS.
// * Every output element is the sum of its own row's products in one fixed k order (tap, segment, channel): a token's bits do not
//   depend on what else is in the launch.
#include "rd_device.h"

namespace rd {

template <bool SPLIT>
__global__ void __launch_bounds__(256) seqconv_kernel(SeqConvParams p) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lhi = lane >> 5;
    const int n0 = (blockIdx.y * 4 + wave) * 64;
    if (n0 >= p.N) return;                      // (no barrier in this kernel)
    const int Cin = p.C0 + p.C1, K = 3 * Cin;
    const int S0 = p.C0 >> 4, SPT = Cin >> 4;   // 16-channel steps of segment 0 / of one tap
    const int nsteps = 3 * SPT;
    const int ldb = SPLIT ? ((K + 31) & ~31) : K;   // weight row stride: split_weights_h3 pads the planes' rows to 32
    const long m0 = (long)blockIdx.x * 64;

    // ---- this lane's two A rows: the line they belong to decides which taps exist
    long row[2];
    unsigned vmask[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        const long m = m0 + mb * 32 + l31;
        const long mm = m < p.M ? m : (long)p.M - 1;
        int pos, len;
        if (p.tokinfo) {
            const unsigned ti = (unsigned)p.tokinfo[mm];
            pos = (int)(ti & 0xffffu);
            len = (int)(ti >> 16);
        } else {
            pos = (int)(mm % p.T);
            len = p.T;
        }
        row[mb] = mm;
        vmask[mb] = ((pos > 0 && mm > 0) ? 1u : 0u) | 2u | ((pos + 1 < len && mm + 1 < p.M) ? 4u : 0u);
    }

    f32x16 acc1[2][2], acc2[2][2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc1[mb][nb][r] = acc2[mb][nb][r] = 0.f;

    // One step = 16 k values of one tap and segment: lane (l31, lhi) holds k = 8 lhi .. 8 lhi + 7 of its row (A) / output channel (B).
    // The loads are unconditional (a missing tap re-reads the row itself) and masked afterwards.
    struct Regs {
        f32x4 a[2][2];
        u32x4 bh[2], bl[2];      // SPLIT: 8 halfs of the hi / lo plane;  fp32: bh / bl = the 8 floats
    };
    auto load = [&](int st, Regs& g, unsigned& ok0, unsigned& ok1) {
        const int tap = st / SPT, r = st - tap * SPT;
        const bool seg1 = r >= S0;
        const int c = (seg1 ? r - S0 : r) * 16 + 8 * lhi;
        const float* xb = seg1 ? p.x1 : p.x0;
        const int ld = seg1 ? p.ld1 : p.ld0;
        const unsigned bit = 1u << tap;
        ok0 = vmask[0] & bit;
        ok1 = vmask[1] & bit;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const long rr = row[mb] + ((vmask[mb] & bit) ? tap - 1 : 0);
            const float* xp = xb + (size_t)rr * ld + c;
            g.a[mb][0] = *reinterpret_cast<const f32x4*>(xp);
            g.a[mb][1] = *reinterpret_cast<const f32x4*>(xp + 4);
        }
        const size_t kk = (size_t)tap * Cin + (seg1 ? p.C0 : 0) + c;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const size_t o = (size_t)(n0 + nb * 32 + l31) * ldb + kk;
            if (SPLIT) {
                g.bh[nb] = *reinterpret_cast<const u32x4*>(p.wh + o);
                g.bl[nb] = *reinterpret_cast<const u32x4*>(p.wl + o);
            } else {
                g.bh[nb] = *reinterpret_cast<const u32x4*>(p.w + o);
                g.bl[nb] = *reinterpret_cast<const u32x4*>(p.w + o + 4);
            }
        }
    };

    float amax = 0.f;
    Regs cur, nxt;
    unsigned ok[2], okn[2];
    load(0, cur, ok[0], ok[1]);
    for (int st = 0; st < nsteps; ++st) {
        if (st + 1 < nsteps) load(st + 1, nxt, okn[0], okn[1]);
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const f32x4 c0 = ok[mb] ? cur.a[mb][0] : z, c1 = ok[mb] ? cur.a[mb][1] : z;
            if (SPLIT) {
#pragma unroll
                for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fmaxf(fabsf(c0[e]), fabsf(c1[e])));
                f16x4 h0, l0, h1, l1;
                rd_split4(c0, h0, l0);
                rd_split4(c1, h1, l1);
                const f16x8 ah = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
                const f16x8 al = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const f16x8 bh = __builtin_bit_cast(f16x8, cur.bh[nb]);
                    const f16x8 bl = __builtin_bit_cast(f16x8, cur.bl[nb]);
                    acc1[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc1[mb][nb], 0, 0, 0);
                    acc2[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc2[mb][nb], 0, 0, 0);
                    acc2[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc2[mb][nb], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const f32x4 b0 = __builtin_bit_cast(f32x4, cur.bh[nb]), b1 = __builtin_bit_cast(f32x4, cur.bl[nb]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc1[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(c0[e], b0[e], acc1[mb][nb], 0, 0, 0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc1[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(c1[e], b1[e], acc1[mb][nb], 0, 0, 0);
                }
            }
        }
        cur = nxt;
        ok[0] = okn[0];
        ok[1] = okn[1];
    }

    // ---- epilogue: lane = output channel, registers = 16 of the block's 32 rows
    unsigned emax = 0;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int n = n0 + nb * 32 + l31;
        const float bv = p.bias ? p.bias[n] : 0.f;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const long mbase = m0 + mb * 32 + 4 * lhi;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float o = (SPLIT ? fmaf(acc2[mb][nb][r], 1.f / 2048.f, acc1[mb][nb][r]) : acc1[mb][nb][r]) + bv;
                emax = max(emax, __float_as_uint(o) & 0x7fffffffu);
                o = rd_act(o, p.act);
                const long mo = mbase + (r & 3) + 8 * (r >> 2);
                if (mo < p.M) p.y[(size_t)mo * p.yld + n] = o;
            }
        }
    }
    if (SPLIT && (emax >= 0x7f800000u || !(amax < 65504.f)) && p.range_flag) rd_raise_flag(p.range_flag);
}

bool seqconv_shape_ok(int C0, int C1, int N) { return C0 >= 16 && C0 % 16 == 0 && C1 >= 0 && C1 % 16 == 0 && N >= 64 && N % 64 == 0; }

void launch_seqconv(const SeqConvParams& p, hipStream_t s) {
    if (p.M <= 0 || !seqconv_shape_ok(p.C0, p.C1, p.N)) return;
    const dim3 grid((unsigned)((p.M + 63) / 64), (unsigned)((p.N + 255) / 256)), block(256);
    if (p.wh && p.wl) hipLaunchKernelGGL(seqconv_kernel<true>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(seqconv_kernel<false>, grid, block, 0, s, p);
}

}  // namespace rd
