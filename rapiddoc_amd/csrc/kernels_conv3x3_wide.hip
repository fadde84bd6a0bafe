// Direct 3x3 / stride-1 / pad-1 convolution to 128 .. 256 output channels on the fp16 matrix cores with ONE fp32 accumulator set -
// the HG_Block layers of PPHGNet_small (PP-OCRv4 server detector / recogniser, rec_hgnet.py:55-110): 128, 160, 192 or 224 output
// channels from 64 .. 768 input channels.  The arithmetic, the patch and the weight stream are those of conv3x3_h1_kernel
// (kernels_conv3x3_h1.hip, read its header first): x = hi + lo unscaled, the weights pre-scaled per matrix by a power of two, the three
// products hi.hi + hi.lo + lo.hi into one accumulator, the exact inverse scale in the epilogue.  What is new is how a tile's output
// channels are spread, so that the input patch is staged and split ONCE for all of them:
//   * a workgroup is EIGHT wavefronts on an 8 x 32 tile: wavefront (rp, ch) = (wave & 3, wave >> 2) owns the two pixel rows 2 rp, 2 rp + 1
//     and the channel half ch, NBH = ceil(ceil(Cout / 32) / 2) blocks of 32 channels: 2 x NBH x 16 = 64 / 96 / 128 accumulator
//     registers (NBH = 2 / 3 / 4).  The four wavefronts of a channel half read the same weight fragments, the two of a row pair the
//     same pixel fragments: 4 + 2 NBH ds_read_b128 per 6 NBH MFMAs (8 per 12, 10 per 18, 12 per 24);
//   * an odd block count (Cout = 160, 224) is padded to the even one with zero weights: the upper half computes one block whose
//     stores are dropped (5 -> 6 and 7 -> 8 blocks: 20 % / 14 % more MFMAs for those two widths; 128 and 192 pay nothing);
//   * LDS: the two patch planes of the sibling (2 x 27 200 bytes, 32 input channels per pass) + a ring of FOUR weight slabs of
//     4 NBH KB (one k-step: 2 NBH blocks x {hi, lo} fragments of 1 KB): 87 168 / 103 552 / 119 936 bytes of the CU's 160 KB - ONE
//     workgroup per CU (__launch_bounds__(512): two wavefronts per SIMD, 256 registers each).  While one wavefront of a SIMD waits at a
//     step's barrier the other one's MFMAs run; the patch staging of a pass (43.5 KB of loads per 18 steps of 6 NBH MFMAs) is exposed -
//     which is what the sibling's two independent workgroups per CU hide, and why two launches of the sibling over <= 96 channels
//     still measure 1.05 - 1.33 x this kernel on the 160- and 192-channel layers (docs/notebook/v4_server.md: the PPHGNet_small builder
//     routes those layers there, and the 224-channel layers of the 1/32 maps to the generic route);
//   * a slab is filled by linear `global_load_lds` copies three steps ahead: 4 NBH pieces of 1 KB, wavefront w issues pieces w and
//     (where there is one) w + 8.
// Registers (hipcc -O3 for gfx950, -Rpass-analysis=kernel-resource-usage): 114 / 162 / 201 VGPRs for NBH = 2 / 3 / 4, no AGPRs, no
// scratch and no VGPR spill in any of the three instantiations.
// Image bases are 64-bit; offsets inside an image are 32-bit byte offsets through a buffer descriptor, so conv3x3_wide_applies refuses
// a layer whose image (H x W x xld floats) reaches 2^31 bytes, and the layer takes the generic route.  Results depend on the layer
// alone: one kernel for every N, persistent workgroups over the tiles, a fixed product order.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "rd_device.h"

namespace rd {

static constexpr int CW_TR = 8, CW_TC = 32;                   // output tile (rows x columns)
static constexpr int CW_PW = CW_TC + 2, CW_PH = CW_TR + 2;    // patch
static constexpr int CW_PP = CW_PW * CW_PH;                   // 340 patch pixels
static constexpr int CW_CC = 32;                              // input channels per pass
static constexpr int CW_S = CW_CC * 2 + 16;                   // bytes per patch pixel in one fp16 plane (80 = 16 x odd)
static constexpr int CW_PLANE = CW_PP * CW_S;                 // 27 200 bytes
static constexpr int CW_D = 4;                                // weight slabs in the ring
static constexpr int CW_NT = 512;                             // threads

typedef _Float16 cw_f16x2 __attribute__((ext_vector_type(2)));
// x = hi + lo, hi = fp16(x), lo = fp16(x - hi) (c3_split4 of the sibling)
__device__ __forceinline__ void cw_split4(const f32x4 v, float neg1, f16x4& hi, f16x4& lo) {
#pragma unroll
    for (int e = 0; e < 4; e += 2) {
        const cw_f16x2 h = __builtin_convertvector(f32x2{v[e], v[e + 1]}, cw_f16x2);
        hi[e] = h[0];
        hi[e + 1] = h[1];
        lo[e] = (_Float16)__builtin_fmaf((float)h[0], neg1, v[e]);
        lo[e + 1] = (_Float16)__builtin_fmaf((float)h[1], neg1, v[e + 1]);
    }
}

template <int NBH>
struct CwFrag { f16x8 ah[2], al[2], bh[NBH], bl[NBH]; };

// "my pieces of the slab about to be read have landed", then the workgroup barrier (c3_wait_slab_barrier of the sibling, whose comment
// gives the argument): a wavefront issues one or two DMA instructions per slab, CW_D - 2 younger slabs may still be in flight.
template <int NBH>
__device__ __forceinline__ void cw_wait_slab_barrier(int wave) {
    constexpr int NF = 4 * NBH;                             // 1-KB pieces of a slab
    if (wave + 8 < NF) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(2)\n\ts_barrier" ::: "memory");
}

template <int NBH>
__global__ void __launch_bounds__(CW_NT) conv3x3_wide_kernel(ConvParams p, int tiles_r, int tiles_c, int ntiles, int nstep) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NF = 4 * NBH;
    constexpr int SLAB = NF * 1024;                         // bytes of one weight slab
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rp = wave & 3, ch = wave >> 2;
    const int l31 = lane & 31, lhi = lane >> 5;
    unsigned char* Ph = smem;
    unsigned char* Pl = smem + CW_PLANE;
    unsigned char* Wb = smem + 2 * CW_PLANE;
    const _Float16* wimg = reinterpret_cast<const _Float16*>(p.w3w);
    float neg1 = -1.f;
    asm volatile("" : "+s"(neg1));

    // ---- weight stream: slab j of the global step sequence = slab (j mod nstep) of the image -> ring buffer j mod CW_D
    int w_issue = 0, w_pos = 0;
    auto dma_slab = [&]() {
        const _Float16* src = wimg + (size_t)w_pos * (SLAB / 2) + lane * 8;
        unsigned char* dst = Wb + (unsigned)(w_issue & (CW_D - 1)) * SLAB;
        auto piece = [&](int f) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + f * 512),
                                             (__attribute__((address_space(3))) void*)(dst + f * 1024), 16, 0, 0);
        };
        piece(wave);
        if (wave + 8 < NF) piece(wave + 8);
        ++w_issue;
        if (++w_pos == nstep) w_pos = 0;
    };

    // ---- patch staging: 10 rows x 34 columns x 8 channel groups (of 4) = 2720 slots; thread t owns slots t, t + 512, ... (six, the
    // last one only for t < 160).  A row has 272 slots, a multiple of 8: the channel group of every slot of a thread is t & 7.
    constexpr int NSLOT = 6, ROWSLOTS = CW_PW * 8;
    int stid = tid;
    auto slot_row = [&](int i) { return (stid + CW_NT * i) / ROWSLOTS; };
    auto slot_col = [&](int i) { return ((stid + CW_NT * i) % ROWSLOTS) >> 3; };
    float amax = 0.f;
    int img = 0, oh0 = 0, ow0 = 0;
    u32x4 pre[NSLOT];
    unsigned pre_ok = 0;
    auto load_patch = [&](int im, int oh, int ow, int c0, int groups) {
        // 32-bit byte offsets inside the image through a buffer descriptor (conv3x3_wide_applies: an image is < 2^31 bytes)
        typedef __amdgpu_buffer_rsrc_t rsrc_t;
        const rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x + (size_t)im * p.H * p.W * p.xld + c0), 0, 0x7fffffff, 0x00020000);
        stid = tid;
        asm volatile("" : "+v"(stid));                      // (the slots' rows / columns are decoded here, not hoisted through the MFMA steps)
        const int s_grp = stid & 7;
        const unsigned gsel = s_grp < groups ? 16u * (unsigned)s_grp : 0u;
        pre_ok = 0;
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) {
            const int pr = min(slot_row(i), CW_PH - 1);     // (the sixth slot of t >= 160 lies behind the patch: loaded clamped, never written)
            const int ih = oh - 1 + pr, iw = ow - 1 + slot_col(i);
            if ((unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W) pre_ok |= 1u << i;
            const unsigned off = ((unsigned)min(max(ih, 0), p.H - 1) * (unsigned)p.W + (unsigned)min(max(iw, 0), p.W - 1)) * (unsigned)p.xld * 4u + gsel;
            pre[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)off, 0, 0);
        }
    };
    auto write_patch = [&](int groups) {
        stid = tid;
        asm volatile("" : "+v"(stid));
        const int s_grp = stid & 7;
        if (s_grp >= groups) return;
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) {
            if (i + 1 == NSLOT && stid + CW_NT * (NSLOT - 1) >= CW_PH * ROWSLOTS) continue;
            const f32x4 x4 = (pre_ok >> i) & 1u ? __builtin_bit_cast(f32x4, pre[i]) : f32x4{0.f, 0.f, 0.f, 0.f};
            f16x4 hi, lo;
            cw_split4(x4, neg1, hi, lo);
#pragma unroll
            for (int e = 0; e < 4; ++e) amax = (x4[e] != x4[e]) ? INFINITY : fmaxf(amax, fabsf(x4[e]));
            const unsigned o = (unsigned)(slot_row(i) * CW_PW + slot_col(i)) * CW_S + (unsigned)s_grp * 8;
            *reinterpret_cast<f16x4*>(Ph + o) = hi;
            *reinterpret_cast<f16x4*>(Pl + o) = lo;
        }
    };

    // ---- fragments of one step: A = this wavefront's two pixel rows at tap (kh, kw), k-step ks of the pass; B = its channel half's fragments
    const unsigned a_lane = (unsigned)((2 * rp) * CW_PW + l31) * CW_S + (unsigned)lhi * 16u;
    const unsigned b_lane = (unsigned)lane * 16u + (unsigned)(ch * NBH) * 2048u;
    auto read_frag = [&](CwFrag<NBH>& f, int tap, int ks, int slab) {
        const int kh = tap / 3, kw = tap - 3 * kh;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const unsigned a = a_lane + (unsigned)((r + kh) * CW_PW + kw) * CW_S + (unsigned)ks * 32u;
            f.ah[r] = *reinterpret_cast<const f16x8*>(Ph + a);
            f.al[r] = *reinterpret_cast<const f16x8*>(Pl + a);
        }
        const unsigned char* wb = Wb + (unsigned)(slab & (CW_D - 1)) * SLAB + b_lane;
#pragma unroll
        for (int nb = 0; nb < NBH; ++nb) {
            f.bh[nb] = *reinterpret_cast<const f16x8*>(wb + (2 * nb) * 1024);
            f.bl[nb] = *reinterpret_cast<const f16x8*>(wb + (2 * nb + 1) * 1024);
        }
    };

    f32x16 acc[2][NBH];
    CwFrag<NBH> fr[2];
    int g = 0;                                              // global step counter (slab index of the step being computed)
    auto run_pass = [&](auto ksn_c) {
        constexpr int KSN = decltype(ksn_c)::value;
        constexpr int NS = 9 * KSN;
        read_frag(fr[0], 0, 0, g);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            // slab g + 1 (read below) has landed everywhere, and every wavefront has read its fragments of slab g: its buffer is free
            cw_wait_slab_barrier<NBH>(wave);
            dma_slab();                                     // slab g + CW_D -> the buffer of slab g
            CwFrag<NBH>& cur = fr[s & 1];
            if (s + 1 < NS) read_frag(fr[(s + 1) & 1], (s + 1) / KSN, (s + 1) % KSN, g + 1);
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int nb = 0; nb < NBH; ++nb) acc[r][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.ah[r], cur.bh[nb], acc[r][nb], 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int nb = 0; nb < NBH; ++nb) acc[r][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.ah[r], cur.bl[nb], acc[r][nb], 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int nb = 0; nb < NBH; ++nb) acc[r][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.al[r], cur.bh[nb], acc[r][nb], 0, 0, 0);
            ++g;
        }
    };

    const int full_passes = p.Cin / CW_CC, tail16 = (p.Cin % CW_CC) / 16;
    auto decode = [&](int v, int& im, int& oh, int& ow) {
        // XCD-contiguous tile order (workgroup b sits on XCD b % 8), as the sibling
        const int xcd = v & 7, jj = v >> 3, q = ntiles >> 3, rm = ntiles & 7;
        int t = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + jj;
        const int tc = t % tiles_c;
        t /= tiles_c;
        const int tr = t % tiles_r;
        im = t / tiles_r;
        oh = tr * CW_TR;
        ow = tc * CW_TC;
    };
#pragma unroll 1
    for (int i = 0; i < CW_D; ++i) dma_slab();              // slabs 0 .. 3 of the stream
    unsigned emax = 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll 1
    for (int v = blockIdx.x; v < ntiles; v += gridDim.x) {
        decode(v, img, oh0, ow0);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int nb = 0; nb < NBH; ++nb)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[r][nb][i] = 0.f;
        // full passes of 32 input channels, then - Cin % 32 == 16 - the 16-channel tail pass (two loops, not a branch inside one: the sibling says why)
#pragma unroll 1
        for (int pass = 0; pass < full_passes; ++pass) {
            load_patch(img, oh0, ow0, pass * CW_CC, 8);
            asm volatile("s_barrier" ::: "memory");         // every wavefront is done with the previous patch
            write_patch(8);
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // the patch is in LDS
            run_pass(std::integral_constant<int, 2>{});
        }
        if (tail16) {
            load_patch(img, oh0, ow0, full_passes * CW_CC, 4);
            asm volatile("s_barrier" ::: "memory");
            write_patch(4);
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            run_pass(std::integral_constant<int, 1>{});
        }

        // ---- epilogue: lane = output channel, registers = 16 of the 32 pixels of a row; the row's buffer descriptor ends behind its last
        // valid pixel, so the hardware's range check drops the stores past the image's right edge
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int oh = oh0 + 2 * rp + r;
            if (oh >= p.OH) continue;
            const size_t pix0 = ((size_t)img * p.OH + oh) * p.OW + ow0;
            const unsigned npix = (unsigned)min(CW_TC, p.OW - ow0);
            typedef __amdgpu_buffer_rsrc_t rsrc_t;
            const rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(p.y + pix0 * p.yld, 0, (int)(npix * (unsigned)p.yld * 4u), 0x00020000);
            int lane_e = lane;
            asm volatile("" : "+v"(lane_e));
            const int l31e = lane_e & 31, lhie = lane_e >> 5;
#pragma unroll
            for (int nb = 0; nb < NBH; ++nb) {
                const int n = (ch * NBH + nb) * 32 + l31e;
                if (n < p.Ng) {
                    const float bv = p.bias ? p.bias[n] : 0.f;
                    float o[16];
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        o[i] = fmaf(acc[r][nb][i], p.w3w_inv, bv);
                        emax = max(emax, __float_as_uint(o[i]) & 0x7fffffffu);
                    }
                    if (p.act == ACT_RELU) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) o[i] = fmaxf(o[i], 0.f);
                    } else if (p.act != ACT_NONE) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) o[i] = rd_act(o[i], p.act);
                    }
                    const unsigned yoff = ((unsigned)(4 * lhie) * (unsigned)p.yld + (unsigned)n) * 4u;
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o[i]), ry, (int)yoff, (int)((unsigned)((i & 3) + 8 * (i >> 2)) * (unsigned)p.yld * 4u), 2);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // (DMA pieces still in flight target this workgroup's LDS)
    if ((emax >= 0x7f800000u || !(amax < 65504.f)) && p.range_flag) rd_raise_flag(p.range_flag);
}

static inline int cw_nbh(int cout) { return ((cout + 31) / 32 + 1) / 2; }

// geometry the kernel can run (and the host prepares a weight image for, where the builder asks for one)
bool conv3x3_wide_shape_ok(int kh, int kw, int cin, int cout) {
    return kh == 3 && kw == 3 && cin % 16 == 0 && cin >= 64 && cin <= 768 && cout % 32 == 0 && cout > 96 && cout <= 256;
}

// p.w3w is set by a builder that asked for the route (Builder::set_conv3x3_wide): the route is never taken by shape alone
bool conv3x3_wide_applies(const ConvParams& p) {
    static const bool off = rd_env_off("RD_CONV3X3_WIDE");
    // the kernel forms byte offsets inside one image of X in 32 bits; a row of Y is addressed from a 64-bit base
    const bool fits32 = (unsigned long long)p.H * p.W * (unsigned long long)p.xld * 4ull < (1ull << 31) && (unsigned long long)CW_TC * p.yld * 4ull < (1ull << 31);
    return !off && p.w3w && p.w3w_inv > 0.f && conv3x3_wide_shape_ok(p.KH, p.KW, p.Cin, p.Ng) && p.SH == 1 && p.SW == 1 && p.PT == 1 && p.PL == 1 &&
           p.OH == p.H && p.OW == p.W && p.out_mode == OUT_NHWC && !p.ascale && !p.ln_g && p.rld == 0 && (p.xld % 4) == 0 && fits32;
}

void launch_conv3x3_wide(const ConvParams& p, hipStream_t s) {
    if (p.M <= 0) return;
    const int tiles_r = (p.OH + CW_TR - 1) / CW_TR, tiles_c = (p.OW + CW_TC - 1) / CW_TC;
    const int ntiles = p.N * tiles_r * tiles_c;
    const int nstep = 9 * (p.Cin / 16);
    const int n_cu = rd_cu_budget(rd_cu_count());
    const int nbh = cw_nbh(p.Ng);
    const size_t lds = (size_t)2 * CW_PLANE + (size_t)CW_D * nbh * 4096;
    const dim3 grid((unsigned)std::min(ntiles, n_cu)), block(CW_NT);
    static unsigned long long ok2 = 0, ok3 = 0, ok4 = 0;
    switch (nbh) {
        case 2:
            rd_allow_dynamic_lds((const void*)conv3x3_wide_kernel<2>, lds, ok2);
            hipLaunchKernelGGL(conv3x3_wide_kernel<2>, grid, block, lds, s, p, tiles_r, tiles_c, ntiles, nstep);
            break;
        case 3:
            rd_allow_dynamic_lds((const void*)conv3x3_wide_kernel<3>, lds, ok3);
            hipLaunchKernelGGL(conv3x3_wide_kernel<3>, grid, block, lds, s, p, tiles_r, tiles_c, ntiles, nstep);
            break;
        default:
            rd_allow_dynamic_lds((const void*)conv3x3_wide_kernel<4>, lds, ok4);
            hipLaunchKernelGGL(conv3x3_wide_kernel<4>, grid, block, lds, s, p, tiles_r, tiles_c, ntiles, nstep);
            break;
    }
}

// Host: the weight image.  w = folded weights [N][K], k = (kh * 3 + kw) * Cin + ci.  Slab order = the kernel's step order (full passes
// of 32 input channels, tap-major, two k-steps per tap; then - Cin % 32 == 16 - one pass of 16).  A slab holds, for every one of the
// 2 NBH 32-wide output blocks (zeros behind N), the hi and the lo fragment (1 KB each): lane (l31, lhi) carries w[nb * 32 + l31][k .. k + 8)
// of its k-half.  Weights are scaled by 2^ex so that max |w| lands in [2^13, 2^14); returns 2^-ex.
float prepare_conv3x3_wide_weights(const float* w, int N, int Cin, std::vector<uint16_t>& img) {
    const int K = 9 * Cin, nb_n = 2 * cw_nbh(N), nstep = 9 * (Cin / 16);
    img.assign((size_t)nstep * nb_n * 2 * 512, 0);
    const int ex = rd_pow2_exp(w, (size_t)N * K, RD_EXP_CLAMP);
    const int full = Cin / 32, tail16 = (Cin % 32) / 16;
    size_t slab = 0;
    for (int pass = 0; pass < full + tail16; ++pass) {
        const int ksn = pass < full ? 2 : 1;
        for (int tap = 0; tap < 9; ++tap)
            for (int ks = 0; ks < ksn; ++ks, ++slab)
                for (int nb = 0; nb < nb_n; ++nb)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int n = nb * 32 + (lane & 31);
                        if (n >= N) continue;
                        for (int e = 0; e < 8; ++e) {
                            const int k = tap * Cin + pass * 32 + ks * 16 + 8 * (lane >> 5) + e;
                            const size_t base = ((slab * nb_n + nb) * 2) * 512 + (size_t)lane * 8 + e;
                            rd_split_scaled(w[(size_t)n * K + k], ex, img[base], img[base + 512]);
                        }
                    }
    }
    return std::ldexp(1.f, -ex);
}

}  // namespace rd
