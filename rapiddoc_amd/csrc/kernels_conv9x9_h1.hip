// Direct 9x9 / stride-1 / pad-4 convolution to 33 .. 64 output channels on the fp16 matrix cores with ONE fp32 accumulator set: LKPAN's
// inp_conv (256 -> 64) and pan_lat_conv (64 -> 64) of the PP-OCRv5 server detector (necks/db_fpn.py:418-525), 186 GFLOP of a 960 x 704
// page.  The scheme is that of conv3x3_h1_kernel (kernels_conv3x3_h1.hip): x = hi + lo unscaled, weights pre-scaled per matrix by a power
// of two, hi.hi + hi.lo + lo.hi into one accumulator, the input patch split ONCE into two fp16 planes in LDS (taps = address offsets),
// weight slabs in consumption order streamed by LDS-DMA through a ring of four, persistent four-wavefront workgroups on 8 x 32 output
// tiles, a wavefront = two rows of 32 pixels x 64 channels, one barrier per k-step (12 MFMAs per wavefront).
//
// Tile and patch - the design question of a 4-pixel halo.  The 8 x 32 tile needs a 16 x 40 patch (640 pixels, 2.5 input pixels per
// output pixel).  With the 3x3 kernel's 32 input channels per pass its two planes are 640 x 80 B x 2 = 102 KB: ONE workgroup per CU, and
// the patch staging (global -> split -> LDS), the epilogue and every barrier wait of that workgroup leave the matrix pipes idle.  Taken
// here: 16 input channels per pass.  A pixel is 32 B + 16 B of padding per plane (48 = 16 x odd: conflict-free ds_read_b128), the two
// planes 61 440 B, with the 16 KB slab ring 77 824 B: TWO workgroups per CU with independent barriers, as the 3x3 kernel has.  What the
// narrower pass costs is staging twice as often - but a pass here is 81 k-steps (972 MFMAs per wavefront) per 640 x 16 staged values,
// where the 3x3 kernel runs 18 steps per 340 x 32: the staging share is a sixth of the 3x3 kernel's, so halving the pass is cheap and a
// smaller tile (4 x 32: 12 x 40 patch, 3.75 input pixels per output pixel, half the MFMAs per weight fragment read) is not needed.
// Everything else (bias, activation, residual, range guard, NHWC views with row strides, XCD-contiguous tile order) as the 3x3 kernel.
// Results do not depend on the launch size (one kernel for every M).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "rd_device.h"

namespace rd {

static constexpr int C9_K = 9, C9_HALO = 4;
static constexpr int C9_TR = 8, C9_TC = 32;                            // output tile (rows x columns)
static constexpr int C9_PW = C9_TC + 2 * C9_HALO, C9_PH = C9_TR + 2 * C9_HALO;   // patch 16 x 40
static constexpr int C9_PP = C9_PW * C9_PH;                            // 640 patch pixels
static constexpr int C9_CC = 16;                                       // input channels per pass
static constexpr int C9_S = C9_CC * 2 + 16;                            // 48 bytes per patch pixel in one fp16 plane
static constexpr int C9_PLANE = C9_PP * C9_S;                          // 30 720 bytes
static constexpr int C9_D = 4;                                         // weight slabs in the ring
static constexpr int C9_NB = 2;                                        // 32-wide output channel blocks
static constexpr int C9_SLAB = C9_NB * 2 * 1024;                       // bytes of one weight slab (one k-step: hi + lo fragment per block)
static constexpr int C9_NS = C9_K * C9_K;                              // k-steps per pass

typedef _Float16 c9_f16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void c9_split4(const f32x4 v, float neg1, f16x4& hi, f16x4& lo) {
#pragma unroll
    for (int e = 0; e < 4; e += 2) {
        const c9_f16x2 h = __builtin_convertvector(f32x2{v[e], v[e + 1]}, c9_f16x2);
        hi[e] = h[0];
        hi[e + 1] = h[1];
        lo[e] = (_Float16)__builtin_fmaf((float)h[0], neg1, v[e]);
        lo[e + 1] = (_Float16)__builtin_fmaf((float)h[1], neg1, v[e + 1]);
    }
}

struct C9Frag { f16x8 ah[2], al[2], bh[C9_NB], bl[C9_NB]; };

// "my piece of the slab about to be read has landed" (every wavefront issues one DMA instruction per slab, C9_D - 2 younger slabs may
// still be in flight), then the workgroup barrier - see c3_wait_slab_barrier in kernels_conv3x3_h1.hip for the argument
__device__ __forceinline__ void c9_wait_slab_barrier() { asm volatile("s_waitcnt vmcnt(2)\n\ts_barrier" ::: "memory"); }

__global__ void __launch_bounds__(256, 2) conv9x9_h1_kernel(ConvParams p, int tiles_r, int tiles_c, int ntiles, int nstep) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lhi = lane >> 5;
    unsigned char* Ph = smem;
    unsigned char* Pl = smem + C9_PLANE;
    unsigned char* Wb = smem + 2 * C9_PLANE;
    const _Float16* wimg = reinterpret_cast<const _Float16*>(p.w9);
    float neg1 = -1.f;
    asm volatile("" : "+s"(neg1));

    // ---- weight stream: slab j of the global step sequence = slab (j mod nstep) of the image -> ring buffer j mod C9_D
    int w_issue = 0, w_pos = 0;
    auto dma_slab = [&]() {
        const _Float16* src = wimg + (size_t)w_pos * (C9_SLAB / 2) + lane * 8 + wave * 512;
        unsigned char* dst = Wb + (unsigned)(w_issue & (C9_D - 1)) * C9_SLAB + wave * 1024;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
        ++w_issue;
        if (++w_pos == nstep) w_pos = 0;
    };

    // ---- patch staging: 640 pixels x 4 channel groups (of 4) = 2560 slots, ten per thread: slot i of thread t is pixel (t >> 2) + 64 i,
    // group t & 3 (decoded from a copy of the thread id the compiler cannot see through, so that the per-slot rows / columns / offsets are
    // not hoisted out of the tile loop and kept alive through the MFMA steps)
    constexpr int NSLOT = 10;
    int stid = tid;
    float amax = 0.f;
    int img = 0, oh0 = 0, ow0 = 0;
    u32x4 pre[NSLOT];
    unsigned pre_ok = 0;
    auto load_patch = [&](int im, int oh, int ow, int c0) {
        typedef __amdgpu_buffer_rsrc_t rsrc_t;
        const rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x + (size_t)im * p.H * p.W * p.xld + c0), 0, 0x7fffffff, 0x00020000);
        stid = tid;
        asm volatile("" : "+v"(stid));
        const unsigned gsel = 16u * (unsigned)(stid & 3);
        const int pix0 = stid >> 2;
        pre_ok = 0;
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) {
            const int pix = pix0 + 64 * i;
            const int pr = pix / C9_PW, pc = pix - pr * C9_PW;
            const int ih = oh - C9_HALO + pr, iw = ow - C9_HALO + pc;
            if ((unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W) pre_ok |= 1u << i;
            const unsigned off = ((unsigned)min(max(ih, 0), p.H - 1) * (unsigned)p.W + (unsigned)min(max(iw, 0), p.W - 1)) * (unsigned)p.xld * 4u + gsel;
            pre[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)off, 0, 0);
        }
    };
    auto write_patch = [&]() {
        stid = tid;
        asm volatile("" : "+v"(stid));
        const unsigned o0 = (unsigned)(stid >> 2) * C9_S + (unsigned)(stid & 3) * 8;
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) {
            const f32x4 x4 = (pre_ok >> i) & 1u ? __builtin_bit_cast(f32x4, pre[i]) : f32x4{0.f, 0.f, 0.f, 0.f};
            f16x4 hi, lo;
            c9_split4(x4, neg1, hi, lo);
#pragma unroll
            for (int e = 0; e < 4; ++e) amax = (x4[e] != x4[e]) ? INFINITY : fmaxf(amax, fabsf(x4[e]));
            const unsigned o = o0 + (unsigned)(64 * i) * C9_S;
            *reinterpret_cast<f16x4*>(Ph + o) = hi;
            *reinterpret_cast<f16x4*>(Pl + o) = lo;
        }
    };

    // ---- fragments of one step: A = this wavefront's two pixel rows at tap (kh, kw); B = the slab's fragments
    const unsigned a_lane = (unsigned)((2 * wave) * C9_PW + l31) * C9_S + (unsigned)lhi * 16u;
    const unsigned b_lane = (unsigned)lane * 16u;
    auto read_frag = [&](C9Frag& f, int tap, int slab) {
        const int kh = tap / C9_K, kw = tap - C9_K * kh;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const unsigned a = a_lane + (unsigned)((r + kh) * C9_PW + kw) * C9_S;
            f.ah[r] = *reinterpret_cast<const f16x8*>(Ph + a);
            f.al[r] = *reinterpret_cast<const f16x8*>(Pl + a);
        }
        const unsigned char* wb = Wb + (unsigned)(slab & (C9_D - 1)) * C9_SLAB + b_lane;
#pragma unroll
        for (int nb = 0; nb < C9_NB; ++nb) {
            f.bh[nb] = *reinterpret_cast<const f16x8*>(wb + (2 * nb) * 1024);
            f.bl[nb] = *reinterpret_cast<const f16x8*>(wb + (2 * nb + 1) * 1024);
        }
    };

    f32x16 acc[2][C9_NB];
    C9Frag fr[2];
    int g = 0;                                              // global step counter (slab index of the step being computed)
    // one pass: 81 k-steps (one per tap) over the staged 16 channels, fully unrolled (taps are compile-time offsets)
    auto run_pass = [&]() {
        read_frag(fr[0], 0, g);
#pragma unroll
        for (int s = 0; s < C9_NS; ++s) {
            // slab g + 1 (read below) has landed everywhere, and every wavefront has read its fragments of slab g: its buffer is free
            c9_wait_slab_barrier();
            dma_slab();                                     // slab g + C9_D -> the buffer of slab g
            C9Frag& cur = fr[s & 1];
            if (s + 1 < C9_NS) read_frag(fr[(s + 1) & 1], s + 1, g + 1);
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int nb = 0; nb < C9_NB; ++nb) acc[r][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.ah[r], cur.bh[nb], acc[r][nb], 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int nb = 0; nb < C9_NB; ++nb) acc[r][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.ah[r], cur.bl[nb], acc[r][nb], 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int nb = 0; nb < C9_NB; ++nb) acc[r][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.al[r], cur.bh[nb], acc[r][nb], 0, 0, 0);
            ++g;
        }
    };

    const int passes = p.Cin / C9_CC;
    auto decode = [&](int v, int& im, int& oh, int& ow) {
        // XCD-contiguous tile order (workgroup b sits on XCD b % 8): an XCD's workgroups walk ONE contiguous run of the tile list
        const int xcd = v & 7, jj = v >> 3, q = ntiles >> 3, rm = ntiles & 7;
        int t = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + jj;
        const int tc = t % tiles_c;
        t /= tiles_c;
        const int tr = t % tiles_r;
        im = t / tiles_r;
        oh = tr * C9_TR;
        ow = tc * C9_TC;
    };
#pragma unroll 1
    for (int i = 0; i < C9_D; ++i) dma_slab();              // slabs 0 .. 3 of the stream
    unsigned emax = 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // (once: from here on a step's barrier has always waited for the next step's slab)
#pragma unroll 1
    for (int v = blockIdx.x; v < ntiles; v += gridDim.x) {
        decode(v, img, oh0, ow0);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int nb = 0; nb < C9_NB; ++nb)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[r][nb][i] = 0.f;
#pragma unroll 1
        for (int pass = 0; pass < passes; ++pass) {
            load_patch(img, oh0, ow0, pass * C9_CC);        // (requested before the barrier: in flight while the stragglers arrive)
            asm volatile("s_barrier" ::: "memory");         // every wavefront is done with the previous patch
            write_patch();
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // the patch is in LDS
            run_pass();
        }

        // ---- epilogue: lane = output channel, registers = 16 of the 32 pixels of a row; every access goes through a buffer descriptor
        // that ENDS behind the row's last valid pixel (the hardware's range check drops what lies past the image's right edge)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int oh = oh0 + 2 * wave + r;
            if (oh >= p.OH) continue;
            const size_t pix0 = ((size_t)img * p.OH + oh) * p.OW + ow0;
            const unsigned npix = (unsigned)min(C9_TC, p.OW - ow0);
            typedef __amdgpu_buffer_rsrc_t rsrc_t;
            const rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(p.y + pix0 * p.yld, 0, (int)(npix * (unsigned)p.yld * 4u), 0x00020000);
            const rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.res ? p.res + pix0 * p.rld : p.y), 0,
                                                                (int)(npix * (unsigned)(p.res ? p.rld : p.yld) * 4u), 0x00020000);
            int lane_e = lane;
            asm volatile("" : "+v"(lane_e));                 // (keeps the epilogue's offsets out of the registers that live through the steps)
            const int l31e = lane_e & 31, lhie = lane_e >> 5;
#pragma unroll
            for (int nb = 0; nb < C9_NB; ++nb) {
                const int n = nb * 32 + l31e;
                if (n < p.Ng) {
                    const float bv = p.bias ? p.bias[n] : 0.f;
                    float o[16];
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        o[i] = fmaf(acc[r][nb][i], p.w9_inv, bv);
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
                    if (p.res) {
                        const unsigned roff = ((unsigned)(4 * lhie) * (unsigned)p.rld + (unsigned)n) * 4u;
                        float rs[16];
#pragma unroll
                        for (int i = 0; i < 16; ++i)
                            rs[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rr, (int)roff, (int)((unsigned)((i & 3) + 8 * (i >> 2)) * (unsigned)p.rld * 4u), 0));
#pragma unroll
                        for (int i = 0; i < 16; ++i) o[i] += rs[i];
                    }
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o[i]), ry, (int)yoff, (int)((unsigned)((i & 3) + 8 * (i >> 2)) * (unsigned)p.yld * 4u), 2);
                }
                __builtin_amdgcn_sched_barrier(0);          // (one block at a time: the blocks' temporaries do not pile up)
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // (DMA pieces still in flight target this workgroup's LDS)
    if ((emax >= 0x7f800000u || !(amax < 65504.f)) && p.range_flag) rd_raise_flag(p.range_flag);
}

// geometry the kernel can run (and the host prepares a weight image for)
bool conv9x9_h1_shape_ok(int kh, int kw, int cin, int cout) {
    return kh == C9_K && kw == C9_K && cin % C9_CC == 0 && cin >= 16 && cin <= 512 && cout > 32 && cout <= 32 * C9_NB;
}

bool conv9x9_h1_applies(const ConvParams& p) {
    static const bool off = rd_env_off("RD_CONV9X9_H1");
    // (the patch loads address an image with 32-bit byte offsets)
    return !off && p.w9 && p.w9_inv > 0.f && conv9x9_h1_shape_ok(p.KH, p.KW, p.Cin, p.Ng) && p.SH == 1 && p.SW == 1 && p.PT == C9_HALO && p.PL == C9_HALO &&
           p.OH == p.H && p.OW == p.W && p.out_mode == OUT_NHWC && !p.ascale && !p.ln_g && (p.xld % 4) == 0 &&
           (unsigned long long)p.H * p.W * (unsigned long long)p.xld < (1ull << 29);
}

void launch_conv9x9_h1(const ConvParams& p, hipStream_t s) {
    if (p.M <= 0) return;
    const int tiles_r = (p.OH + C9_TR - 1) / C9_TR, tiles_c = (p.OW + C9_TC - 1) / C9_TC;
    const int ntiles = p.N * tiles_r * tiles_c;
    const int nstep = C9_NS * (p.Cin / C9_CC);
    const int n_cu = rd_cu_budget(rd_cu_count());
    const size_t lds = (size_t)2 * C9_PLANE + (size_t)C9_D * C9_SLAB;
    const dim3 grid((unsigned)std::min(ntiles, 2 * n_cu)), block(256);
    static unsigned long long ok = 0;
    rd_allow_dynamic_lds((const void*)conv9x9_h1_kernel, lds, ok);
    hipLaunchKernelGGL(conv9x9_h1_kernel, grid, block, lds, s, p, tiles_r, tiles_c, ntiles, nstep);
}

// Host: the weight image.  w = folded weights [N][K], k = (kh * 9 + kw) * Cin + ci.  Slab order = the kernel's step order: passes of 16
// input channels, tap-major inside a pass.  A slab holds, for both 32-wide output blocks, the hi and the lo fragment (1 KB each): lane
// (l31, lhi) carries w[nb * 32 + l31][k .. k + 8) of its k-half.  Weights are scaled by 2^ex so that max |w| lands in [2^13, 2^14);
// returns 2^-ex.
float prepare_conv9x9_h1_weights(const float* w, int N, int Cin, std::vector<uint16_t>& img) {
    const int K = C9_NS * Cin, passes = Cin / C9_CC, nstep = C9_NS * passes;
    img.assign((size_t)nstep * C9_NB * 2 * 512, 0);
    const int ex = rd_pow2_exp(w, (size_t)N * K, RD_EXP_CLAMP);
    size_t slab = 0;
    for (int pass = 0; pass < passes; ++pass)
        for (int tap = 0; tap < C9_NS; ++tap, ++slab)
            for (int nb = 0; nb < C9_NB; ++nb)
                for (int lane = 0; lane < 64; ++lane) {
                    const int n = nb * 32 + (lane & 31);
                    if (n >= N) continue;
                    for (int e = 0; e < 8; ++e) {
                        const int k = tap * Cin + pass * C9_CC + 8 * (lane >> 5) + e;
                        const size_t base = ((slab * C9_NB + nb) * 2) * 512 + (size_t)lane * 8 + e;
                        rd_split_scaled(w[(size_t)n * K + k], ex, img[base], img[base + 512]);
                    }
                }
    return std::ldexp(1.f, -ex);
}

}  // namespace rd
