// MobileNetV3 (large, scale 0.5, no SE) in the detector geometry: the backbone of the PP-OCRv3 multilingual detector
// (build_ppocrv3_det_mobile).  An inverted-residual block is, after the load-time fold of its three Conv + BatchNorm pairs
// (derive_ppocrv3_det_mobile_weights):
//   e = act(x We^T + be)            expand 1x1, cin -> mid
//   d = act(dw_kxk(pad0(e)) + bd)   depthwise k = 3 / 5, stride 1 / 2, zero padding around the ACTIVATED e
//   y = d Wl^T + bl (+ x)           linear 1x1, mid -> cout; the shortcut where stride == 1 and cin == cout
// with act = ReLU (the blocks at 1/2, 1/4 and 1/8 of the page) or hardswish v relu6(v + 3) / 6 (everything below).  The channel counts
// are narrow and odd: cin / cout 8 ... 80, mid 8 ... 480, all multiples of 8, six of them no multiple of 16.
//
// mbv3_dw_kernel<K, S, TW>: the depthwise layer alone (the unfused route).  One thread = 4 channels x TW adjacent output columns of one
// row, channel quads fastest (every access a coalesced 16 bytes), as lcv3_dw_kernel - which knows hardswish and a scalar affine only.
// pre_act (MBV3_NONE / RELU / HSWISH) is the PRODUCER's activation, applied on load to the elements inside the map only, so the padding
// is zeros of the activated tensor; post_act is this layer's own, applied in the epilogue.  The sum runs from the bias over kh, kw.
//
// mbv3_block_kernel<K, S, ACT>: the whole block in one launch, all in fp32 FMA chains (the fp32-input MFMA gives the same bits at the
// same rate on gfx950, and at under 500 MAC per pixel the block is bound by memory, not arithmetic), so no precision mode and no range
// guard applies to it.  A 256-thread workgroup owns TH x TW output pixels of one image:
//   1. the input patch with its halo, (TH - 1) S + K by (TW - 1) S + K pixels x cin, goes to LDS (in_hswish: the producer wrote
//      convolution + bias of a hardswish layer - conv1 - and the activation is applied here, on load, and again on the shortcut's read);
//   2. e for every patch pixel -> LDS; a patch pixel outside the map gets ZERO, not act(be): it is the depthwise layer's padding;
//   3. d for every output pixel -> LDS (over the input patch, which is dead by then);
//   4. y = d Wl^T + bl (+ shortcut, read again from global memory: it is hot in L2) -> global NHWC.
// Rows of the LDS images are padded by 4 floats: a wavefront's 16-byte reads of 16 consecutive pixels then fall on 64 distinct banks for
// every cin / mid served.  We, be, Wl, bl sit in LDS too (read as broadcasts); the depthwise weights come from global memory (coalesced,
// L1-resident).  Every sum runs from its bias over the channel (or tap) index upwards: the order is a property of the layer and does not
// depend on tile, column, image index or batch.
//
//   <K, S>   tile (rows x cols)   patch     LDS bytes at the served geometry                 VGPRs (ReLU / hardswish)   workgroups / CU (LDS-bound unless noted)
//   <3, 1>   8 x 16               10 x 18   17856 (8-8-8), 59552 (16-40-16)                  146 / 146                  3 (VGPR-bound), 2
//   <3, 2>   8 x 8                17 x 17   58752 (8-32-16)                                  146 / 146                  2
//   <5, 2>   4 x 8                11 x 19   60160 (16-40-24)                                 161 / 166                  2
//   <5, 1>   8 x 8                12 x 12   69216 (24-64-24; above 64 KB: dynamic, opted in) 161 / 166                  2
// mbv3_dw_kernel: 90 / 90 / 101 / 106 VGPRs for <3,1> / <3,2> / <5,1> / <5,2>.  No scratch, nothing spilled
// (tests/test_isa_resources.py::test_no_hot_kernel_spills).
// mbv3_block_launch_ok declines everything else: another k or stride, channels off the multiples (cin % 4, mid % 8, cout % 8), more than
// 80 KB of LDS (two workgroups per CU; mid 120 at 3x3 / 2 needs 147 KB), a shortcut on a block that has none, misaligned views, an
// empty map or a grid beyond 2^31 workgroups.  Ragged tiles, maps smaller than a tile or the halo, odd H / W under stride 2: every global
// load is guarded by the map's bounds and every store by (OH, OW).
#include "rd_device.h"

namespace rd {

template <int ACT>
__device__ __forceinline__ float mbv3_act(float v) {
    if (ACT == MBV3_RELU) return fmaxf(v, 0.f);
    if (ACT == MBV3_HSWISH) return v * fminf(fmaxf(v + 3.f, 0.f), 6.f) * (1.f / 6.f);
    return v;
}
__device__ __forceinline__ f32x4 mbv3_act4(f32x4 v, int act) {
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = act == MBV3_RELU ? mbv3_act<MBV3_RELU>(v[e]) : act == MBV3_HSWISH ? mbv3_act<MBV3_HSWISH>(v[e]) : v[e];
    return r;
}

// ---------------------------------------------------------------------------------------------------------------- depthwise layer alone
template <int K, int S, int TW>
__global__ void __launch_bounds__(256) mbv3_dw_kernel(Mbv3DwParams p) {
    constexpr int P = K / 2, NIN = (TW - 1) * S + K;
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
        const int iw0 = ow0 * S - P;
#pragma unroll
        for (int kh = 0; kh < K; ++kh) {
            const int ih = oh * S - P + kh;
            if (ih < 0 || ih >= p.H) continue;
            const float* row = p.x + ((size_t)n * p.H + ih) * p.W * p.xld + c;
            f32x4 in[NIN];
#pragma unroll
            for (int i = 0; i < NIN; ++i) {
                const int iw = iw0 + i;
                in[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (iw >= 0 && iw < p.W) in[i] = mbv3_act4(*reinterpret_cast<const f32x4*>(row + (size_t)iw * p.xld), p.pre_act);
            }
#pragma unroll
            for (int kw = 0; kw < K; ++kw) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(p.w + (size_t)(kh * K + kw) * p.C + c);
#pragma unroll
                for (int j = 0; j < TW; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(in[j * S + kw][e], wv[e], acc[j][e]);
            }
        }
        float* yrow = p.y + ((size_t)n * p.OH + oh) * p.OW * p.yld + c;
#pragma unroll
        for (int j = 0; j < TW; ++j) {
            const int ow = ow0 + j;
            if (ow >= p.OW) break;
            *reinterpret_cast<f32x4*>(yrow + (size_t)ow * p.yld) = mbv3_act4(acc[j], p.post_act);
        }
    }
}

static inline bool mbv3_act_ok(int a) { return a == MBV3_NONE || a == MBV3_RELU || a == MBV3_HSWISH; }
static inline bool mbv3_aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

bool mbv3_dw_shape_ok(int k, int s, int c) { return (k == 3 || k == 5) && (s == 1 || s == 2) && c >= 4 && c % 4 == 0; }

bool mbv3_dw_launch_ok(const Mbv3DwParams& p) {
    return mbv3_dw_shape_ok(p.K, p.S, p.C) && p.N >= 1 && p.H >= 1 && p.W >= 1 && p.OH == (p.H - 1) / p.S + 1 && p.OW == (p.W - 1) / p.S + 1 &&
           p.xld >= p.C && p.yld >= p.C && p.xld % 4 == 0 && p.yld % 4 == 0 && mbv3_act_ok(p.pre_act) && mbv3_act_ok(p.post_act) &&
           mbv3_aligned16(p.x) && mbv3_aligned16(p.y) && mbv3_aligned16(p.w) && mbv3_aligned16(p.bias);   // (a null pointer: filled in later)
}

bool launch_mbv3_dw(const Mbv3DwParams& p, hipStream_t s) {
    if (!mbv3_dw_launch_ok(p) || !p.x || !p.y || !p.w || !p.bias) return false;
    constexpr int TW = 4;
    const long total = (long)p.N * p.OH * ((p.OW + TW - 1) / TW) * (p.C >> 2);
    const long blocks = (total + 255) / 256;
    const long cap = p.max_blocks > 0 ? p.max_blocks : 65536;                 // (grid-stride loop; max_blocks: a test's way to the wrap)
    const dim3 g((unsigned)(blocks > cap ? cap : blocks)), b(256);
    if (p.K == 3 && p.S == 1) hipLaunchKernelGGL((mbv3_dw_kernel<3, 1, TW>), g, b, 0, s, p);
    else if (p.K == 3 && p.S == 2) hipLaunchKernelGGL((mbv3_dw_kernel<3, 2, TW>), g, b, 0, s, p);
    else if (p.K == 5 && p.S == 1) hipLaunchKernelGGL((mbv3_dw_kernel<5, 1, TW>), g, b, 0, s, p);
    else hipLaunchKernelGGL((mbv3_dw_kernel<5, 2, TW>), g, b, 0, s, p);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- the block in one launch
template <int K, int S>
struct Mbv3Tile {
    static constexpr int TH = (K == 5 && S == 2) ? 4 : 8;
    static constexpr int TW = (K == 3 && S == 1) ? 16 : 8;
    static constexpr int PH = (TH - 1) * S + K, PW = (TW - 1) * S + K;
    static constexpr int NHP = PH * PW, NOP = TH * TW;
};
constexpr int MBV3_PAD = 4;                      // floats behind every LDS row of the patch images
constexpr size_t MBV3_MAX_LDS = 80 * 1024;       // two workgroups per CU

// floats of LDS: [patch x (cin + 4) | outputs x (mid + 4), whichever is larger][patch x (mid + 4)][We][be][Wl][bl]
static inline size_t mbv3_block_lds_floats(int nhp, int nop, int cin, int mid, int cout) {
    const size_t xs = (size_t)nhp * (cin + MBV3_PAD), ds = (size_t)nop * (mid + MBV3_PAD);
    return (xs > ds ? xs : ds) + (size_t)nhp * (mid + MBV3_PAD) + (size_t)mid * cin + mid + (size_t)cout * mid + cout;
}

template <int K, int S, int ACT>
__global__ void __launch_bounds__(256) mbv3_block_kernel(Mbv3BlockParams p, int tiles_h, int tiles_w) {
    using T = Mbv3Tile<K, S>;
    constexpr int P = K / 2, TH = T::TH, TW = T::TW, PW = T::PW, NHP = T::NHP, NOP = T::NOP;
    extern __shared__ __align__(16) float mbv3_lds[];
    const int cin = p.cin, mid = p.mid, cout = p.cout;
    const int XS = cin + MBV3_PAD, ES = mid + MBV3_PAD;
    const int xs_fl = NHP * XS, ds_fl = NOP * ES;
    float* Xs = mbv3_lds;                        // input patch [NHP][XS]; from step 3 on: depthwise output Ds [NOP][ES]
    float* Ds = mbv3_lds;
    float* Es = mbv3_lds + (xs_fl > ds_fl ? xs_fl : ds_fl);     // expanded patch [NHP][ES]
    float* We = Es + NHP * ES;                   // [mid][cin]
    float* be = We + mid * cin;
    float* Wl = be + mid;                        // [cout][mid]
    float* bl = Wl + cout * mid;

    int bid = blockIdx.x;
    const int ow0 = (bid % tiles_w) * TW;
    bid /= tiles_w;
    const int oh0 = (bid % tiles_h) * TH;
    const int n = bid / tiles_h;
    const int t = threadIdx.x;
    const int ih0 = oh0 * S - P, iw0 = ow0 * S - P;
    const float* xn = p.x + (size_t)n * p.H * p.W * p.xld;

    // ---- 1. parameters and the input patch
    for (int i = t; i < (mid * cin) >> 2; i += 256) reinterpret_cast<f32x4*>(We)[i] = reinterpret_cast<const f32x4*>(p.we)[i];
    for (int i = t; i < (cout * mid) >> 2; i += 256) reinterpret_cast<f32x4*>(Wl)[i] = reinterpret_cast<const f32x4*>(p.wl)[i];
    for (int i = t; i < mid; i += 256) be[i] = p.be[i];
    for (int i = t; i < cout; i += 256) bl[i] = p.bl[i];
    const int cin4 = cin >> 2;
    for (int i = t; i < NHP * cin4; i += 256) {
        const int pix = i / cin4, c = (i - pix * cin4) << 2;
        const int ih = ih0 + pix / PW, iw = iw0 + pix % PW;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ih >= 0 && ih < p.H && iw >= 0 && iw < p.W) {
            v = *reinterpret_cast<const f32x4*>(xn + ((size_t)ih * p.W + iw) * p.xld + c);
            if (p.in_hswish) v = mbv3_act4(v, MBV3_HSWISH);
        }
        *reinterpret_cast<f32x4*>(Xs + pix * XS + c) = v;
    }
    __syncthreads();

    // ---- 2. expand: item = (8 mid channels, patch pixel), pixels fastest (the weight reads of a wavefront are broadcasts)
    const int nchunk_e = mid >> 3;
    for (int i = t; i < nchunk_e * NHP; i += 256) {
        const int chunk = i / NHP, pix = i - chunk * NHP;
        const int m0 = chunk << 3;
        const int ih = ih0 + pix / PW, iw = iw0 + pix % PW;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = be[m0 + j];
        const float* xr = Xs + pix * XS;
        const float* wr = We + m0 * cin;
        for (int c = 0; c < cin; c += 4) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + c);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + j * cin + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j] = fmaf(xv[e], wv[e], acc[j]);
            }
        }
        const bool inside = ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
        f32x4 o0, o1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o0[j] = inside ? mbv3_act<ACT>(acc[j]) : 0.f;
            o1[j] = inside ? mbv3_act<ACT>(acc[4 + j]) : 0.f;
        }
        *reinterpret_cast<f32x4*>(Es + pix * ES + m0) = o0;
        *reinterpret_cast<f32x4*>(Es + pix * ES + m0 + 4) = o1;
    }
    __syncthreads();

    // ---- 3. depthwise: item = (output pixel, 4 mid channels), channels fastest
    const int q = mid >> 2;
    for (int i = t; i < NOP * q; i += 256) {
        const int op = i / q, c = (i - op * q) << 2;
        const int r = op / TW, col = op % TW;
        f32x4 acc = *reinterpret_cast<const f32x4*>(p.bd + c);
        const float* er = Es + ((r * S) * PW + col * S) * ES + c;
#pragma unroll
        for (int kh = 0; kh < K; ++kh)
#pragma unroll
            for (int kw = 0; kw < K; ++kw) {
                const f32x4 ev = *reinterpret_cast<const f32x4*>(er + (kh * PW + kw) * ES);
                const f32x4 wv = *reinterpret_cast<const f32x4*>(p.wd + (size_t)(kh * K + kw) * mid + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(ev[e], wv[e], acc[e]);
            }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = mbv3_act<ACT>(acc[e]);
        *reinterpret_cast<f32x4*>(Ds + op * ES + c) = acc;
    }
    __syncthreads();

    // ---- 4. linear (+ shortcut): item = (8 output channels, output pixel), pixels fastest
    const int nchunk_l = cout >> 3;
    for (int i = t; i < nchunk_l * NOP; i += 256) {
        const int chunk = i / NOP, op = i - chunk * NOP;
        const int o0 = chunk << 3;
        const int oh = oh0 + op / TW, ow = ow0 + op % TW;
        if (oh >= p.OH || ow >= p.OW) continue;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = bl[o0 + j];
        const float* dr = Ds + op * ES;
        const float* wr = Wl + o0 * mid;
        for (int m = 0; m < mid; m += 4) {
            const f32x4 dv = *reinterpret_cast<const f32x4*>(dr + m);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + j * mid + m);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j] = fmaf(dv[e], wv[e], acc[j]);
            }
        }
        f32x4 y0 = {acc[0], acc[1], acc[2], acc[3]}, y1 = {acc[4], acc[5], acc[6], acc[7]};
        if (p.shortcut) {              // (stride 1, cin == cout: the output pixel IS the input pixel)
            const float* xs = xn + ((size_t)oh * p.W + ow) * p.xld + o0;
            f32x4 s0 = *reinterpret_cast<const f32x4*>(xs), s1 = *reinterpret_cast<const f32x4*>(xs + 4);
            if (p.in_hswish) {
                s0 = mbv3_act4(s0, MBV3_HSWISH);
                s1 = mbv3_act4(s1, MBV3_HSWISH);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                y0[e] += s0[e];
                y1[e] += s1[e];
            }
        }
        float* yp = p.y + (((size_t)n * p.OH + oh) * p.OW + ow) * p.yld + o0;
        *reinterpret_cast<f32x4*>(yp) = y0;
        *reinterpret_cast<f32x4*>(yp + 4) = y1;
    }
}

template <int K, int S>
static long mbv3_block_grid(const Mbv3BlockParams& p, int* tiles_h, int* tiles_w) {
    using T = Mbv3Tile<K, S>;
    *tiles_h = (p.OH + T::TH - 1) / T::TH;
    *tiles_w = (p.OW + T::TW - 1) / T::TW;
    return (long)p.N * *tiles_h * *tiles_w;
}

template <int K, int S>
static bool mbv3_block_fits(const Mbv3BlockParams& p, size_t* lds_bytes, long* grid, int* tiles_h, int* tiles_w) {
    using T = Mbv3Tile<K, S>;
    *lds_bytes = mbv3_block_lds_floats(T::NHP, T::NOP, p.cin, p.mid, p.cout) * sizeof(float);
    *grid = mbv3_block_grid<K, S>(p, tiles_h, tiles_w);
    return *lds_bytes <= MBV3_MAX_LDS && *grid >= 1 && *grid <= 0x7fffffffL;
}

static bool mbv3_block_plan(const Mbv3BlockParams& p, size_t* lds_bytes, long* grid, int* tiles_h, int* tiles_w) {
    if (!(p.K == 3 || p.K == 5) || !(p.S == 1 || p.S == 2)) return false;
    if (p.cin < 4 || p.cin % 4 != 0 || p.mid < 8 || p.mid % 8 != 0 || p.cout < 8 || p.cout % 8 != 0 || p.cin > 4096 || p.mid > 4096 || p.cout > 4096) return false;
    if (p.act != MBV3_RELU && p.act != MBV3_HSWISH) return false;
    if (p.shortcut && (p.S != 1 || p.cin != p.cout)) return false;
    if (p.N < 1 || p.H < 1 || p.W < 1 || p.OH != (p.H - 1) / p.S + 1 || p.OW != (p.W - 1) / p.S + 1) return false;
    if (p.xld < p.cin || p.yld < p.cout || p.xld % 4 != 0 || p.yld % 4 != 0) return false;
    const void* ptrs[] = {p.x, p.y, p.we, p.be, p.wd, p.bd, p.wl, p.bl};
    for (const void* q : ptrs)
        if (!mbv3_aligned16(q)) return false;        // (a null pointer passes: a planner fills x / y in at run time; the launch wants all)
    if (p.K == 3 && p.S == 1) return mbv3_block_fits<3, 1>(p, lds_bytes, grid, tiles_h, tiles_w);
    if (p.K == 3 && p.S == 2) return mbv3_block_fits<3, 2>(p, lds_bytes, grid, tiles_h, tiles_w);
    if (p.K == 5 && p.S == 1) return mbv3_block_fits<5, 1>(p, lds_bytes, grid, tiles_h, tiles_w);
    return mbv3_block_fits<5, 2>(p, lds_bytes, grid, tiles_h, tiles_w);
}

bool mbv3_block_launch_ok(const Mbv3BlockParams& p) {
    size_t lds;
    long grid;
    int th, tw;
    return mbv3_block_plan(p, &lds, &grid, &th, &tw);
}

template <int K, int S, int ACT>
static void mbv3_block_launch(const Mbv3BlockParams& p, size_t lds, long grid, int tiles_h, int tiles_w, hipStream_t s) {
    static unsigned long long allowed = 0;
    if (lds > 64 * 1024) rd_allow_dynamic_lds(reinterpret_cast<const void*>(&mbv3_block_kernel<K, S, ACT>), MBV3_MAX_LDS, allowed);
    hipLaunchKernelGGL((mbv3_block_kernel<K, S, ACT>), dim3((unsigned)grid), dim3(256), lds, s, p, tiles_h, tiles_w);
}

bool launch_mbv3_block(const Mbv3BlockParams& p, hipStream_t s) {
    size_t lds;
    long grid;
    int th, tw;
    if (!mbv3_block_plan(p, &lds, &grid, &th, &tw)) return false;
    if (!p.x || !p.y || !p.we || !p.be || !p.wd || !p.bd || !p.wl || !p.bl) return false;
    const bool relu = p.act == MBV3_RELU;
    if (p.K == 3 && p.S == 1) relu ? mbv3_block_launch<3, 1, MBV3_RELU>(p, lds, grid, th, tw, s) : mbv3_block_launch<3, 1, MBV3_HSWISH>(p, lds, grid, th, tw, s);
    else if (p.K == 3 && p.S == 2) relu ? mbv3_block_launch<3, 2, MBV3_RELU>(p, lds, grid, th, tw, s) : mbv3_block_launch<3, 2, MBV3_HSWISH>(p, lds, grid, th, tw, s);
    else if (p.K == 5 && p.S == 1) relu ? mbv3_block_launch<5, 1, MBV3_RELU>(p, lds, grid, th, tw, s) : mbv3_block_launch<5, 1, MBV3_HSWISH>(p, lds, grid, th, tw, s);
    else relu ? mbv3_block_launch<5, 2, MBV3_RELU>(p, lds, grid, th, tw, s) : mbv3_block_launch<5, 2, MBV3_HSWISH>(p, lds, grid, th, tw, s);
    return true;
}

}  // namespace rd
