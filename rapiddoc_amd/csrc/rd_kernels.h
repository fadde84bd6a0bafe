// Kernel launch interface of the MI355X page-inference engine (gfx950 only).
// All activations are NHWC fp32; a "view" is (base pointer, channel stride ld) so that channel
// slices of a wider buffer (concat-free dense blocks, FPN concat) are addressed without copies.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/rapiddoc_mi355.h"      // rd_formula_crop, rd_formula_plan
#include "rd_host.h"

namespace rd {

enum Act : int { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2, ACT_SILU = 3, ACT_SIGMOID = 4, ACT_HSIG = 5, ACT_HSIG_PADDLE = 6 };
enum OutMode : int { OUT_NHWC = 0, OUT_DECONV2X2 = 1 };

// Dense convolution as implicit GEMM on fp32 MFMA:  Y[M, Ng] = im2col(X)[M, K] * W[Ng, K]^T
//   M = N*OH*OW, K = KH*KW*Cin (ci fastest), Ng = Cout (OUT_NHWC) or 4*Cout (OUT_DECONV2X2).
struct ConvParams {
    const float* x; int xld;
    int N, H, W, Cin;
    const float* w;      // [Ng][K]
    const uint16_t* wh;  // fp16x3 ("h3") mode: the same weights split into hi / lo fp16 matrices [Ng][Kp], Kp = ceil8(K)
    const uint16_t* wl;
    const float* bias;   // [Cout] or nullptr (BN already folded into w / bias)
    float* y; int yld;
    int OH, OW, Cout;
    int KH, KW, SH, SW, PT, PL;
    const float* res; int rld;      // added after the activation, same geometry as y
    const float* ascale;            // must be null: once a [N][Cin] multiplier of the X rows on load (1x1 only), applied by NO kernel since
                                    // round 2.  launch_conv_route throws on it and Builder::conv refuses it at plan time
    const float* ln_g; const float* ln_b;   // skinny path (M <= 32, K <= 512) only: LayerNorm(eps 1e-5) applied to every X row
                                            // before the product (fuses the pre-LN of a transformer decode step)
    int act, out_mode;
    int M, K, Ng;
    unsigned* range_flag = nullptr;   // split-fp16 kernels: raised when an activation leaves the fp16 range
    // single-accumulator split GEMM (kernels_gemm_h1.hip): fragment-ordered image of the power-of-two pre-scaled weights and the
    // inverse of that scale (prepare_gemm_h1_weights), or nullptr / 0
    const uint16_t* w1 = nullptr;
    float w1_inv = 0.f;
    // the small-M (<= 32 rows) fp32 path of launch_conv_igemm: only for layers whose M is a batch size BY CONSTRUCTION (the formula decoder's
    // linears); image layers never set it - their kernel is picked by the layer, not by how many rows a launch happens to hold
    int allow_skinny = 0;
    // one-accumulator direct 3x3 (kernels_conv3x3_h1.hip): slab-ordered fragment image of the pre-scaled weights + the inverse scale
    const uint16_t* w3 = nullptr;
    float w3_inv = 0.f;
    // one-accumulator direct 9x9 (kernels_conv9x9_h1.hip): slab-ordered fragment image of the pre-scaled weights + the inverse scale
    const uint16_t* w9 = nullptr;
    float w9_inv = 0.f;
    int fast_epi = 1;               // interior tiles of the split implicit-GEMM kernels store through buffer accesses (round 5; RD_CONV_FAST_EPI=0: A/B)
    // one-accumulator direct 3x3 to 128 .. 256 output channels (kernels_conv3x3_wide.hip): set only for the layers of a builder that asked for
    // the route (Builder::set_conv3x3_wide), so no other layer of that shape moves
    const uint16_t* w3w = nullptr;
    float w3w_inv = 0.f;
};
// The kernel a dense convolution runs on.  The route of an op is decided ONCE - by conv_split_route (ops that carry p.wh / p.wl) or
// conv_f32_route - from the geometry, the weight-image pointers, the mode fields (act, out_mode, allow_skinny, ln_g) and the RD_* switches;
// x, y, res and ascale are never read, so a planner asks with unbound ConvParams and gets the answer of the launch.  Whether the op
// multiplies its rows by `ascale` is passed in.  The builder names the op with conv_route_name and launches with launch_conv_route.
enum ConvRoute : int {
    // split-fp16 path, in the order conv_split_route asks (the *_applies predicate next to each kernel)
    CONV_STREAM, CONV_C3H1, CONV_C3WIDE, CONV_C9H1, CONV_DIRECT, CONV_GEMM_H1, CONV_DMA16, CONV_DMA8,
    CONV_H3_256x128, CONV_H3_128x96, CONV_H3_256x64, CONV_H3_128x32, CONV_H3_128x64,   // the staged implicit-GEMM tiles (kernels_conv_h3.hip)
    CONV_H3_TO_F32,       // a tensor beyond the staged kernels' 32-bit offsets: whatever conv_f32_route says, at launch
    // fp32 MFMA path (kernels_conv.hip)
    CONV_SKINNY, CONV_F32_128x32, CONV_F32_128x64, CONV_F32_128x96, CONV_F32_128x128
};
ConvRoute conv_split_route(const ConvParams& p, bool has_ascale);
ConvRoute conv_f32_route(const ConvParams& p);      // CONV_SKINNY is the one route that honours ln_g / ln_b (K <= 512 then)
const char* conv_route_name(ConvRoute r);           // the per-op profile's tag (the builder appends "/h3" on the split path)
void launch_conv_route(ConvRoute r, const ConvParams& p, hipStream_t s);
void launch_conv_f32_route(ConvRoute r, const ConvParams& p, hipStream_t s);   // its fp32 half (kernels_conv.hip)
// callers without a plan: the route, then launch_conv_route
void launch_conv_igemm(const ConvParams& p, hipStream_t s);
// fp32-accurate variant on the fp16 matrix cores (3 MFMAs per product, see kernels_conv_h3.hip); needs p.wh / p.wl
bool gemm_h3_dma_applies(const ConvParams& p);
bool gemm_h3_dma_uses16(const ConvParams& p);   // the 16-wavefront kernel (short-K GELU layers, > 2^32-element tensors) or the 8-wavefront one
void launch_gemm_h3_dma(const ConvParams& p, bool use16, hipStream_t s);
// single-accumulator split GEMM, 64 x 128 per wavefront, two 4-wavefront workgroups per CU (kernels_gemm_h1.hip); needs p.w1 / p.w1s
bool gemm_h1_shape_ok(int K, int cout);       // host-side: which layers get a weight image
bool gemm_h1_applies(const ConvParams& p);
void launch_gemm_h1(const ConvParams& p, hipStream_t s);
float prepare_gemm_h1_weights(const float* w, int N, int K, std::vector<uint16_t>& img);   // returns the inverse scale
void launch_conv_igemm_h3(const ConvParams& p, hipStream_t s);
// RT-DETR-family head operators, preparation only (kernels_rtdetr.hip; nothing in the engine calls them)
void launch_msdeform_attn(const float* value, const int32_t* shapes, const int32_t* start, const float* loc, const float* attn, float* out, int B,
                          int S, int H, int D, int Q, int L, int P, hipStream_t s);
void launch_topk_rows(const float* scores, int rows, int n, int k, float* out_vals, int32_t* out_idx, hipStream_t s);
// stem tail: 3x3 / stride 2 / pad 1 conv (+ bias + act3) -> 1x1 conv (+ bias + act4) in one kernel (kernels_stem34.hip, round 6).
// x NHWC [N][H][W][xld >= Cin]; y NHWC [N][OH][OW][yld >= N2], OH = (H - 1) / 2 + 1, OW likewise; pointers and row strides 16-byte aligned.
struct Stem34Params {
    const float* x; int xld;
    int N, H, W, Cin;
    float* y; int yld;
    int OH, OW, N1, N2;
    const uint16_t* w3; float w3_inv; const float* b3;     // slab-ordered image of the 3x3, bias padded with zeros to 32-wide blocks
    const uint16_t* w4; float w4_inv; const float* b4;     // fragment image of the 1x1 (input channels in the 3x3's C/D register order), bias [N2]
    int act3, act4;
    unsigned* range_flag = nullptr;
    int abl = 0;     // developer ablation bits (results are garbage): 1 no fragment reads / MFMAs, 2 no patch split / write, 4 no patch loads, 8 no epilogue, 16 no weight DMA
};
bool stem34_shape_ok(int cin, int n1, int n2);
bool stem34_enabled();                        // RD_STEM34=1 (default off: measured level with the two-kernel path, profiles/r6_stem34.txt)
void launch_stem34(const Stem34Params& p, hipStream_t s);
void prepare_stem34_weights(const float* w3, const float* w4, int Cin, int N1, int N2, std::vector<uint16_t>& img3, std::vector<uint16_t>& img4,
                            float inv[2]);
// direct 3x3 / stride 1 / pad 1, <= 96 output channels, one accumulator set, two workgroups per CU (kernels_conv3x3_h1.hip, round 6)
bool conv3x3_h1_shape_ok(int kh, int kw, int cin, int cout);   // host-side: which layers get a weight image
bool conv3x3_h1_applies(const ConvParams& p);
void launch_conv3x3_h1(const ConvParams& p, hipStream_t s);
float prepare_conv3x3_h1_weights(const float* w, int N, int Cin, std::vector<uint16_t>& img);   // returns the inverse scale
// direct 3x3 / stride 1 / pad 1 to 128 .. 256 output channels (multiples of 32) from 64 .. 768 input channels, one accumulator set, eight
// wavefronts on one staged patch (kernels_conv3x3_wide.hip): PPHGNet_small's HG_Block layers.  Needs p.w3w / p.w3w_inv, which only a builder
// that opted in sets; refuses (and the layer takes the generic route) an image of 2^31 bytes or more, and a layer with a residual (p.rld != 0:
// the planner sets rld only with one).  RD_CONV3X3_WIDE=0: A/B switch
bool conv3x3_wide_shape_ok(int kh, int kw, int cin, int cout);
bool conv3x3_wide_applies(const ConvParams& p);
void launch_conv3x3_wide(const ConvParams& p, hipStream_t s);
float prepare_conv3x3_wide_weights(const float* w, int N, int Cin, std::vector<uint16_t>& img);   // returns the inverse scale
// direct 9x9 / stride 1 / pad 4 to 33 .. 64 output channels, one accumulator set, two workgroups per CU (kernels_conv9x9_h1.hip): LKPAN
bool conv9x9_h1_shape_ok(int kh, int kw, int cin, int cout);   // host-side: which layers get a weight image
bool conv9x9_h1_applies(const ConvParams& p);
void launch_conv9x9_h1(const ConvParams& p, hipStream_t s);
float prepare_conv9x9_h1_weights(const float* w, int N, int Cin, std::vector<uint16_t>& img);   // returns the inverse scale
// direct 2x2 / 3x3 stride-1 convolution for narrow outputs (kernels_conv_direct_h3.hip); launch_conv_igemm_h3 dispatches to it
bool conv_direct_h3_supported(const ConvParams& p);   // geometry
bool conv_direct_h3_applies(const ConvParams& p);     // geometry + routing policy
void launch_conv_direct_h3(const ConvParams& p, hipStream_t s);
// small-K layers (padded K <= 256, <= 96 output channels), operands streamed from global memory (kernels_conv_stream_h3.hip)
bool conv_stream_h3_enabled();                        // RD_CONV_STREAM != 0 (read once)
bool conv_stream_h3_supported(const ConvParams& p);
bool conv_stream_h3_applies(const ConvParams& p);
void launch_conv_stream_h3(const ConvParams& p, hipStream_t s);
// host-side twin of conv_stream_h3_supported for the weight preparation (no ConvParams yet)
inline bool conv_stream_h3_shape_ok(int kh, int kw, int cin, int cout) {
    return cin % 4 == 0 && cin <= 64 && kh * kw * ((cin + 15) / 16 * 16) <= 256 && cout <= 96;
}
// 1 x 3 sequence convolution over token rows with two K segments (kernels_seqconv.hip): the SVTR neck's conv1 / conv4 of the PP-OCRv5
// server recogniser.  Y[m][n] = act(sum_tap sum_c X[m + tap - 1][c] W[n][tap Cin + c] + bias[n]), Cin = C0 + C1, channels [0, C0) read
// from x0 and [C0, Cin) from x1; row m + tap - 1 counts as zero where it leaves m's text line.
struct SeqConvParams {
    const float* x0; int ld0, C0;     // token rows [M][ld0]; pointers and row strides 16-byte aligned, C0 % 16 == 0
    const float* x1; int ld1, C1;     // second K segment, or nullptr / 0 / 0
    const float* w;                   // fp32 [N][3 Cin], BN folded (the native fp32 route)
    const uint16_t* wh; const uint16_t* wl;   // the same matrix as (hi, lo) fp16 planes (split_weights_h3: rows padded to 32), or nullptr: fp32 route
    const float* bias;                // [N] or nullptr
    float* y; int yld;
    int M, N;                         // N % 64 == 0
    int T;                            // uniform form: M = B T rows, every line has T tokens
    const int32_t* tokinfo;           // ragged form (or nullptr): [M] position in the line | tokens of the line << 16
    int act;
    unsigned* range_flag;             // split route: raised when an operand leaves the fp16 range
};
bool seqconv_shape_ok(int C0, int C1, int N);
void launch_seqconv(const SeqConvParams& p, hipStream_t s);

// First conv of a network: 3x3 stride 2 pad 1, Cin = 3, reads the caller's NCHW (or NHWC u8/f32) image.
struct StemParams {
    const float* x;   // NCHW f32 [N,3,H,W]  (or [N,1,H,W] read three times when in_ch == 1: the reference repeats grey formulas)
    int N, H, W, in_ch;
    const float* w;   // [27][Cout] (kh,kw,ci major; co fastest)
    const float* bias;
    float* y; int yld; int OH, OW, Cout;
    int act;
};
void launch_stem_conv3x3s2(const StemParams& p, hipStream_t s);

// Fused stem front (kernels_stem_fused.hip): stem1 (3x3 s2) + stem2a + stem2b (2x2, pad right / bottom) + the 2x2 / s1 max-pool in
// one kernel, x NCHW -> cat NHWC [N][H2][W2][2 c1] = [pool | stem2b]; split-fp16 matrix cores; c1 in {24, 32, 48}
bool stem_fused_supported(int c1);
void prepare_stem_fused_weights(int c1, const float* w1_stem_layout, const float* w2a_folded, const float* w2b_folded, std::vector<uint16_t>& img);
// line_tab (optional): the recogniser's per-line width table (LineTab below) - every image n is treated as if it were only
// line_tab[4 n] columns wide: e / a / cat beyond its own half-resolution width are the zero padding the next layer expects
void launch_stem_fused(int c1, const float* x, int N, int H, int W, int in_ch, const uint16_t* wimg, const float* bias, float* y, int yld,
                       unsigned* range_flag, hipStream_t s, const int32_t* line_tab = nullptr);

// Per-line widths of a recogniser launch (REC_LINE_WIDTHS): text lines of DIFFERENT reference padded widths share one [B,3,48,W]
// tensor and every line is computed exactly as if it had been padded to its own width only (rapid_ocr.py:404-449 pads a line to
// its chunk-of-6's width; LightSVTR, the SE pooling and the conv borders all see that width).  int32 [B][4]:
//   0: w_in  the line's reference padded width (columns >= w_in of x are zero)
//   1: w2 = (w_in - 1) / 2 + 1 after stem1            2: w4 = (w2 - 1) / 2 + 1 after stem3 = the width of every block
//   3: first token of the line in the token buffer (the line has w4 / 2 tokens)
constexpr int kLineTabStride = 4;

struct DwParams {
    const float* x; int xld;
    int N, H, W, C;
    const float* w;     // [KH*KW][C]
    const float* bias;  // [C]
    float* y; int yld;
    int OH, OW, KH, KW, SH, SW, PT, PL;
    int act;
    const float* res; int rld;  // added after activation
    float* gap_partial;         // optional [N][gap_chunks][C] partial sums of the OUTPUT (SE fusion), or nullptr
    int gap_chunks;             // host only: the chunk count the buffer was sized for (dwconv_gap_chunks); launch_dwconv checks it
    // ragged rows (the recogniser's batched tail): the tensor is [1][1][W = all tokens][C], token i sits at position
    // tokinfo[i] & 0xffff of a text line of tokinfo[i] >> 16 tokens and the kernel's horizontal taps stop at the line's ends
    const int32_t* tokinfo = nullptr;
    // per-image valid width (LineTab column 2; stride-1 'same' convs only): input columns >= line_w[n * line_w_stride] read as the
    // conv's zero padding and are left out of the SE partial sums
    const int32_t* line_w = nullptr; int line_w_stride = 0;
    int dbg = 0;                // developer (RD_DW_DBG): 1 no stores, 2 no loads - timing only
};
// The kernel a depthwise convolution runs on and the partial-sum chunks per image it writes when the SE pooling rides along (0: the fused
// pooling is not available on that kernel).  variant: the LDS kernels' instantiation (dwconv_lds_variant / kernel size), the tiled kernel's width.
enum DwKernel : int { DW_PIXEL, DW_LDS, DW_KXK_LDS, DW_COL, DW_TILED };
struct DwRoute { DwKernel kernel; int variant; int gap_chunks; };
// launch_dwconv and the planner (dwconv_gap_chunks, which sizes the partial-sum buffer) both ask here.  Ragged rows (p.tokinfo) and the line
// table (p.line_w) are read from p as the launch sees it; wants_gap = the launch will carry gap_partial.  The rule that lets the planner ask
// with wants_gap = true and an UNBOUND DwParams: the only kernel that looks at a pointer or a leading dimension is DW_KXK_LDS, and it is
// never taken when the gap is wanted; ragged ops (1 x k) have no pooled kernel.  Everything else is geometry and switches.
DwRoute dw_route(const DwParams& p, bool wants_gap);
// throws std::runtime_error when p.gap_partial is set and p.gap_chunks (the planner's count) is not the route's
void launch_dwconv(const DwParams& p, hipStream_t s);
inline int dwconv_gap_chunks(const DwParams& p) { return dw_route(p, true).gap_chunks; }
// kernels_dw_lds.hip: the LDS-DMA-staged 3x3 / stride 1 for the recogniser's 3 / 6 / 12-row maps (geometry only; 0 = none) ...
int dwconv_lds_variant(const DwParams& p);
int dwconv_lds_gap_chunks(const DwParams& p);
void launch_dwconv_lds(const DwParams& p, int variant, hipStream_t s);
// ... and the 5x5 / 7x7 stride-1 kernel with one channel per lane (no ragged rows, line table or SE pooling: dw_route)
bool dwconv_kxk_lds_applies(const DwParams& p);
void launch_dwconv_kxk_lds(const DwParams& p, int k, hipStream_t s);

// PPLCNetV3 depthwise layer (kernels_lcv3.hip): y = post_act ? post_s hardswish(dw(x') + bias) + post_b : dw(x') + bias, x' = pre_act ? pre_s hardswish(x) + pre_b : x,
// k = 3 / 5, strides (1,1), (2,1), (1,2), (2,2), 'same' padding of ZEROS around the pre-affined map; per-image valid widths of the input / output (LineTab columns) or nullptr
struct Lcv3DwParams {
    const float* x; int xld;
    int N, H, W, C;
    const float* w;      // [K*K][C]
    const float* bias;   // [C]
    float* y; int yld;
    int OH, OW, K, SH, SW;
    int pre_act; float pre_s, pre_b;     // the producing pointwise layer's hardswish + act.lab, applied on load inside the map
    float post_s, post_b;   // this layer's act.lab
    const int32_t* line_in; const int32_t* line_out; int line_stride;
    int post_act;           // 0: convolution + bias only (a stride-2 layer of the detector geometry)
};
bool lcv3_dw_shape_ok(int k, int sh, int sw, int c);
void launch_lcv3_dw(const Lcv3DwParams& p, hipStream_t s);
// The same layer for the mobile detector's rectangular maps (kernels_lcv3_det.hip): a workgroup stages a 2-D input patch with its halo in
// LDS - contiguous row segments of 16 channels, the producer's hardswish + affine applied once per element, inside the map only - and
// computes its output tile from there.  k = 3 / 5, stride (1,1) or (2,2), C % 16 == 0, no line table.
bool lcv3_dw2d_shape_ok(int k, int sh, int sw, int c);
bool lcv3_dw2d_launch_ok(const Lcv3DwParams& p);   // shape_ok, no line table, a non-empty output and a grid below 2^31 workgroups
bool launch_lcv3_dw2d(const Lcv3DwParams& p, hipStream_t s);   // false: not launched (launch_ok says no)
// The 5x5 layer of the recogniser geometry, LDS-staged, with the line table (kernels_mv1e.hip): one workgroup = one line x a strip of output
// columns x 16 channels x all rows.  k = 5, strides (1,1), (2,1), (1,2), H <= 6, C % 16 == 0; launch_ok declines everything else (and a grid
// beyond 2^31 workgroups) and the caller stays on launch_lcv3_dw
bool dw5_strip_launch_ok(const Lcv3DwParams& p);
bool launch_dw5_strip(const Lcv3DwParams& p, hipStream_t s);   // false: not launched (launch_ok says no)
// MobileNetV1Enhance's end: y = AvgPool2d(2, 2)(hardswish(x)) over rows 0 and 1 of a map of H >= 2 rows, floor(W / 2) tokens; line_tab as
// launch_avgpool3x2
void launch_mv1e_pool(const float* x, int xld, float* y, int yld, int N, int H, int W, int C, hipStream_t s, const int32_t* line_tab = nullptr);
// y = s hardswish(x) + b, elementwise: the four stage outputs of the detector's backbone, whose consumers are matrix kernels
void launch_lcv3_act(const float* x, int xld, float* y, int yld, long pixels, int C, float s, float b, hipStream_t st);
// One PPLCNetV3 block without SE, 3x3 / stride 1, in one launch (kernels_lcv3_block.hip): the depthwise layer as above into an LDS tile, the
// pointwise layer on the matrix cores from it.  y = out_act ? out_s hardswish(a W^T + pw_b) + out_b : a W^T + pw_b with
// a = mid_s hardswish(dw(x') + dw_b) + mid_b; split = 1: split-fp16 product guarded by range_flag, 0: fp32 MFMA.
struct Lcv3BlockParams {
    const float* x; int xld;
    int N, H, W, cin, cout;
    const float* dw_w;   // [9][cin]
    const float* dw_b;   // [cin]
    const float* pw_w;   // [cout][cin]
    const float* pw_b;   // [cout]
    float* y; int yld;
    int pre_act; float pre_s, pre_b;
    float mid_s, mid_b;
    int out_act; float out_s, out_b;
    const int32_t* line_w; int line_stride;
    int split; unsigned* range_flag;
};
bool lcv3_block_shape_ok(int cin, int cout);      // (16, 32), (32, 64), (64, 64)
void launch_lcv3_block(const Lcv3BlockParams& p, hipStream_t s);
// MobileNetV3 in the detector geometry (kernels_mbv3.hip; PP-OCRv3 multilingual detector).  Activations of its layers:
enum Mbv3Act : int { MBV3_NONE = 0, MBV3_RELU = 1, MBV3_HSWISH = 2 };
// Depthwise layer: y = post(dw_kxk(pre(x)) + bias), zero padding around pre(x) (the producer's activation touches the elements INSIDE the
// map only); k = 3 / 5, stride (1,1) / (2,2), C % 4 == 0, OH = (H - 1) / S + 1
struct Mbv3DwParams {
    const float* x; int xld;
    int N, H, W, C;
    const float* w;      // [K*K][C]
    const float* bias;   // [C]
    float* y; int yld;
    int OH, OW, K, S;
    int pre_act, post_act;   // Mbv3Act
    int max_blocks = 0;      // > 0: cap of the grid (default 65536 workgroups; the kernel walks the rest in a grid-stride loop)
};
bool mbv3_dw_shape_ok(int k, int s, int c);
bool mbv3_dw_launch_ok(const Mbv3DwParams& p);    // shape, strides and 16-byte alignment of every pointer that is set
bool launch_mbv3_dw(const Mbv3DwParams& p, hipStream_t s);   // false: not launched (launch_ok says no, or a pointer is null)
// One inverted-residual block without SE in one launch, all fp32: y = act(dw_kxk(pad0(act(x' We^T + be))) + bd) Wl^T + bl (+ x'),
// x' = in_hswish ? hardswish(x) : x.  The expanded tensor never leaves the chip.
struct Mbv3BlockParams {
    const float* x; int xld;
    int N, H, W, cin, mid, cout;
    const float* we; const float* be;   // expand [mid][cin], [mid]
    const float* wd; const float* bd;   // depthwise [K*K][mid], [mid]
    const float* wl; const float* bl;   // linear [cout][mid], [cout]
    float* y; int yld;
    int OH, OW, K, S;
    int act;         // MBV3_RELU / MBV3_HSWISH: the expand and the depthwise layer's activation
    int in_hswish;   // x is convolution + bias of a hardswish layer (conv1): activated on load, for the expand and the shortcut alike
    int shortcut;    // y += x' (stride 1 and cin == cout only)
};
// what the kernel serves: k 3 / 5, stride 1 / 2, cin % 4, mid % 8, cout % 8, at most 80 KB of LDS for the tile of (k, stride), 16-byte
// aligned views, a non-empty map, OH / OW as above, a grid below 2^31 workgroups.  Null pointers pass (a planner fills them in later)
bool mbv3_block_launch_ok(const Mbv3BlockParams& p);
bool launch_mbv3_block(const Mbv3BlockParams& p, hipStream_t s);   // false: not launched (launch_ok says no, or a pointer is null)
// MobileNetV3 small in the text-line geometry (kernels_mbv3s.hip; the text-line direction classifier).  Depthwise layer with separate row
// and column strides: y = post(dw_kxk(pre(x)) + bias), zero padding around pre(x); k = 3 / 5, strides (1,1) / (2,1), C % 8 == 0,
// OH = (H - 1) / SH + 1, OW = (W - 1) / SW + 1
struct Mbv3sDwParams {
    const float* x; int xld;
    int N, H, W, C;
    const float* w;      // [K*K][C]
    const float* bias;   // [C]
    float* y; int yld;
    int OH, OW, K, SH, SW;
    int pre_act, post_act;   // Mbv3Act
    int max_blocks = 0;      // > 0: cap of the grid (default 65536 workgroups; the kernel walks the rest in a grid-stride loop)
};
bool mbv3s_dw_shape_ok(int k, int sh, int sw, int c);
bool mbv3s_dw_launch_ok(const Mbv3sDwParams& p);    // shape, strides and 16-byte alignment of every pointer that is set
bool launch_mbv3s_dw(const Mbv3sDwParams& p, hipStream_t s);   // false: not launched (launch_ok says no, or a pointer is null)
// The classifier's end: x = conv2's convolution + bias [N][H][W][xld >= C] -> hardswish -> MaxPool2d(2, 2) -> global average ->
// Linear C -> 2 -> softmax; prob [N][2]; aux (optional) [N][2 + C] = logits | pooled features.  H, W >= 2 (a non-empty pooled map), C <= 1024
struct ClsTailParams {
    const float* x; int xld;
    int N, H, W, C;
    const float* w;      // [2][C]
    const float* bias;   // [2]
    float* prob;
    float* aux;
};
bool cls_tail_launch_ok(const ClsTailParams& p);
bool launch_cls_tail(const ClsTailParams& p, hipStream_t s);
// One inverted-residual block of the fused classifier route (cls_line_kernel / cls_block_kernel), on folded weights:
// we [mid][cin], be [mid], wd [K*K][mid], bd [mid], squeeze-excite w1 [mid/4][mid], b1, w2 [mid][mid/4], b2 (se != 0), wl [cout][mid], bl
struct ClsBlockParams {
    const float *we, *be, *wd, *bd, *w1, *b1, *w2, *b2, *wl, *bl;
    int k, cin, mid, cout, sh;       // kernel 3 / 5, row stride 1 / 2 (the column stride is 1)
    int se, act, shortcut;           // act: MBV3_RELU / MBV3_HSWISH
    int ms, es_ld;                   // cls_block_plan: mid channels per expand / depthwise slice, LDS row stride of the slice
};
bool cls_block_plan(ClsBlockParams& L, int H, int W);
size_t cls_block_scratch_floats(const ClsBlockParams& L, int H, int W);   // per workgroup (min(N, 512) of them)
bool cls_block_launch_ok(const ClsBlockParams& L, int N, int H, int W, int xld, int yld);
bool launch_cls_block(const ClsBlockParams& L, const float* x, int xld, float* y, int yld, int N, int H, int W, float* scratch, hipStream_t s);
// The whole classifier in one launch: x NCHW [B][3][H][W] -> prob [B][2] (aux [B][2 + c2], stage_out[i] NCHW: optional).  conv1 as the stem
// builder folds it (w1c [27][c1], b1c [c1]), conv2 w2c [c2][32], b2c [c2], the head wf [2][c2], bf [2].  scratch: cls_line_scratch_floats
struct ClsLineParams {
    const float* x; int B, H, W;
    const float* w1c; const float* b1c; int c1;
    ClsBlockParams blk[11]; int n_blocks;
    const float* w2c; const float* b2c; int c2;
    const float* wf; const float* bf;
    float* prob; float* aux;
    float* stage_out[4]; int stage_block[4];
    float* scratch;
    size_t act_floats, d_floats, per_wg;      // cls_line_plan
    int max_blocks = 0;                       // > 0: cap of the persistent grid (default 512 workgroups), a test's way to the line loop
};
bool cls_line_plan(ClsLineParams& p);
size_t cls_line_scratch_floats(const ClsLineParams& p);
int cls_line_grid(int B, int max_blocks);
bool cls_line_launch_ok(const ClsLineParams& p);     // the plan is current, the shape fits, the views are aligned (null pointers pass)
bool launch_cls_line(const ClsLineParams& p, hipStream_t s);
// cv2.rotate(ROTATE_180) of the packed uint8 crops (LineCropDesc::scratch_off, crop_w x crop_h x 3) of the lines whose classifier output says
// "turned": prob[2 i + 1] > prob[2 i] and prob[2 i + 1] >= thresh; flipped[i] = that decision (0 / 1).  In place: one thread owns both pixels of a pair
struct LineCropDesc;
int launch_line_flip180(const LineCropDesc* descs, int n, const float* prob, float thresh, uint8_t* scratch, int32_t* flipped, hipStream_t s);
// partial[n][h][c] = sum over w < line_w[n * stride] (or W) of x[n][h][w][c]: the SE pooling partial sums, one chunk per map row
bool lcv3_gap_shape_ok(int c);      // c % 4 == 0, c <= 4096
void launch_lcv3_gap_rows(const float* x, int xld, int N, int H, int W, int C, float* partial, const int32_t* line_w, int stride, hipStream_t s);
// y = post_s avg_pool2d([3, 2])(hardswish(x)) + post_b of a 3-row map; line_tab as launch_avgpool3x2
void launch_lcv3_pool(const float* x, int xld, float* y, int yld, int N, int H, int W, int C, float post_s, float post_b, hipStream_t s,
                      const int32_t* line_tab = nullptr);

// 2x2 stride-1 max-pool over an input zero-padded by one pixel on the right/bottom (stem branch b)
void launch_maxpool2x2s1(const float* x, int xld, float* y, int yld, int N, int H, int W, int C, hipStream_t s);
// avg_pool2d(kernel (3,2), stride (3,2)) - rec height collapse
// line_tab: image n writes its w4 / 2 tokens at row line_tab[4 n + 3] of y (compact token buffer) instead of [n][OW]
void launch_avgpool3x2(const float* x, int xld, float* y, int yld, int N, int H, int W, int C, hipStream_t s, const int32_t* line_tab = nullptr);
// y[n, :, w >= line_w[n * stride], :] = 0 (the separate-kernel stem of the fp32 mode under a line table)
void launch_mask_cols(float* y, int yld, int N, int H, int W, int C, const int32_t* line_w, int stride, hipStream_t s);

// Squeeze-excite: deterministic two-stage global average pool, tiny FCs, then y = x * (alpha + s)
void launch_gap_partial(const float* x, int xld, int N, int HW, int C, float* partial, int chunks, hipStream_t s);
struct SeFcParams {
    const float* partial; int chunks; int N, C, Cr; float inv_hw;
    const float* w1; const float* b1;  // [Cr][C], [Cr]
    const float* w2; const float* b2;  // [C][Cr], [C]
    int gate;                          // ACT_HSIG (x/6+.5) or ACT_HSIG_PADDLE (.2x+.5)
    float* scale;                      // [N][C]
    const int32_t* line_w = nullptr; int line_w_stride = 0; int H = 0;   // per-image pooling extent H x line_w[n * stride] instead of 1 / inv_hw
};
// the widths se_fc_kernel serves: float4 channel quads, a row of W1 in two 16-byte loads per lane (Builder::se_gate and rd_debug_se_chain ask here)
bool se_fc_shape_ok(int c);
void launch_se_fc(const SeFcParams& p, hipStream_t s);
bool det_head_tail_supported(int cin, int cmid, int cout);
void launch_det_head_tail(const float* x, int xld, int N, int H, int W, const float* w1, const float* b1, const float* w2, const float* b2,
                          float* y, hipStream_t s);
// Fused local tail of PFHeadLocal (kernels_det_local.hip): maps = 0.5 (shrink + sigmoid(last_1(relu(bn(last_3(cat[shrink, up2(f)])))))),
// f NHWC [N][H/2][W/2][fld >= 64], shrink / y [N][H][W]; H and W even.  wimg16 set: the split-fp16 route, else native fp32 (wimg32).
struct DetLocalParams {
    const float* f; int fld;
    const float* shrink;
    float* y;
    int N, H, W;
    const float* wimg32;            // prepare_det_local_weights' fp32 fragment image
    const uint16_t* wimg16;         // ... and its (hi, lo) fp16 image of the pre-scaled weights, or nullptr
    float w_inv;                    // inverse of that scale
    const float* b3;                // [64] last_3's folded BatchNorm shift
    const float* w1; float b1;      // last_1: [64], bias
    unsigned* range_flag;           // split route: raised when an operand leaves the fp16 range
};
void launch_det_local(const DetLocalParams& p, hipStream_t s);
float prepare_det_local_weights(const float* w3_folded, std::vector<float>& img32, std::vector<uint16_t>& img16);   // returns the inverse scale
void launch_scale_channels(const float* x, int xld, float* y, int yld, const float* scale, float alpha,
                           int N, int HW, int C, hipStream_t s);
// ESE gate of PPHGNet_small's HG_Block (kernels_ese.hip): s[n][c] = sigmoid(b[c] + sum_k w[c][k] mean[n][k]) from launch_gap_partial's sums
// (chunks = ese_gap_chunks(H W): from the layer's map alone), C % 4 == 0 up to 1024; then y = x s (+ idn), in place or into a channel slot
bool ese_shape_ok(int c);
int ese_gap_chunks(int hw);
void launch_ese_gate(const float* partial, int chunks, int N, int C, float inv_hw, const float* w, const float* b, float* s, hipStream_t st);
void launch_ese_apply(const float* x, int xld, const float* s, const float* idn, int ild, float* y, int yld, int N, int HW, int C, hipStream_t st);
// MaxPool2d(3, stride 2, padding 1) with torch's -inf padding: y [N][(H - 1) / 2 + 1][(W - 1) / 2 + 1][C], C % 4 == 0
void launch_maxpool3x3s2(const float* x, int xld, float* y, int yld, int N, int H, int W, int C, hipStream_t st);

// y[n,h,w,:] (+)= x[n,h/f,w/f,:]   (nearest-neighbour upsample by integer factor f)
void launch_upsample(const float* x, int xld, float* y, int yld, int N, int H, int W, int C, int f, int accumulate,
                     hipStream_t s);

void launch_layernorm(const float* x, int xld, float* y, int yld, const float* g, const float* b, int M, int C,
                      float eps, hipStream_t s);
// qkv: [B*T][3*heads*hd] (q|k|v, head-major) -> o: [B*T][heads*hd]
// seg != nullptr: ragged batch - sequence b is seg[2b+1] tokens starting at token seg[2b]; T is then the longest one
int attention_h3_max_t();                     // lines up to this many tokens run on the matrix-core kernel, longer ones on the VALU kernel
bool attention_h3_applies(int T, int hd);     // kernels_attention_h3.hip: the same attention on the split-fp16 matrix cores
int attention_lds_keys(int hd);               // keys whose K and V rows the VALU kernel holds in LDS at once; longer lines run over key tiles
// range_flag (optional): raised when the matrix-core kernel converts a K, V or scaled Q value outside the fp16 range (as ConvParams::range_flag)
void launch_attention_h3(const float* qkv, float* o, int B, int T, int heads, int hd, float scale, hipStream_t s, const int32_t* seg,
                         unsigned* range_flag = nullptr);
void launch_attention(const float* qkv, float* o, int B, int T, int heads, int hd, float scale, hipStream_t s, const int32_t* seg = nullptr,
                      unsigned* range_flag = nullptr);
// the VALU kernel (native fp32) for EVERY line, whatever its length: precision "fp32", developer entries
void launch_attention_valu(const float* qkv, float* o, int B, int T, int heads, int hd, float scale, hipStream_t s, const int32_t* seg = nullptr);

// kernels_vit_attn.hip (the UniTable encoder, a plain ViT-B).  The same attention contract at head dimension 64, T <= 1024, dense batches:
// keys in tiles of 64 with an online softmax, both products on the fp32-input matrix cores - one kernel for every precision mode, no range flag
bool vit_attention_applies(int T, int hd);
void launch_vit_attention(const float* qkv, float* o, int B, int T, int heads, float scale, hipStream_t s);
// x NCHW [B][3][H][W] (H, W multiples of 16) -> y [B * (H/16) * (W/16)][768], column (c * 16 + ky) * 16 + kx: the rows of the patch-embedding GEMM
void launch_vit_patchify(const float* x, float* y, int B, int H, int W, hipStream_t s);
// x [B][T][C] += pos [T][C], in place (C % 4 == 0)
void launch_vit_add_pos(float* x, const float* pos, int B, int T, int C, hipStream_t s);
// launch_layernorm's arithmetic at C = 768 exactly (xld, yld multiples of 4)
void launch_layernorm768(const float* x, int xld, float* y, int yld, const float* g, const float* b, int M, float eps, hipStream_t s);

// y = a + b (same geometry, views)
void launch_add(const float* a, int ald, const float* b, int bld, float* y, int yld, int M, int C, hipStream_t s);

// CTC head statistics from logits: idx[m] = argmax_c z[m][c], prob[m] = 1 / sum_c exp(z[m][c]-max)
void launch_rowmax_softmax(const float* logits, int ld, int M, int C, int32_t* idx, float* prob, hipStream_t s);
// full softmax (only when the caller asks for the reference-shaped [B,T,C] probabilities)
// softmax rows; with idx / prob also numpy's argmax / max of the rows WRITTEN (lowest class among equal values)
void launch_row_softmax(const float* logits, int ld, float* out, int M, int C, hipStream_t s, int32_t* idx = nullptr, float* prob = nullptr);
// Fused CTC head: logits are never materialised.
struct CtcParams {
    const float* x; int xld;   // [M][K]
    const float* w;            // [C][K]
    const float* bias;         // [C]
    int M, K, C;
    float* part;               // workspace [M][nsplit][4] (max, sumexp, idx, pad)
    int nsplit;
    int32_t* idx; float* prob;
    // split-fp16 variant: W' [C][128] as (hi, lo) fp16; range_flag as in ConvParams
    const uint16_t* wh = nullptr; const uint16_t* wl = nullptr;
    unsigned* range_flag = nullptr;
};
void launch_ctc_head(const CtcParams& p, hipStream_t s);   // dispatches on p.wh
int ctc_head_nsplit(int M, int C, bool split_fp16);   // class splits the kernel that launch_ctc_head picks (p.wh set or not) wants

// layout conversion at the C-ABI boundary
void launch_nhwc_to_nchw(const float* x, int xld, float* y, int N, int H, int W, int C, hipStream_t s);
void launch_nchw_to_nhwc(const float* x, float* y, int yld, int N, int C, int H, int W, hipStream_t s);

// image pre-processing: u8 HWC -> bilinear/bicubic resize -> (v*scale - mean)/std -> NCHW f32
struct PreprocParams {
    const uint8_t* src; int H, W;      // HWC, 3 channels
    float* dst; int OH, OW;            // [3][OH][OW] plane of one batch element
    float mean[3], inv_std[3]; float scale;
    int interp;                         // 1 = bilinear, 2 = bicubic (a=-0.75, OpenCV convention)
    int swap_rb;
    int batch = 1;                      // images in this launch: image i reads src + i * src_stride, writes dst + i * dst_stride
    size_t src_stride = 0, dst_stride = 0;
};
void launch_preproc_resize_norm(const PreprocParams& p, hipStream_t s);

// Pillow's antialiased bilinear resample + ToTensor / Normalize (kernels_resize_aa.hip; rd_preproc_resize_aa_norm).  Returns 0, or 1 with
// the message in `err` (a size outside 1 .. RD_RESIZE_AA_MAX_SIDE never launches).  resize_aa_coeffs: the per-axis tables on the host.
// resample_coeffs: the same for a filter (RD_RESAMPLE_*) over the box [box0, box1) of the `in` source pixels.
int resize_aa_coeffs(int in, int out, std::vector<int32_t>& bounds, std::vector<int32_t>& kk);
int resample_coeffs(int filter, int in, double box0, double box1, int out, std::vector<int32_t>& bounds, std::vector<int32_t>& kk);
// The formula pre-process (kernels_resize_aa.hip; rd_formula_margin_boxes / _preproc_plan / _preproc_batch).  The launchers return 0, or 1
// with the message in `err` and nothing launched.
void formula_preproc_plan(int w, int h, rd_formula_plan* plan);
int launch_formula_margin_boxes(int device, const rd_formula_crop* descs_dev, int n, int32_t* boxes_dev, hipStream_t s, std::string& err);
int launch_formula_preproc_batch(int device, const rd_formula_crop* descs, const int32_t* boxes, int n, float* out, uint8_t* out_u8, hipStream_t s,
                                 std::string& err);
int launch_resize_aa_norm(int device, const uint8_t* src, int H, int W, int OH, int OW, const float mean[3], const float std[3], int swap_rb,
                          float* out, uint8_t* out_u8, hipStream_t s, std::string& err);

// Text-line crops for the recogniser, one launch per rec batch: for crop i, output pixel (ox, oy) of the
// 48 x out_w[i] resized line maps to crop coordinates, then through the 3x3 matrix m (crop -> page, i.e. the
// inverse of the reference's cv2.getPerspectiveTransform in utils/ocr_utils.py:494-536) to a bilinear sample
// of page `page`; columns >= out_w[i] are zero (rapidocr resize_norm_img right-pads with 0).
struct CropDesc {
    int32_t page;     // index into the page batch
    int32_t out_w;    // resized width (<= padded batch width)
    float crop_w, crop_h;
    float m[9];
    int32_t rot90;    // 1: the crop is rotated by 90 deg counter-clockwise first (h/w >= 1.5 rule, ocr_utils.py:531-535)
    int32_t pad_;
};
struct CropBatchParams {
    const uint8_t* pages; int H, W; size_t page_stride;   // [P][H][W][3] u8
    const CropDesc* descs; int n;
    float* dst; int OH, OWp;                               // [n][3][OH][OWp]
    float mean[3], inv_std[3]; float scale; int swap_rb;
};
void launch_crop_resize_norm_batch(const CropBatchParams& p, hipStream_t s);

// Reference-shaped text-line crops (kernels_image.hip): cubic perspective warp to the integer-sized uint8 crop
// (cv2.warpPerspective INTER_CUBIC / BORDER_REPLICATE, utils/ocr_utils.py:523-529), 90-degree rotation of tall crops, linear
// resize to height 48, /255, (x - 0.5) / 0.5, zero right-padding (rapidocr resize_norm_img) - two kernels per rec batch.
struct LineCropDesc {
    int32_t page;          // page index in the batch
    int32_t out_w;         // resized width (<= padded batch width)
    int32_t crop_w, crop_h;   // size of the rectified crop (before the optional rotation)
    int32_t rot90;         // np.rot90 the crop first (h / w >= 2, ocr_utils.py:533-535)
    int32_t scratch_off;   // byte offset of this crop's [crop_h][crop_w][3] uint8 image in the scratch buffer
    double m[9];           // crop pixel (x, y, 1) -> page (X, Y, W), row-major (the inverse of getPerspectiveTransform's matrix)
};
struct LineCropParams {
    const uint8_t* pages; int H, W; size_t page_stride;   // [P][H][W][3] u8
    const LineCropDesc* descs; int n;
    uint8_t* scratch; long max_crop_pixels;                // largest crop_w * crop_h of the batch (grid sizing)
    float* dst; int OH, OWp;                               // [n][3][OH][OWp]
    int swap_rb;
};
int launch_line_crops(const LineCropParams& p, hipStream_t s);
int launch_line_warp(const LineCropParams& p, hipStream_t s);          // stage 1 only (pages -> uint8 crops in the scratch buffer)
int launch_line_resize_norm(const LineCropParams& p, hipStream_t s);   // stage 2 only (scratch crops -> fp32 rec batch tensor)
// stage 1 for lines that each name their own source image: include/rapiddoc_mi355.h rd_line_warp_sources.  `host` / `dev`: the same
// descriptors on the host (checked here, line_sources_check.h) and on the device (read by the kernel).  Returns 0, or 1 with the message
// in `err` and nothing launched.
int launch_line_warp_sources(int device, const rd_line_source_desc* host, const rd_line_source_desc* dev, int n, uint8_t* scratch,
                             int64_t scratch_bytes, hipStream_t s, std::string& err);
// resize + normalise of n sources of any sizes in one launch (kernels_resize_sources.hip): include/rapiddoc_mi355.h
// rd_preproc_resize_norm_sources.  `host` / `dev`: the same descriptors on the host (checked, resize_sources_check.h) and on the device
// (read by the kernel).  Returns 0, or 1 with the message in `err` and nothing launched.
int launch_preproc_resize_norm_sources(int device, const rd_resize_source_desc* host, const rd_resize_source_desc* dev, int n, const float mean[3],
                                       const float std[3], float scale, int interp, int swap_rb, float* out, int64_t out_floats, hipStream_t s,
                                       std::string& err);
// CTC greedy decode on the device: idx / prob [B][T] -> per line (row stride row_bytes): int32 n_text_bytes, float32
// confidence (numpy float32 mean of the kept probabilities), int32 n_kept, int32 0, UTF-8 text.  ctab: [n_classes][1 + max_len]
// bytes (length, then the entry's UTF-8 bytes).
// box_score_fast of the DB post-process candidates (kernels_image.hip), used by launch_db_boxes
int launch_db_scores(const float* prob, int B, int H, int W, const void* cand, const int32_t* n_cand, int max_cand, double* scores, hipStream_t s);
// checkbox detection on the device (kernels_checkbox.hip): include/rapiddoc_mi355.h rd_checkbox_workspace / rd_checkbox_detect_device.
// The launcher returns 0, or 1 with the message in `err` and nothing launched.
size_t checkbox_workspace_bytes(int P, int H, int W, int max_runs, int max_cand, size_t* offsets);
int launch_checkbox_detect(int device, const uint8_t* pages, int P, int H, int W, int bgr, int max_runs, int max_cand, void* ws, size_t ws_bytes,
                           rd_checkbox_page* hdr, rd_checkbox_cand* cands, hipStream_t s, std::string& err);
void launch_checkbox_bin(const uint8_t* pages, int P, int H, int W, int bgr, uint64_t* bin, hipStream_t s);      // the threshold kernel alone
// its host half (checkbox_host.cpp): 0, or 1 / 2 / 3 as rd_checkbox_finish documents, the message in `err`
int checkbox_finish(const rd_checkbox_cand* cands, int n, int H, int W, rd_checkbox_box* out, int max_out, int32_t* n_out, std::string& err);
// region composition on the device (kernels_region.hip): include/rapiddoc_mi355.h rd_region_canvases_workspace / rd_region_canvases.
// The launcher returns 0, or 1 with the message in `err` and nothing launched.
size_t region_canvases_workspace_bytes(int n, int gh, int gw);
int launch_region_canvases(int device, const rd_region_desc* descs, int n, const int32_t* pts, const int32_t* boxes, int gh, int gw, uint8_t* canv,
                           uint8_t* det, void* ws, size_t ws_bytes, hipStream_t s, std::string& err);
// canvases from uploaded host crops (kernels_stage.hip): include/rapiddoc_mi355.h rd_stage_canvases.  `host` / `dev`: the same descriptors on
// the host (checked here) and on the device (read by the kernel).  Returns 0, or 1 with the message in `err` and nothing launched.
int launch_stage_canvases(int device, const rd_stage_desc* host, const rd_stage_desc* dev, int n, hipStream_t s, std::string& err);
// polygon_ops.cpp: the external contours of a u8 mask, last found first; `none` = CHAIN_APPROX_NONE, else CHAIN_APPROX_SIMPLE
void find_external_contours(const uint8_t* mask, int h, int w, bool none, std::vector<std::vector<int32_t>>& xy_out);

// the whole DB post-process on the device (kernels_dbpost.hip): include/rapiddoc_mi355.h rd_db_boxes_device
size_t db_boxes_workspace_bytes(int B, int H, int max_runs, int max_cand);
int launch_db_boxes(const float* prob, int B, int H, int W, const int32_t* src_hw_dev, float thresh, float box_thresh, float unclip_ratio,
                    int dilate, int max_cand, int max_runs, void* ws, size_t ws_bytes, void* out_boxes, int max_out, int32_t* n_out_dev,
                    hipStream_t s);
int launch_ctc_collapse(const int32_t* idx, const float* prob, int B, int T, const int32_t* seg, const uint8_t* ctab, int max_len, int n_classes,
                        uint8_t* out, int row_bytes, uint16_t* kept_cols, float* kept_conf, hipStream_t s);

}  // namespace rd

namespace rd {
void split_weights_h3(const float* w, int rows, int K, std::vector<uint16_t>& hi, std::vector<uint16_t>& lo);
// Fused PPLCNetV4 channel mixer for residual ("rep") blocks (rec_lcnetv4.py:226-236):
//   X' = X * gate            (optional SE gate, per sample and channel)
//   Y  = X' + W2 . GELU(W1 . X' + b1) + b2      W1: [2C][C], W2: [C][2C]  (BN folded)
// The [M][2C] hidden activation never leaves the CU.  C in {48, 96, 192}.
struct MixerParams {
    const float* x; int xld;
    float* y; int yld;
    int M, HW, C;
    const float* gate;   // [N][C] or nullptr
    const float* w1; const float* b1; const float* w2; const float* b2;
    // RD_PRECISION=h3 only: fp16 (hi, lo) splits of w1 [2C][C] and of w2 [C][2C] (hidden columns permuted per 32-chunk)
    const uint16_t* w1h = nullptr; const uint16_t* w1l = nullptr; const uint16_t* w2h = nullptr; const uint16_t* w2l = nullptr;
    unsigned* range_flag = nullptr;   // raised when a split operand leaves the fp16 range (|v| >= 65504)
    int dbg = 0;   // microbenchmark ablation bits (h3 kernel): 1 no GELU, 2 no weight streaming, 4 skip GEMM1, 8 skip GEMM2
    float ws_inv1 = 1.f, ws_inv2 = 1.f;   // ws kernel: inverse power-of-two scales of its weight stream image
    bool ws_pf = false;                   // ws kernel (C = 192): tile prefetch into the X registers, residual folded into the accumulator
    // resident-weights kernel (kernels_mixer_res.hip) only: the block's depthwise 3x3 / stride 1 / pad 1 computed in the tile load (round 6).
    // x is then the block's INPUT [N][dwH][dwW][xld]; dw_w [9][C] (tap-major) and dw_b [C] as Builder::dwconv folds them; dw_line_w as
    // DwParams::line_w (per-image valid width, or nullptr)
    const float* dw_w = nullptr; const float* dw_b = nullptr;
    int dwH = 0, dwW = 0;
    const int32_t* dw_line_w = nullptr; int dw_line_w_stride = 0;
};
bool mixer_fused_supported(int C);
bool mixer_res_fuses_dw(int C);      // kernels_mixer_res.hip: the block's depthwise 3x3 computed in the tile load (round 6)
void launch_mixer_fused_h3(const MixerParams& p, hipStream_t s);
void prepare_mixer_weights_h3(const float* w1, const float* w2, int C, std::vector<uint16_t>& w1h, std::vector<uint16_t>& w1l,
                              std::vector<uint16_t>& w2h, std::vector<uint16_t>& w2l);
void launch_mixer_fused(const MixerParams& p, hipStream_t s);
// round-2 weight-streaming variant (kernels_mixer_ws.hip; C = 96 / 192): activations in registers, LDS = weight stream only,
// persistent 8-wavefront workgroups.  p.w1h carries the stream image built by prepare_mixer_weights_ws.
bool mixer_ws_supported(int C);
bool mixer_ws_preferred(int C);   // where it measures faster than the round-1 kernel
void prepare_mixer_weights_ws(const float* w1, const float* w2, int C, std::vector<uint16_t>& img, float inv[2]);
bool mixer_ws_prefetch();             // RD_WS_PF (default 1): the engine launches the prefetching form of the ws kernel
void launch_mixer_fused_ws(const MixerParams& p, hipStream_t s);
void launch_mixer_debug(const MixerParams& p, int variant, hipStream_t s);
// resident-weights variant for the narrow blocks (kernels_mixer_res.hip; C = 96): all split weights in LDS, 16 independent
// wavefronts per CU.  p.w1h carries the fragment image built by prepare_mixer_weights_res.
bool mixer_res_supported(int C);
void prepare_mixer_weights_res(const float* w1, const float* w2, int C, std::vector<uint16_t>& img, float inv[2]);   // inv -> ws_inv1 / ws_inv2
void launch_mixer_fused_res(const MixerParams& p, hipStream_t s);
}  // namespace rd
