// The developer entries of librapiddoc_mi355.so (rd_debug_*): single kernels and plan variants with taps, for the tests, tools/ and the
// micro-benchmarks.  None of them is part of the public header; the product C surface is api.cpp.
#include <algorithm>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "api_handle.h"
#include "builder_util.h"
#include "region_geom.h"

extern "C" {

// shared by the timing entries below: one untimed launch (so `iters` = 0 still runs the kernel once: the correctness tests rely on
// that), `after_first` (when given: what an entry launches once behind it, untimed), then `iters` timed launches between two events;
// ms per timed launch.  A developer tool: HIP return codes are not looked at
static float rd_debug_time(int iters, const std::function<void()>& launch, const std::function<void()>& after_first = nullptr) {
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    launch();
    if (after_first) after_first();
    (void)hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters; ++i) launch();
    (void)hipEventRecord(e1, nullptr);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return iters > 0 ? ms / iters : 0.f;
}

// developer entry ("ppocrv3_det_mobile" only): rd_det_forward plus `fuse` and the backbone's four stage features, written as NCHW back to
// back into aux_dev: [B,96,H/4,W/4], [B,16,H/4,W/4], [B,24,H/8,W/8], [B,56,H/16,W/16], [B,480,H/32,W/32].  The plan of the engine's
// DET_WANT_NECK | DET_WANT_STAGES variant; the internal workspace.  Not part of the public header.
int rd_debug_det_forward_stages(rd_handle* h, const float* x, int B, int H, int W, float* prob, float* aux, void* stream) {
    return guarded(h, [&] {
        RD_CHECK(h->eng && h->eng->kind() == "ppocrv3_det_mobile", "handle is not a ppocrv3_det_mobile model");
        RD_CHECK(x && prob && aux && B > 0 && H > 0 && W > 0 && H % 32 == 0 && W % 32 == 0, "null input/output, or H / W no multiple of 32");
        static const int kC[5] = {96, 16, 24, 56, 480}, kR[5] = {4, 4, 8, 16, 32};
        std::vector<void*> ext = {(void*)x, (void*)prob};
        float* q = aux;
        for (int i = 0; i < 5; ++i) {
            ext.push_back(q);
            q += (size_t)B * kC[i] * (H / kR[i]) * (W / kR[i]);
        }
        h->eng->run(B, H, W, rd::DET_WANT_NECK | rd::DET_WANT_STAGES, ext, nullptr, 0, (hipStream_t)stream);
    });
}

// developer entry ("ppocr_cls_mobile" only): rd_cls_forward with RD_CLS_WANT_AUX plus the outputs of blocks 0, 3, 8, 10, written as NCHW back
// to back into stages_dev ([B,8,r0,w], [B,16,r1,w], [B,32,r2,w], [B,32,r3,w]: rd::cls_mobile_geometry).  The internal workspace.  Not part
// of the public header.
int rd_debug_cls_forward_stages(rd_handle* h, const float* x, int B, int H, int W, float* prob, float* aux, float* stages, void* stream) {
    return guarded(h, [&] {
        RD_CHECK(h->eng && h->eng->kind() == "ppocr_cls_mobile", "handle is not a ppocr_cls_mobile model");
        RD_CHECK(x && prob && aux && stages && B > 0, "null input/output");
        int rows[4], cols = 0;
        RD_CHECK(rd::cls_mobile_geometry(H, W, rows, &cols), "text-line classifier: H x W leaves an empty map");
        static const int kC[4] = {8, 16, 32, 32};
        std::vector<void*> ext = {(void*)x, (void*)prob, (void*)aux};
        float* q = stages;
        for (int i = 0; i < 4; ++i) {
            ext.push_back(q);
            q += (size_t)B * kC[i] * rows[i] * cols;
        }
        h->eng->run(B, H, W, rd::CLS_WANT_AUX | rd::CLS_WANT_STAGES, ext, nullptr, 0, (hipStream_t)stream);
    });
}

// developer entry ("unitable_decoder"): `steps` decode steps with traces.  forced_dev (int32 [B][steps], or null): the token fed to step t
// of table b (the EOS latch is off); null = the free loop of rd_table_decode.  Traces (device, each may be null): hidden [steps][4][B][768]
// = the row after each block, logits [steps][B][960] (before the whitelist), chosen / emitted int32 [steps][B] = the whitelist argmax and the
// token after the bbox rule.  Rows of steps the loop did not run stay as they were.  Not part of the public header.
int rd_debug_table_decode(rd_handle* h, const float* memory, int B, int S, int steps, const rd_table_decode_cfg* cfg, const int32_t* forced,
                          int64_t* ids, float* trace_hidden, float* trace_logits, int32_t* trace_chosen, int32_t* trace_emitted, void* stream) {
    return guarded(h, [&] {
        RD_CHECK(h->kind == "unitable_decoder" && h->tdec, "handle is not a loaded table-structure decoder (unitable_decoder)");
        int c[6];
        table_cfg6(cfg, c);
        rd::table_decoder_decode(h->tdec, memory, B, S, steps, c, (long long*)ids, nullptr, (hipStream_t)stream, (const int*)forced, trace_hidden,
                                 trace_logits, (int*)trace_chosen, (int*)trace_emitted);
    });
}

// developer entry ("unitable_decoder"): rd_table_decode_stream plus optional traces written inside the step (graph replay included), indexed
// by what the slot holds: trace_logits [N][max_new_tokens][960] and trace_hidden [N][max_new_tokens][4][768] (the row after each block) by
// (table, position), and trace_sched int32 [sched_steps][slots][2] = the (table or -1, position) of every slot at the start of every step
// (steps past sched_steps are not recorded).  With all three null it enqueues exactly what rd_table_decode_stream enqueues.
int rd_debug_table_decode_stream(rd_handle* h, const float* memory, int N, int S, int max_new_tokens, int slots, const rd_table_decode_cfg* cfg,
                                 int64_t* ids, int32_t* lens, rd_table_stream_stats* stats, void* stream, float* trace_logits, float* trace_hidden,
                                 int32_t* trace_sched, int sched_steps) {
    return guarded(h, [&] {
        RD_CHECK(h->kind == "unitable_decoder" && h->tdec, "handle is not a loaded table-structure decoder (unitable_decoder)");
        int c[6];
        table_cfg6(cfg, c);
        rd::table_decoder_decode_stream(h->tdec, memory, N, S, max_new_tokens, slots, c, (long long*)ids, (int*)lens, stats, (hipStream_t)stream,
                                        trace_logits, trace_hidden, (int*)trace_sched, sched_steps);
    });
}

// developer entry ("unitable_encoder" only): rd_table_encoder_forward plus three taps, each [B,T,768], back to back in taps_dev: the patch
// embedding (before the position rows) and the outputs of encoder layers 0 and 11.  The plan of the engine's VIT_WANT_TAPS variant; the
// internal workspace.  Not part of the public header.
int rd_debug_table_encoder_taps(rd_handle* h, const float* x, int B, int H, int W, float* memory, float* taps, void* stream) {
    return guarded(h, [&] {
        RD_CHECK(h->eng && h->eng->kind() == "unitable_encoder", "handle is not a unitable_encoder model");
        RD_CHECK(x && memory && taps && B > 0 && H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0, "null input/output, or H / W no multiple of 16");
        const size_t n = (size_t)B * (H / 16) * (W / 16) * 768;
        h->eng->run(B, H, W, rd::VIT_WANT_TAPS, {(void*)x, (void*)memory, (void*)taps, (void*)(taps + n), (void*)(taps + 2 * n)}, nullptr, 0, (hipStream_t)stream);
    });
}

// developer entry: rd_formula_decode plus two optional traces written inside every step (graph replay included): the step's logits
// trace_logits [max_new_tokens][B][V] and the hidden row in front of the final LayerNorm trace_hidden [max_new_tokens][B][512].  With both
// null it enqueues exactly what rd_formula_decode enqueues.
int rd_debug_formula_decode(rd_handle* h, const float* enc, int B, int S, int max_new_tokens, int64_t* ids, int32_t* n_cols, void* stream,
                            float* trace_logits, float* trace_hidden) {
    return guarded(h, [&] {
        RD_CHECK(h->kind == "ppformulanet_head" && h->dec, "handle is not a loaded ppformulanet_head model");
        RD_CHECK(enc && ids && n_cols, "null input/output");
        *n_cols = rd::formula_decoder_decode(h->dec, enc, B, S, max_new_tokens, reinterpret_cast<long long*>(ids), (hipStream_t)stream,
                                             trace_logits, trace_hidden);
    });
}

// developer entry: rd_formula_decode_stream plus optional traces written inside the step (graph replay included), indexed by what the slot
// holds: trace_logits [N][max_new_tokens][V] and trace_hidden [N][max_new_tokens][512] by (formula, position), and trace_sched int32
// [sched_steps][slots][2] = the (formula or -1, position) of every slot at the start of every step (steps past sched_steps are not recorded).
// With all three null it enqueues exactly what rd_formula_decode_stream enqueues.
int rd_debug_formula_decode_stream(rd_handle* h, const float* enc, int N, int S, int max_new_tokens, int slots, int64_t* ids, int32_t* lens,
                                   rd_formula_stream_stats* stats, void* stream, float* trace_logits, float* trace_hidden, int32_t* trace_sched,
                                   int sched_steps) {
    return guarded(h, [&] {
        RD_CHECK(h->kind == "ppformulanet_head" && h->dec, "handle is not a loaded ppformulanet_head model");
        RD_CHECK(enc && ids && lens, "null input/output");
        RD_CHECK(!trace_sched || sched_steps > 0, "trace_sched needs sched_steps > 0");
        rd::formula_decoder_decode_stream(h->dec, enc, N, S, max_new_tokens, slots, reinterpret_cast<long long*>(ids), (int*)lens, stats,
                                          (hipStream_t)stream, trace_logits, trace_hidden, (int*)trace_sched, sched_steps);
    });
}

// developer entry (host only): the per-axis tables rd_preproc_resize_aa_norm uploads.  bounds_out int32 [out][2], kk_out int32 [out][ksize]
// with kk_cap entries of room; returns ksize, or -1 on bad arguments / too little room.
int rd_debug_resize_aa_coeffs(int in, int out, int32_t* bounds_out, int32_t* kk_out, int64_t kk_cap) {
    if (in < 1 || out < 1 || in > RD_RESIZE_AA_MAX_SIDE || out > RD_RESIZE_AA_MAX_SIDE || !bounds_out || !kk_out) return -1;
    std::vector<int32_t> bounds, kk;
    const int ksize = rd::resize_aa_coeffs(in, out, bounds, kk);
    if ((int64_t)kk.size() > kk_cap) return -1;
    std::copy(bounds.begin(), bounds.end(), bounds_out);
    std::copy(kk.begin(), kk.end(), kk_out);
    return ksize;
}

// developer entry (host only): the same for a filter (RD_RESAMPLE_BILINEAR / RD_RESAMPLE_BICUBIC) sampled over the box [box0, box1) of the
// `in` source pixels: the tables of the formula pre-process (rd_formula_preproc_batch hands over box0 = 0 and a float32 box1).
int rd_debug_resample_coeffs(int filter, int in, double box0, double box1, int out, int32_t* bounds_out, int32_t* kk_out, int64_t kk_cap) {
    if ((filter != RD_RESAMPLE_BILINEAR && filter != RD_RESAMPLE_BICUBIC) || in < 1 || out < 1 || in > RD_RESIZE_AA_MAX_SIDE ||
        out > RD_RESIZE_AA_MAX_SIDE || !(box0 >= 0.0) || !(box1 > box0) || !(box1 <= (double)in) || !bounds_out || !kk_out)
        return -1;
    std::vector<int32_t> bounds, kk;
    const int ksize = rd::resample_coeffs(filter, in, box0, box1, out, bounds, kk);
    if ((int64_t)kk.size() > kk_cap) return -1;
    std::copy(bounds.begin(), bounds.end(), bounds_out);
    std::copy(kk.begin(), kk.end(), kk_out);
    return ksize;
}

// developer entry (host only, no HIP call): the keep mask of rd_region_canvases for ONE polygon on an h x w window, from the functions of
// region_geom.h that the device evaluates - out_u8 [h][w] = 1 where cv2.fillPoly(mask, [pts], 1) sets the pixel.  pts int32 [n][2] in
// window coordinates.  Returns 0, or -1 on bad arguments (n above RD_REGION_MAX_POLY included).
int rd_debug_region_keep_mask(int h, int w, const int32_t* pts, int n, uint8_t* out_u8) {
    if (h < 1 || w < 1 || n < 0 || n > RD_REGION_MAX_POLY || (n > 0 && !pts) || !out_u8) return -1;
    rd_region::Edge edges[rd_region::kMaxPoly];
    for (int t = 0; t < n; ++t) {
        const int32_t* p = pts + 2 * (t == 0 ? n - 1 : t - 1);
        edges[t] = rd_region::make_edge(p[0], p[1], pts[2 * t], pts[2 * t + 1]);
    }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) out_u8[(size_t)y * w + x] = rd_region::keep(edges, n, x, y) ? 1 : 0;
    return 0;
}

// ---- developer micro-benchmarks (not part of the public header): time one kernel on caller-provided buffers
float rd_debug_time_mixer(int C, int M, int variant, int iters, float* x, float* y, float* w1, float* b1, float* w2, float* b2) {
    rd::MixerParams p{};
    p.x = x; p.xld = C; p.y = y; p.yld = C; p.M = M; p.HW = M; p.C = C; p.gate = nullptr;
    p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    void* hbuf[4] = {nullptr, nullptr, nullptr, nullptr};
    int ws_abl = 0;                       // 1000 + 256 * bits: ablations of the ws kernel (C = 192, results are garbage)
    if (variant >= 1000) { ws_abl = (variant - 1000) & ~0xff; variant = 200 + ((variant - 1000) & 0xff); }
    if (variant >= 600) variant -= 300;   // (600+ = 300+: keeps the resident-weights variants clear of the 400..599 PF range)
    if (variant >= 300 && variant < 400) {  // resident-weights split mixer (kernels_mixer_res.hip)
        std::vector<float> hw1((size_t)2 * C * C), hw2((size_t)2 * C * C);
        (void)hipMemcpy(hw1.data(), w1, hw1.size() * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hw2.data(), w2, hw2.size() * 4, hipMemcpyDeviceToHost);
        std::vector<uint16_t> img;
        float inv[2];
        rd::prepare_mixer_weights_res(hw1.data(), hw2.data(), C, img, inv);
        p.ws_inv1 = inv[0]; p.ws_inv2 = inv[1];
        (void)hipMalloc(&hbuf[0], img.size() * 2);
        (void)hipMemcpy(hbuf[0], img.data(), img.size() * 2, hipMemcpyHostToDevice);
        p.w1h = (const uint16_t*)hbuf[0];
    } else if (variant >= 200) {  // weight-streaming split mixer (kernels_mixer_ws.hip); 400+: the prefetching form (PF)
        const bool pf = variant >= 400 && variant < 600;
        if (pf) variant -= 200;
        p.ws_pf = pf;
        p.dbg = (variant - 200) | ws_abl;
        std::vector<float> hw1((size_t)2 * C * C), hw2((size_t)2 * C * C);
        (void)hipMemcpy(hw1.data(), w1, hw1.size() * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hw2.data(), w2, hw2.size() * 4, hipMemcpyDeviceToHost);
        std::vector<uint16_t> img;
        float inv[2];
        rd::prepare_mixer_weights_ws(hw1.data(), hw2.data(), C, img, inv);
        p.ws_inv1 = inv[0]; p.ws_inv2 = inv[1];
        (void)hipMalloc(&hbuf[0], img.size() * 2);
        (void)hipMemcpy(hbuf[0], img.data(), img.size() * 2, hipMemcpyHostToDevice);
        p.w1h = (const uint16_t*)hbuf[0];
    } else if (variant >= 100) {  // fp16x3 mixer (+ ablation bits)
        p.dbg = variant - 100;
        std::vector<float> hw1((size_t)2 * C * C), hw2((size_t)2 * C * C);
        (void)hipMemcpy(hw1.data(), w1, hw1.size() * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hw2.data(), w2, hw2.size() * 4, hipMemcpyDeviceToHost);
        std::vector<uint16_t> v[4];
        rd::prepare_mixer_weights_h3(hw1.data(), hw2.data(), C, v[0], v[1], v[2], v[3]);
        for (int i = 0; i < 4; ++i) {
            (void)hipMalloc(&hbuf[i], v[i].size() * 2);
            (void)hipMemcpy(hbuf[i], v[i].data(), v[i].size() * 2, hipMemcpyHostToDevice);
        }
        p.w1h = (const uint16_t*)hbuf[0]; p.w1l = (const uint16_t*)hbuf[1];
        p.w2h = (const uint16_t*)hbuf[2]; p.w2l = (const uint16_t*)hbuf[3];
    }
    auto go = [&] {
        if (variant >= 300 && !p.ws_pf) rd::launch_mixer_fused_res(p, nullptr);
        else if (variant >= 200) rd::launch_mixer_fused_ws(p, nullptr);
        else if (variant >= 100) rd::launch_mixer_fused_h3(p, nullptr);
        else rd::launch_mixer_debug(p, variant, nullptr);
    };
    go();
    (void)hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters; ++i) go();
    (void)hipEventRecord(e1, nullptr);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    for (void* b : hbuf) if (b) (void)hipFree(b);
    return ms / iters;
}
// h1 image of device weights w [N][K] (single-accumulator split GEMM, kernels_gemm_h1.hip): uploaded into fresh device buffers
static bool debug_h1_image(const float* w_dev, int N, int K, void** img_dev, float* inv) {
    if (!rd::gemm_h1_shape_ok(K, N)) return false;
    std::vector<float> hw((size_t)N * K);
    if (hipMemcpy(hw.data(), w_dev, hw.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
    std::vector<uint16_t> img;
    *inv = rd::prepare_gemm_h1_weights(hw.data(), N, K, img);
    if (hipMalloc(img_dev, img.size() * 2) != hipSuccess) return false;
    (void)hipMemcpy(*img_dev, img.data(), img.size() * 2, hipMemcpyHostToDevice);
    return true;
}
float rd_debug_time_gemm(int M, int K, int N, int act, int iters, float* x, float* w, float* b, float* y, void* wh, void* wl) {
    rd::ConvParams p{};
    p.wh = (const uint16_t*)wh; p.wl = (const uint16_t*)wl;
    p.x = x; p.xld = K; p.N = 1; p.H = 1; p.W = M; p.Cin = K; p.w = w; p.bias = b; p.y = y; p.yld = N;
    p.OH = 1; p.OW = M; p.Cout = N; p.KH = p.KW = p.SH = p.SW = 1; p.act = act; p.out_mode = rd::OUT_NHWC;
    p.M = M; p.K = K; p.Ng = N;
    void* img = nullptr;
    float inv = 0.f;
    if (wh && debug_h1_image(w, N, K, &img, &inv)) { p.w1 = (const uint16_t*)img; p.w1_inv = inv; }   // as the engine prepares it
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    auto go = [&] { if (wh) rd::launch_conv_igemm_h3(p, nullptr); else rd::launch_conv_igemm(p, nullptr); };
    go();
    (void)hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters; ++i) go();
    (void)hipEventRecord(e1, nullptr);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (img) (void)hipFree(img);
    return ms / iters;
}
// developer entry: the single-accumulator split GEMM alone, with strides, residual and the range flag:
// y[M][yld] = act(x[M][xld(K used)] * w[N][K]^T + b) + res[M][rld].  Returns ms per launch, or -1 when the kernel does not take the shape.
// *range_out (optional) receives 1 when the kernel raised its range flag.
float rd_debug_gemm_h1(int M, int K, int N, int act, int iters, float* x, int xld, float* w, float* b, float* res, int rld, float* y, int yld,
                       int* range_out) {
    rd::ConvParams p{};
    p.x = x; p.xld = xld; p.N = 1; p.H = 1; p.W = M; p.Cin = K; p.w = w; p.bias = b; p.y = y; p.yld = yld;
    p.OH = 1; p.OW = M; p.Cout = N; p.KH = p.KW = p.SH = p.SW = 1; p.act = act; p.out_mode = rd::OUT_NHWC;
    p.res = res; p.rld = rld;
    p.M = M; p.K = K; p.Ng = N;
    void* img = nullptr;
    float inv = 0.f;
    if (!debug_h1_image(w, N, K, &img, &inv)) return -1.f;
    p.w1 = (const uint16_t*)img; p.w1_inv = inv;
    unsigned* flag = nullptr;
    (void)hipHostMalloc((void**)&flag, sizeof(unsigned), hipHostMallocMapped);
    *flag = 0;
    p.range_flag = flag;
    float ms = -1.f;
    if (rd::gemm_h1_applies(p)) ms = rd_debug_time(iters, [&] { rd::launch_gemm_h1(p, nullptr); });
    (void)hipDeviceSynchronize();
    if (range_out) *range_out = (int)*flag;
    (void)hipHostFree(flag);
    (void)hipFree(img);
    return ms;
}

// developer entry: the 1 x 3 sequence convolution alone (kernels_seqconv.hip).  x0 [M][ld0] / x1 [M][ld1] (or null) = the two K segments,
// w [N][3 (C0 + C1)] fp32 in the kernel's order (tap, then segment 0 | segment 1 channels), tokinfo [M] (or null: uniform lines of T
// tokens), split != 0: the split-fp16 route (the weights are split here the way the engine splits them), else native fp32.
// Returns ms per launch (iters timed launches after one untimed), or -1 when the kernel does not take the shape.
float rd_debug_seqconv(int M, int C0, int C1, int N, int T, int act, int split, int iters, float* x0, int ld0, float* x1, int ld1, float* w, float* b,
                       const int32_t* tokinfo, float* y, int yld, int* range_out) {
    if (M <= 0 || !rd::seqconv_shape_ok(C0, C1, N) || ld0 % 4 || ld1 % 4 || (!tokinfo && T <= 0)) return -1.f;
    rd::SeqConvParams p{};
    p.x0 = x0; p.ld0 = ld0; p.C0 = C0; p.x1 = C1 ? x1 : nullptr; p.ld1 = C1 ? ld1 : 0; p.C1 = C1;
    p.w = w; p.bias = b; p.y = y; p.yld = yld; p.M = M; p.N = N; p.T = T; p.tokinfo = tokinfo; p.act = act;
    const int K = 3 * (C0 + C1);
    void *dh = nullptr, *dl = nullptr;
    unsigned* flag = nullptr;
    (void)hipHostMalloc((void**)&flag, sizeof(unsigned), hipHostMallocMapped);
    *flag = 0;
    if (split) {
        std::vector<float> hw((size_t)N * K);
        if (hipMemcpy(hw.data(), w, hw.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1.f;
        std::vector<uint16_t> hi, lo;
        rd::split_weights_h3(hw.data(), N, K, hi, lo);
        if (hipMalloc(&dh, hi.size() * 2) != hipSuccess || hipMalloc(&dl, lo.size() * 2) != hipSuccess) return -1.f;
        (void)hipMemcpy(dh, hi.data(), hi.size() * 2, hipMemcpyHostToDevice);
        (void)hipMemcpy(dl, lo.data(), lo.size() * 2, hipMemcpyHostToDevice);
        p.wh = (const uint16_t*)dh; p.wl = (const uint16_t*)dl;
        p.range_flag = flag;
    }
    float ms = rd_debug_time(iters, [&] { rd::launch_seqconv(p, nullptr); });
    (void)hipDeviceSynchronize();
    if (hipGetLastError() != hipSuccess) ms = -1.f;
    if (range_out) *range_out = (int)*flag;
    (void)hipHostFree(flag);
    if (dh) (void)hipFree(dh);
    if (dl) (void)hipFree(dl);
    return ms;
}

// developer entry: the fused local tail of PFHeadLocal alone (kernels_det_local.hip).  Device pointers: f NHWC [N][H/2][W/2][64], shrink
// [N][H][W], w3 = last_3's folded weights [64][65][3][3] (input channel 0 = shrink), b3 [64], w1 [64], y [N][H][W]; split != 0: the
// split-fp16 route, else native fp32.  Returns ms per launch (iters timed launches after one untimed), or -1 for a geometry it does not take.
float rd_debug_det_local(int N, int H, int W, int split, int iters, float* f, float* shrink, float* w3, float* b3, float* w1, float b1, float* y,
                         int* range_out) {
    if (N <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return -1.f;
    std::vector<float> hw((size_t)64 * 65 * 9);
    if (hipMemcpy(hw.data(), w3, hw.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1.f;
    std::vector<float> img32;
    std::vector<uint16_t> img16;
    const float inv = rd::prepare_det_local_weights(hw.data(), img32, img16);
    void *d32 = nullptr, *d16 = nullptr;
    if (hipMalloc(&d32, img32.size() * 4) != hipSuccess || hipMalloc(&d16, img16.size() * 2) != hipSuccess) return -1.f;
    (void)hipMemcpy(d32, img32.data(), img32.size() * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(d16, img16.data(), img16.size() * 2, hipMemcpyHostToDevice);
    unsigned* flag = nullptr;
    (void)hipHostMalloc((void**)&flag, sizeof(unsigned), hipHostMallocMapped);
    *flag = 0;
    rd::DetLocalParams p{};
    p.f = f; p.fld = 64; p.shrink = shrink; p.y = y; p.N = N; p.H = H; p.W = W;
    p.wimg32 = (const float*)d32; p.b3 = b3; p.w1 = w1; p.b1 = b1;
    if (split) { p.wimg16 = (const uint16_t*)d16; p.w_inv = inv; p.range_flag = flag; }
    float ms = rd_debug_time(iters, [&] { rd::launch_det_local(p, nullptr); });
    (void)hipDeviceSynchronize();
    if (hipGetLastError() != hipSuccess) ms = -1.f;
    if (range_out) *range_out = (int)*flag;
    (void)hipHostFree(flag);
    (void)hipFree(d32);
    (void)hipFree(d16);
    return ms;
}

// what rd_debug_conv reports in *used_direct for a route
static int debug_conv_code(rd::ConvRoute r) {
    return r == rd::CONV_DIRECT ? 1 : r == rd::CONV_STREAM ? 2 : r == rd::CONV_C3H1 ? 3 : r == rd::CONV_C9H1 ? 4 : 0;
}
static void debug_copy_name(const char* s, char* name, int name_len) {
    if (name && name_len > 0) { std::strncpy(name, s, (size_t)name_len - 1); name[name_len - 1] = 0; }
}

// developer entry, host only (no HIP call): the route of a dense convolution as the planner decides it.  Geometry as rd_debug_conv with a dense
// input (xld = Cin), N images; images: bit 0 the (hi, lo) split weights, 1 the one-accumulator GEMM image, 2 the 3x3 image, 3 the 9x9 image,
// 4 the wide 3x3 image a builder's opt-in hands out (Builder::set_conv3x3_wide; asked without a residual, as those layers are)
// (only bits are looked at: the images themselves are not); split = 0 asks conv_f32_route, with allow_skinny.  The route's name goes to
// name[name_len]; returns the code rd_debug_conv reports for the route in *used_direct, -1 on a bad argument.
int rd_debug_conv_route(int N, int H, int W, int Cin, int Cout, int KH, int KW, int S, int PT, int PL, int PB, int PR, int act, int images,
                        int has_ascale, int allow_skinny, int split, char* name, int name_len) {
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || S <= 0) return -1;
    static const uint16_t image[8] = {};       // something for the image pointers to point at
    rd::ConvParams p{};
    p.xld = Cin; p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.yld = Cout;
    p.OH = (H + PT + PB - KH) / S + 1; p.OW = (W + PL + PR - KW) / S + 1; p.Cout = Cout;
    p.KH = KH; p.KW = KW; p.SH = p.SW = S; p.PT = PT; p.PL = PL; p.act = act; p.out_mode = rd::OUT_NHWC; p.rld = Cout;
    p.M = N * p.OH * p.OW; p.K = KH * KW * Cin; p.Ng = Cout;
    p.allow_skinny = allow_skinny;
    if (images & 1) p.wh = p.wl = image;
    if (images & 2) { p.w1 = image; p.w1_inv = 1.f; }
    if (images & 4) { p.w3 = image; p.w3_inv = 1.f; }
    if (images & 8) { p.w9 = image; p.w9_inv = 1.f; }
    if (images & 16) { p.w3w = image; p.w3w_inv = 1.f; p.rld = 0; }
    const rd::ConvRoute r = split ? rd::conv_split_route(p, has_ascale != 0) : rd::conv_f32_route(p);
    debug_copy_name(rd::conv_route_name(r), name, name_len);
    return debug_conv_code(r);
}

// a host array as a fresh device buffer (freed by the entry that made it)
static bool debug_upload(const void* src, size_t bytes, void** dev) {
    if (hipMalloc(dev, bytes) != hipSuccess) return false;
    return hipMemcpy(*dev, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
}

// `force` of rd_debug_conv_ex: the staged tile of that name in the precision asked for
static bool debug_conv_tile(const char* force, int split, rd::ConvRoute* r) {
    static const rd::ConvRoute h3[] = {rd::CONV_H3_256x128, rd::CONV_H3_128x96, rd::CONV_H3_256x64, rd::CONV_H3_128x32, rd::CONV_H3_128x64};
    static const rd::ConvRoute f32[] = {rd::CONV_F32_128x32, rd::CONV_F32_128x64, rd::CONV_F32_128x96, rd::CONV_F32_128x128};
    const rd::ConvRoute* t = split ? h3 : f32;
    for (int i = 0, n = split ? 5 : 4; i < n; ++i)
        if (std::strcmp(force, rd::conv_route_name(t[i])) == 0) { *r = t[i]; return true; }
    return false;
}

// what rd_debug_conv hands to the body it shares with rd_debug_conv_ex: the caller's own split planes instead of the ones prepared here, and
// its route code (*used_direct on entry: 1 the direct k x k kernel, 2 the streaming one, 4 the 9x9 one, where they support the geometry)
struct DebugConvOld {
    const void* wh; const void* wl;
    int code;
};

// the body of rd_debug_conv_ex (its comment says what the arguments mean); *route_out receives the route launched
static float debug_conv_run(int N, int H, int W, int Cin, int Cout, int KH, int KW, int SH, int SW, int PT, int PL, int PB, int PR, int act, int xld,
                            int yld, int rld, int out_mode, int split, int images, int allow_skinny, int iters, float* x, float* w, float* bias,
                            float* res, float* y, const float* dscale, const float* dshift, const float* ln_g, const float* ln_b, const float* ascale,
                            const char* force, const DebugConvOld* old, rd::ConvRoute* route_out, int* range_out) {
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || SH <= 0 || SW <= 0 || PT < 0 || PL < 0 || PB < 0 || PR < 0) return -1.f;
    if (!x || !w || !y || H + PT + PB < KH || W + PL + PR < KW) return -1.f;
    if (Cin % 4 != 0 || xld % 4 != 0 || xld < Cin || yld < Cout || (res && rld < Cout)) return -1.f;     // (Cin % 4: as Builder::conv)
    const bool deconv = out_mode == rd::OUT_DECONV2X2;
    if (out_mode != rd::OUT_NHWC && !deconv) return -1.f;
    if (deconv && (res || KH != 1 || KW != 1 || SH != 1 || SW != 1 || PT || PL || PB || PR)) return -1.f;
    if ((ln_g != nullptr) != (ln_b != nullptr)) return -1.f;
    rd::ConvParams p{};
    p.x = x; p.xld = xld; p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.w = w; p.bias = bias; p.y = y; p.yld = yld;
    p.OH = rd::out_dim(H, KH, SH, PT, PB); p.OW = rd::out_dim(W, KW, SW, PL, PR); p.Cout = Cout;
    p.KH = KH; p.KW = KW; p.SH = SH; p.SW = SW; p.PT = PT; p.PL = PL; p.act = act; p.out_mode = out_mode;
    p.res = res; p.rld = rld; p.ascale = ascale; p.ln_g = ln_g; p.ln_b = ln_b; p.allow_skinny = allow_skinny;
    p.M = N * p.OH * p.OW; p.K = KH * KW * Cin; p.Ng = deconv ? 4 * Cout : Cout;
    std::vector<void*> owned;                  // device buffers of this call
    unsigned* flag = nullptr;
    auto done = [&](float ms) {
        (void)hipDeviceSynchronize();
        if (flag) {
            if (range_out) *range_out = (int)*flag;
            (void)hipHostFree(flag);
        }
        for (void* b : owned) (void)hipFree(b);
        return ms;
    };
    auto upload = [&](const auto& v, void** dev) {
        const bool ok = debug_upload(v.data(), v.size() * sizeof(v[0]), dev);
        if (*dev) owned.push_back(*dev);
        return ok;
    };
    // the weights as the engine holds them: [Ng][K] on the host for the images, the deconvolution's repacked from its checkpoint layout
    const bool want_images = split && !(old && old->wh);
    std::vector<float> hw;
    if (deconv) {
        std::vector<float> ck((size_t)Cin * Cout * 4), hb(Cout), sc(Cout, 1.f), sh(Cout, 0.f), bf;
        if (hipMemcpy(ck.data(), w, ck.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return done(-1.f);
        if (bias && hipMemcpy(hb.data(), bias, hb.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return done(-1.f);
        if (dscale && hipMemcpy(sc.data(), dscale, sc.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return done(-1.f);
        if (dshift && hipMemcpy(sh.data(), dshift, sh.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return done(-1.f);
        rd::pack_deconv2x2(ck.data(), bias ? hb.data() : nullptr, Cin, Cout, sc.data(), sh.data(), hw, bf);
        void *dw = nullptr, *db = nullptr;
        if (!upload(hw, &dw) || !upload(bf, &db)) return done(-1.f);
        p.w = (const float*)dw; p.bias = (const float*)db;
    } else if (want_images || (split && old && (images & 12))) {
        hw.resize((size_t)p.Ng * p.K);
        if (hipMemcpy(hw.data(), w, hw.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return done(-1.f);
    }
    if (split) {
        if (old && old->wh) {
            p.wh = (const uint16_t*)old->wh; p.wl = (const uint16_t*)old->wl;
        } else {
            if (!rd::fits_fp16_range(hw)) return done(-1.f);
            std::vector<uint16_t> hi, lo;
            rd::split_weights_h3(hw.data(), p.Ng, p.K, hi, lo);
            void *dh = nullptr, *dl = nullptr;
            if (!upload(hi, &dh) || !upload(lo, &dl)) return done(-1.f);
            p.wh = (const uint16_t*)dh; p.wl = (const uint16_t*)dl;
        }
        // the one-accumulator images, prepared the way the engine prepares them for the layers that get one
        std::vector<uint16_t> img;
        void* d = nullptr;
        if ((images & 2) && !deconv && rd::gemm_h1_shape_ok(p.K, p.Ng)) {
            p.w1_inv = rd::prepare_gemm_h1_weights(hw.data(), p.Ng, p.K, img);
            if (!upload(img, &d)) return done(-1.f);
            p.w1 = (const uint16_t*)d;
        }
        if ((images & 4) && !deconv && rd::conv3x3_h1_shape_ok(KH, KW, Cin, Cout)) {
            p.w3_inv = rd::prepare_conv3x3_h1_weights(hw.data(), Cout, Cin, img);
            d = nullptr;
            if (!upload(img, &d)) return done(-1.f);
            p.w3 = (const uint16_t*)d;
        }
        if ((images & 8) && !deconv && rd::conv9x9_h1_shape_ok(KH, KW, Cin, Cout)) {
            p.w9_inv = rd::prepare_conv9x9_h1_weights(hw.data(), Cout, Cin, img);
            d = nullptr;
            if (!upload(img, &d)) return done(-1.f);
            p.w9 = (const uint16_t*)d;
        }
        if ((images & 16) && !deconv && rd::conv3x3_wide_shape_ok(KH, KW, Cin, Cout)) {      // (the opt-in a PPHGNet_small layer carries)
            p.w3w_inv = rd::prepare_conv3x3_wide_weights(hw.data(), Cout, Cin, img);
            d = nullptr;
            if (!upload(img, &d)) return done(-1.f);
            p.w3w = (const uint16_t*)d;
        }
        if (range_out) {
            if (hipHostMalloc((void**)&flag, sizeof(unsigned), hipHostMallocMapped) != hipSuccess) { flag = nullptr; return done(-1.f); }
            *flag = 0;
            p.range_flag = flag;
        }
    } else if (range_out) {
        *range_out = 0;
    }
    rd::ConvRoute route = split ? rd::conv_split_route(p, ascale != nullptr) : rd::conv_f32_route(p);
    if (force) {
        // the staged tiles take any geometry below their 32-bit offsets (the rule of conv_split_route)
        if (!debug_conv_tile(force, split, &route)) return done(-1.f);
        if (split && ((unsigned long long)N * H * W * (unsigned long long)xld >= (1ull << 32) ||
                      (unsigned long long)p.Ng * (unsigned long long)((p.K + 31) & ~31) >= (1ull << 32)))
            return done(-1.f);
    }
    if (old && split && old->code == 2 && rd::conv_stream_h3_supported(p)) route = rd::CONV_STREAM;
    else if (old && split && old->code == 1 && rd::conv_direct_h3_supported(p)) route = rd::CONV_DIRECT;
    if (ln_g && route != rd::CONV_SKINNY) return done(-1.f);        // every other route would drop the LayerNorm
    if (route_out) *route_out = route;
    float ms = -2.f;
    try {
        ms = rd_debug_time(iters, [&] { rd::launch_conv_route(route, p, nullptr); });
    } catch (const std::exception&) {
        ms = -2.f;
    }
    return done(ms);
}

// developer entry: one dense convolution through launch_conv_route on operands prepared the way the engine prepares them, with every field
// of ConvParams the builder sets open to the caller.  x NHWC fp32 [N][H][W][xld >= Cin]; w folded [Cout][K], k = (kh * KW + kw) * Cin + ci;
// bias [Cout] or null; res [N][OH][OW][rld >= Cout] or null; y [N][OH][OW][yld >= Cout] with OH / OW from out_dim.  out_mode = OUT_DECONV2X2
// (1 x 1 geometry, no res): w is the checkpoint's [Cin][Cout][2][2], bias its [Cout] or null, dscale / dshift [Cout] (device, or null: 1 / 0)
// the channel affine of a folded BatchNorm - repacked here by pack_deconv2x2 as Builder::deconv2x2 does - and y is [N][2 H][2 W][yld].
// split = 1: the split-fp16 path, the (hi, lo) planes made here by split_weights_h3; 0: the fp32 MFMA path.  images (split only): bit 1 the
// one-accumulator GEMM image, bit 2 the 3x3 image, bit 3 the 9x9 image, each for the layers that get one in the engine (the bits of
// rd_debug_conv_route).  ln_g / ln_b [K] (the skinny route's fused LayerNorm) or null.  force: null = the natural route (conv_split_route /
// conv_f32_route), else the name of a staged tile of the precision ("256x128", "128x96", "256x64", "128x32", "128x64" split; "128x32" ..
// "128x128" fp32).  name[name_len] receives conv_route_name of the route launched, *range_out (optional) the range flag (0 on the fp32 path).
// Returns ms per launch (iters timed launches after one untimed); -1 with nothing launched: Cin % 4 or xld % 4 != 0, a view narrower than its
// channels, res or a geometry other than 1 x 1 with OUT_DECONV2X2, ln_g on a route that is not "skinny", a `force` that names no tile of the
// precision; -2: the launcher threw (a non-null ascale: no kernel applies it).
float rd_debug_conv_ex(int N, int H, int W, int Cin, int Cout, int KH, int KW, int SH, int SW, int PT, int PL, int PB, int PR, int act, int xld, int yld,
                       int rld, int out_mode, int split, int images, int allow_skinny, int iters, float* x, float* w, float* bias, float* res, float* y,
                       const float* dscale, const float* dshift, const float* ln_g, const float* ln_b, const float* ascale, const char* force,
                       char* name, int name_len, int* range_out) {
    rd::ConvRoute route = rd::CONV_F32_128x128;
    debug_copy_name("", name, name_len);
    const float ms = debug_conv_run(N, H, W, Cin, Cout, KH, KW, SH, SW, PT, PL, PB, PR, act, xld, yld, rld, out_mode, split, images, allow_skinny, iters,
                                    x, w, bias, res, y, dscale, dshift, ln_g, ln_b, ascale, force, nullptr, &route, range_out);
    if (ms != -1.f) debug_copy_name(rd::conv_route_name(route), name, name_len);
    return ms;
}

// developer entry: one 3x3 / stride 1 / pad 1 convolution of PPHGNet_small's widths on one of the three routes tools/mb_v4_server.py compares,
// operands prepared as the engine prepares them.  route 0: conv3x3_wide_h1 (kernels_conv3x3_wide.hip); 1: what conv_split_route gives the layer
// without the builder's opt-in (the generic split implicit GEMM); 2: conv3x3_h1 launched over pieces of <= 96 output channels (Cin <= 512).
// x NHWC [N][H][W][xld >= Cin], w folded [Cout][9 Cin], bias [Cout] or null, y [N][H][W][yld >= Cout]; name receives the route launched
// (of the last piece), *range_out (optional) the range flag.  Returns ms per launch (the pieces' sum), -1: the route does not take the layer
// (nothing launched), -2: a launcher threw.
float rd_debug_conv3x3_wide(int route, int N, int H, int W, int Cin, int Cout, int act, int xld, int yld, int iters, float* x, float* w, float* bias,
                            float* y, char* name, int name_len, int* range_out) {
    debug_copy_name("", name, name_len);
    if (route < 0 || route > 2 || !rd::conv3x3_wide_shape_ok(3, 3, Cin, Cout)) return -1.f;
    rd::ConvRoute r = rd::CONV_F32_128x128;
    float ms = 0.f;
    if (route == 2) {
        if (!rd::conv3x3_h1_shape_ok(3, 3, Cin, 96)) return -1.f;
        int any = 0;
        for (int n0 = 0; n0 < Cout; n0 += 96) {
            const int nn = std::min(96, Cout - n0);
            int flag = 0;
            const float t = debug_conv_run(N, H, W, Cin, nn, 3, 3, 1, 1, 1, 1, 1, 1, act, xld, yld, 0, rd::OUT_NHWC, 1, 4, 0, iters, x, w + (size_t)n0 * 9 * Cin,
                                           bias ? bias + n0 : nullptr, nullptr, y + n0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &r,
                                           range_out ? &flag : nullptr);
            if (t < 0.f || r != rd::CONV_C3H1) return t < 0.f ? t : -1.f;
            ms += t;
            any |= flag;
        }
        if (range_out) *range_out = any;
    } else {
        ms = debug_conv_run(N, H, W, Cin, Cout, 3, 3, 1, 1, 1, 1, 1, 1, act, xld, yld, 0, rd::OUT_NHWC, 1, route == 0 ? 16 : 0, 0, iters, x, w, bias, nullptr, y,
                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &r, range_out);
        if (ms >= 0.f && route == 0 && r != rd::CONV_C3WIDE) return -1.f;      // (refused by conv3x3_wide_applies: the generic route ran instead)
    }
    if (ms != -1.f) debug_copy_name(rd::conv_route_name(r), name, name_len);
    return ms;
}

// developer entry: rd_debug_conv_ex's convolution on dense maps (xld = Cin, yld = rld = Cout) with one stride S, NHWC output, no range flag,
// and the CALLER's split planes wh / wl (rows padded to Kp = ceil32(K)), or null for the fp32 MFMA kernels.  The one-accumulator 3x3 image is
// prepared when *used_direct is 0 or absent, the 9x9 image when it is 4.  *used_direct: in = 1 forces the direct k x k kernel when it
// supports the geometry, in = 2 the small-K streaming kernel, in = 4 the direct 9x9 kernel (kernels_conv9x9_h1.hip; in = 0 leaves a 9x9 layer
// on the generic k x k implicit GEMM it displaces); out = 1 / 2 / 4 when the direct / streaming / 9x9 kernel ran (3: the one-accumulator 3x3).
// Returns ms per launch (iters timed launches after one untimed).
float rd_debug_conv(int N, int H, int W, int Cin, int Cout, int KH, int KW, int S, int PT, int PL, int PB, int PR, int act, int iters,
                    float* x, float* w, void* wh, void* wl, float* bias, float* res, float* y, int* used_direct) {
    const DebugConvOld old{wh, wl, used_direct ? *used_direct : 0};
    const int images = old.code == 0 ? 4 : old.code == 4 ? 8 : 0;
    rd::ConvRoute route = rd::CONV_F32_128x128;
    const float ms = debug_conv_run(N, H, W, Cin, Cout, KH, KW, S, S, PT, PL, PB, PR, act, Cin, Cout, Cout, rd::OUT_NHWC, wh != nullptr, images, 0, iters, x,
                                    w, bias, res, y, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &old, &route, nullptr);
    if (used_direct && ms != -1.f) *used_direct = debug_conv_code(route);
    return ms;
}

// developer entry: the fused stem tail (kernels_stem34.hip).  x NHWC fp32 [N][H][W][xld >= Cin]; w3 [N1][9 Cin] with k = (kh * 3 + kw) * Cin + ci,
// w4 [N2][N1], biases [N1] / [N2] (device pointers); y NHWC [N][OH][OW][yld >= N2].  Images are prepared here the way the engine prepares them.
// Returns ms per launch, -1 when the shape is not covered.
float rd_debug_stem34(int N, int H, int W, int Cin, int xld, int N1, int N2, int yld, int act3, int act4, int iters, float* x, float* w3, float* b3,
                      float* w4, float* b4, float* y, unsigned* range_flag) {
    if (!rd::stem34_shape_ok(Cin, N1, N2)) return -1.f;
    std::vector<float> h3((size_t)N1 * 9 * Cin), h4((size_t)N2 * N1), hb3((size_t)((N1 + 31) / 32) * 32, 0.f);
    if (hipMemcpy(h3.data(), w3, h3.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1.f;
    if (hipMemcpy(h4.data(), w4, h4.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1.f;
    if (hipMemcpy(hb3.data(), b3, (size_t)N1 * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1.f;
    std::vector<uint16_t> i3, i4;
    float inv[2];
    rd::prepare_stem34_weights(h3.data(), h4.data(), Cin, N1, N2, i3, i4, inv);
    void *d3 = nullptr, *d4 = nullptr, *db3 = nullptr;
    if (hipMalloc(&d3, i3.size() * 2) != hipSuccess || hipMalloc(&d4, i4.size() * 2) != hipSuccess || hipMalloc(&db3, hb3.size() * 4) != hipSuccess) return -1.f;
    (void)hipMemcpy(d3, i3.data(), i3.size() * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(d4, i4.data(), i4.size() * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(db3, hb3.data(), hb3.size() * 4, hipMemcpyHostToDevice);
    rd::Stem34Params p{};
    p.x = x; p.xld = xld; p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.y = y; p.yld = yld;
    p.OH = (H - 1) / 2 + 1; p.OW = (W - 1) / 2 + 1; p.N1 = N1; p.N2 = N2;
    p.w3 = (const uint16_t*)d3; p.w3_inv = inv[0]; p.b3 = (const float*)db3;
    p.w4 = (const uint16_t*)d4; p.w4_inv = inv[1]; p.b4 = b4;
    p.act3 = act3; p.act4 = act4; p.range_flag = range_flag;
    const float ms = rd_debug_time(iters, [&] { rd::launch_stem34(p, nullptr); });
    (void)hipFree(d3); (void)hipFree(d4); (void)hipFree(db3);
    return ms;
}

// developer entry: the stem front alone.  route 1: the fused kernel (kernels_stem_fused.hip) - x NCHW fp32 [N][in_ch][H][W] (in_ch 1 or 3);
// w1 [27][C1] in the stem layout (row (kh * 3 + kw) * 3 + ci, co fastest), w2a folded [C1/2][4 C1] with k = tap * C1 + c, w2b folded
// [C1][4 (C1/2)], biases [C1] / [C1/2] / [C1] (device pointers, BN folded); y = cat NHWC [N][H2][W2][yld >= 2 C1] = [pool | stem2b];
// line_tab int32 [N][4] (rd_kernels.h LineTab) or null; range_flag or null.  The weight image and the bias vector are built here the way
// Builder::stem_front builds them (fits_fp16_range, prepare_stem_fused_weights, bias [C1 | C1/2 | C1]).  route 0: launch_stem_conv3x3s2
// alone (the fp32 kernel of the four-kernel plan): y = e NHWC [N][H2][W2][yld >= C1] with ReLU; w2a .. b2b, line_tab and range_flag are
// not read.  Returns ms per launch, -1 with nothing launched for an unsupported C1 / in_ch / yld or weights beyond the fp16 range.
float rd_debug_stem_front(int route, int N, int H, int W, int in_ch, int C1, int yld, int iters, float* x, float* w1, float* b1, float* w2a,
                          float* b2a, float* w2b, float* b2b, float* y, const int32_t* line_tab, unsigned* range_flag) {
    if ((route != 0 && route != 1) || N <= 0 || H <= 0 || W <= 0 || (in_ch != 1 && in_ch != 3) || !rd::stem_fused_supported(C1)) return -1.f;
    if (!x || !w1 || !b1 || !y || yld % 4 != 0 || yld < (route == 1 ? 2 * C1 : C1)) return -1.f;
    if (route == 0) {
        rd::StemParams p{};
        p.x = x; p.N = N; p.H = H; p.W = W; p.in_ch = in_ch; p.w = w1; p.bias = b1; p.y = y; p.yld = yld;
        p.OH = (H - 1) / 2 + 1; p.OW = (W - 1) / 2 + 1; p.Cout = C1; p.act = rd::ACT_RELU;
        return rd_debug_time(iters, [&] { rd::launch_stem_conv3x3s2(p, nullptr); });
    }
    if (!w2a || !b2a || !w2b || !b2b) return -1.f;
    const int na = C1 / 2;
    std::vector<float> h1((size_t)27 * C1), h2a((size_t)na * 4 * C1), h2b((size_t)C1 * 4 * na), bias((size_t)C1 + na + C1);
    if (hipMemcpy(h1.data(), w1, h1.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1.f;
    if (hipMemcpy(h2a.data(), w2a, h2a.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1.f;
    if (hipMemcpy(h2b.data(), w2b, h2b.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1.f;
    if (hipMemcpy(bias.data(), b1, (size_t)C1 * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1.f;
    if (hipMemcpy(bias.data() + C1, b2a, (size_t)na * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1.f;
    if (hipMemcpy(bias.data() + C1 + na, b2b, (size_t)C1 * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1.f;
    if (!rd::fits_fp16_range(h1) || !rd::fits_fp16_range(h2a) || !rd::fits_fp16_range(h2b)) return -1.f;
    std::vector<uint16_t> img;
    rd::prepare_stem_fused_weights(C1, h1.data(), h2a.data(), h2b.data(), img);
    void *dimg = nullptr, *dbias = nullptr;
    if (hipMalloc(&dimg, img.size() * 2) != hipSuccess) return -1.f;
    if (hipMalloc(&dbias, bias.size() * 4) != hipSuccess) { (void)hipFree(dimg); return -1.f; }
    (void)hipMemcpy(dimg, img.data(), img.size() * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(dbias, bias.data(), bias.size() * 4, hipMemcpyHostToDevice);
    const float ms = rd_debug_time(iters, [&] {
        rd::launch_stem_fused(C1, x, N, H, W, in_ch, (const uint16_t*)dimg, (const float*)dbias, y, yld, range_flag, nullptr, line_tab);
    });
    (void)hipFree(dimg); (void)hipFree(dbias);
    return ms;
}

// "lds1" .. "lds5" = dwconv_lds_variant, "kxk_lds5" / "7", "tiled4" / "8", "col", "pixel": what rd_debug_dw_route and rd_debug_dwconv_ex report
static std::string debug_dw_route_name(const rd::DwRoute& r) {
    static const char* const kernels[] = {"pixel", "lds", "kxk_lds", "col", "tiled"};
    return std::string(kernels[r.kernel]) + (r.kernel == rd::DW_PIXEL || r.kernel == rd::DW_COL ? "" : std::to_string(r.variant));
}

// developer entry: one depthwise convolution through launch_dwconv with every field of DwParams the engine sets open to the caller: x NHWC
// fp32 [N][H][W][xld >= C], w [KH*KW][C], bias [C] or null, res [N][OH][OW][rld >= C] or null, y [N][OH][OW][yld >= C] with OH / OW from
// out_dim as Builder::dwconv has them, line_w int32 [N] valid widths or null (stride-1 'same' widths only), tokinfo int32 [W] or null (ragged
// rows: N = H = KH = 1), gap = [N][chunks][C] partial sums of the output or null.  *gap_chunks as rd_debug_dwconv; name[name_len] receives the
// route's name (debug_dw_route_name) from the dw_route call the launch makes.  Returns ms per launch, -1 on a bad argument (nothing launched).
float rd_debug_dwconv_ex(int N, int H, int W, int C, int KH, int KW, int SH, int SW, int PT, int PL, int PB, int PR, int act, int xld, int yld, int rld,
                         int iters, float* x, float* w, float* bias, float* res, float* y, const int32_t* line_w, const int32_t* tokinfo, float* gap,
                         int* gap_chunks, char* name, int name_len) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 != 0 || KH <= 0 || KW <= 0 || SH <= 0 || SW <= 0 || PT < 0 || PL < 0 || PB < 0 || PR < 0) return -1.f;
    if (!x || !w || !y || xld < C || xld % 4 != 0 || yld < C || yld % 4 != 0 || (res && (rld < C || rld % 4 != 0))) return -1.f;
    if (H + PT + PB < KH || W + PL + PR < KW) return -1.f;
    rd::DwParams p = rd::dw_geometry(N, H, W, C, KH, KW, SH, SW, PT, PL, PB, PR);
    if (tokinfo && !(N == 1 && H == 1 && KH == 1 && SW == 1 && p.OW == W)) return -1.f;          // (Builder::dwconv's rules for the two tables)
    if (line_w && !(SW == 1 && p.OW == W)) return -1.f;
    p.x = x; p.xld = xld; p.w = w; p.bias = bias; p.y = y; p.yld = yld; p.act = act; p.res = res; p.rld = res ? rld : 0;
    p.tokinfo = tokinfo;
    if (line_w) { p.line_w = line_w; p.line_w_stride = 1; }
    p.gap_chunks = rd::dwconv_gap_chunks(p);
    p.gap_partial = p.gap_chunks > 0 ? gap : nullptr;
    const rd::DwRoute r = rd::dw_route(p, p.gap_partial != nullptr);
    // (tests: -1 = the one-channel-per-lane 5x5 / 7x7 kernel takes this call)
    if (gap_chunks) *gap_chunks = r.kernel == rd::DW_KXK_LDS ? -1 : p.gap_chunks;
    debug_copy_name(debug_dw_route_name(r).c_str(), name, name_len);
    return rd_debug_time(iters, [&] { rd::launch_dwconv(p, nullptr); });
}

// developer entry: rd_debug_dwconv_ex on dense maps (xld = yld = rld = C) with a square K x K kernel, stride (SH, 1), padding K / 2 and OW = W.
// *gap_chunks receives the chunk count the launcher uses for this geometry.  Returns ms per launch.
float rd_debug_dwconv(int N, int H, int W, int C, int K, int SH, int act, int iters, float* x, float* w, float* bias, float* res, float* y,
                      const int32_t* line_w, float* gap, int* gap_chunks) {
    return rd_debug_dwconv_ex(N, H, W, C, K, K, SH, 1, K / 2, K / 2, K / 2, K - 1 - K / 2, act, C, C, C, iters, x, w, bias, res, y, line_w, nullptr, gap,
                              gap_chunks, nullptr, 0);
}

// developer entry, host only (no HIP call): the route of a depthwise convolution.  Geometry as rd_debug_dwconv (K = 1 with ragged: the
// recogniser's 1 x 3 over one token row).  The kernel's name goes to name[name_len] ("lds1" .. "lds5" = dwconv_lds_variant, "kxk_lds5" / "7",
// "tiled4" / "8", "col", "pixel"), *gap_chunks (optional) receives the route's chunk count.  Returns the count the planner sizes the partial-sum
// buffer with (dwconv_gap_chunks on the unbound geometry), -1 on a bad argument.
int rd_debug_dw_route(int N, int H, int W, int C, int K, int SH, int ragged, int has_line_w, int wants_gap, char* name, int name_len, int* gap_chunks) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0 || SH <= 0) return -1;
    static const int32_t table[1] = {};        // something for the ragged / line-table pointers to point at
    rd::DwParams p{};
    p.xld = p.yld = p.rld = C; p.N = N; p.H = H; p.W = W; p.C = C;
    p.KH = ragged ? 1 : K; p.KW = ragged ? 3 : K; p.SH = SH; p.SW = 1; p.PT = p.KH / 2; p.PL = p.KW / 2;
    p.OH = (H + 2 * p.PT - p.KH) / SH + 1; p.OW = W;
    const int planned = rd::dwconv_gap_chunks(p);
    if (ragged) p.tokinfo = table;
    if (has_line_w) { p.line_w = table; p.line_w_stride = 1; }
    const rd::DwRoute r = rd::dw_route(p, wants_gap != 0);
    debug_copy_name(debug_dw_route_name(r).c_str(), name, name_len);
    if (gap_chunks) *gap_chunks = r.gap_chunks;
    return planned;
}

// developer entry, host only (no HIP call): the weight rules of rd_host.h on w[n].  Returns rd_pow2_exp(w, n, clamp) (clamp <= 0: not
// clamped) and writes, per element i, the fp16 bits (hi, lo) of rd_split_scaled at that exponent to scaled[2 i], scaled[2 i + 1] and of
// rd_split_2048 to h3[2 i], h3[2 i + 1].  Returns -1000 (no exponent) on a bad argument.
int rd_debug_weight_split(const float* w, int n, int clamp, uint16_t* scaled, uint16_t* h3) {
    if (!w || n <= 0 || !scaled || !h3) return -1000;
    const int ex = rd::rd_pow2_exp(w, (size_t)n, clamp);
    for (int i = 0; i < n; ++i) {
        rd::rd_split_scaled(w[i], ex, scaled[2 * i], scaled[2 * i + 1]);
        rd::rd_split_2048(w[i], h3[2 * i], h3[2 * i + 1]);
    }
    return ex;
}

// developer entry: one PPLCNetV3 depthwise layer through launch_lcv3_dw (kernels_lcv3.hip; x NHWC fp32 [N][H][W][C], w [K*K][C], bias [C],
// y [N][OH][OW][C]; aff = {pre_s, pre_b, post_s, post_b}, pre_act: hardswish + (pre_s, pre_b) on load; line_in / line_out int32 [N] valid
// widths or null; gap: [N][OH][C] row sums of y over the output width, or null).  Returns ms per launch, < 0: geometry not served.
float rd_debug_lcv3_dw(int N, int H, int W, int C, int K, int SH, int SW, int pre_act, int iters, const float* aff, float* x, float* w, float* bias,
                       float* y, const int32_t* line_in, const int32_t* line_out, float* gap) {
    if (!rd::lcv3_dw_shape_ok(K, SH, SW, C) || !aff || (gap && !rd::lcv3_gap_shape_ok(C))) return -1.f;
    rd::Lcv3DwParams p{};
    p.x = x; p.xld = C; p.N = N; p.H = H; p.W = W; p.C = C; p.w = w; p.bias = bias; p.y = y; p.yld = C;
    p.K = K; p.SH = SH; p.SW = SW;
    p.OH = (H + 2 * (K / 2) - K) / SH + 1; p.OW = (W + 2 * (K / 2) - K) / SW + 1;
    p.pre_act = pre_act; p.pre_s = aff[0]; p.pre_b = aff[1]; p.post_s = aff[2]; p.post_b = aff[3]; p.post_act = 1;
    p.line_in = line_in; p.line_out = line_out; p.line_stride = 1;
    return rd_debug_time(iters, [&] { rd::launch_lcv3_dw(p, nullptr); },
                         [&] { if (gap) rd::launch_lcv3_gap_rows(y, C, N, p.OH, p.OW, C, gap, line_out, 1, nullptr); });
}

// developer entry: one 5x5 depthwise layer of the recogniser geometry through launch_dw5_strip (kernels_mv1e.hip; x NHWC fp32 [N][H][W][xld],
// w [25][C], bias [C], y [N][OH][OW][yld], OH = (H - 1) / SH + 1, OW = (W - 1) / SW + 1; aff = {pre_s, pre_b, post_s, post_b}; pre_act:
// hardswish + (pre_s, pre_b) on load; post_act 0: convolution + bias only; line_in / line_out int32 [N] valid widths or null).  Returns ms
// per launch, < 0: geometry not served (dw5_strip_launch_ok).
float rd_debug_dw5_strip(int N, int H, int W, int C, int SH, int SW, int pre_act, int post_act, int xld, int yld, int iters, const float* aff, float* x,
                         float* w, float* bias, float* y, const int32_t* line_in, const int32_t* line_out) {
    if (!aff || SH < 1 || SW < 1) return -1.f;
    rd::Lcv3DwParams p{};
    p.x = x; p.xld = xld; p.N = N; p.H = H; p.W = W; p.C = C; p.w = w; p.bias = bias; p.y = y; p.yld = yld;
    p.K = 5; p.SH = SH; p.SW = SW;
    p.OH = (H - 1) / SH + 1; p.OW = (W - 1) / SW + 1;
    p.pre_act = pre_act; p.pre_s = aff[0]; p.pre_b = aff[1]; p.post_s = aff[2]; p.post_b = aff[3]; p.post_act = post_act;
    p.line_in = line_in; p.line_out = line_out; p.line_stride = 1;
    if (!rd::dw5_strip_launch_ok(p)) return -1.f;
    return rd_debug_time(iters, [&] { (void)rd::launch_dw5_strip(p, nullptr); });
}

// developer entry: MobileNetV1Enhance's final pooling through launch_mv1e_pool (x NHWC [N][H][W][C], H >= 2; y [N][W / 2][C], or with
// line_tab int32 [N][4] the compact token rows it names).  Returns 0, < 0: geometry not served.
int rd_debug_mv1e_pool(int N, int H, int W, int C, float* x, float* y, const int32_t* line_tab) {
    if (N < 1 || H < 2 || W < 2 || C < 4 || C % 4 != 0) return -1;
    rd::launch_mv1e_pool(x, C, y, C, N, H, W, C, nullptr, line_tab);
    return hipStreamSynchronize(nullptr) == hipSuccess ? 0 : -2;
}

// developer entry, host only (no device is touched): the load-time derived tensor `name` of "ppocrv5_det_mobile" - a folded
// LearnableRepLayer (`<layer>.fold.weight / .bias`) or `neck.ins_conv.<i>.fold.*` - or of "ppocrv3_det_mobile" - a folded Conv + BatchNorm
// (`backbone.stages.<s>.<i>.{expand,bottleneck,linear}_conv.fold.*`, `backbone.stages.3.3.fold.*`) - from a safetensors image.  Copies at most
// `capacity` floats to `out` and returns the tensor's element count; -1: unknown kind, name or a malformed image.
long rd_debug_derived_tensor(const char* kind, const void* img, size_t nbytes, const char* name, float* out, long capacity) {
    try {
        if (!kind || !img || !name) return -1;
        const std::string k(kind);
        rd::WeightStore ws;
        ws.load_safetensors(img, nbytes);
        const rd::ModelDesc* m = rd::find_model(k);
        if (!m || !m->derived_tensors) return -1;
        m->derive(ws);
        if (!ws.has(name)) return -1;
        const rd::HostTensor& t = ws.get(name);
        const long n = (long)t.numel();
        if (out) std::copy(t.f32(), t.f32() + std::min(n, capacity), out);
        return n;
    } catch (const std::exception&) {
        return -1;
    }
}

// developer entry: one MobileNetV3 depthwise layer through launch_mbv3_dw (kernels_mbv3.hip; x NHWC fp32 [N][H][W][xld >= C], w [K*K][C], bias
// [C], y [N][OH][OW][yld >= C], OH = (H - 1) / S + 1; pre_act / post_act: 0 none, 1 ReLU, 2 hardswish - the producer's on load inside the map,
// the layer's own in the epilogue; max_blocks > 0 caps the grid, so that a small map meets the grid-stride loop).  Returns ms per launch, < 0: not served (mbv3_dw_launch_ok).
float rd_debug_mbv3_dw(int N, int H, int W, int C, int K, int S, int pre_act, int post_act, int xld, int yld, int iters, int max_blocks, float* x, float* w,
                       float* bias, float* y) {
    if (S < 1) return -1.f;
    rd::Mbv3DwParams p{};
    p.x = x; p.xld = xld; p.N = N; p.H = H; p.W = W; p.C = C; p.w = w; p.bias = bias; p.y = y; p.yld = yld;
    p.K = K; p.S = S; p.OH = (H - 1) / S + 1; p.OW = (W - 1) / S + 1;
    p.pre_act = pre_act; p.post_act = post_act; p.max_blocks = max_blocks;
    if (!x || !w || !bias || !y || !rd::mbv3_dw_launch_ok(p)) return -1.f;
    return rd_debug_time(iters, [&] { (void)rd::launch_mbv3_dw(p, nullptr); });
}

// developer entry: one MobileNetV3 inverted-residual block through launch_mbv3_block (kernels_mbv3.hip; x NHWC fp32 [N][H][W][xld >= cin],
// we [mid][cin], be [mid], wd [K*K][mid], bd [mid], wl [cout][mid], bl [cout], y [N][OH][OW][yld >= cout]; act 1 ReLU / 2 hardswish;
// in_hswish: hardswish on load; shortcut: y += x').  Returns ms per launch, < 0: not served (mbv3_block_launch_ok).
float rd_debug_mbv3_block(int N, int H, int W, int cin, int mid, int cout, int K, int S, int act, int in_hswish, int shortcut, int xld, int yld, int iters,
                          float* x, float* we, float* be, float* wd, float* bd, float* wl, float* bl, float* y) {
    if (S < 1) return -1.f;
    rd::Mbv3BlockParams p{};
    p.x = x; p.xld = xld; p.N = N; p.H = H; p.W = W; p.cin = cin; p.mid = mid; p.cout = cout;
    p.we = we; p.be = be; p.wd = wd; p.bd = bd; p.wl = wl; p.bl = bl; p.y = y; p.yld = yld;
    p.K = K; p.S = S; p.OH = (H - 1) / S + 1; p.OW = (W - 1) / S + 1;
    p.act = act; p.in_hswish = in_hswish; p.shortcut = shortcut;
    if (!x || !we || !be || !wd || !bd || !wl || !bl || !y || !rd::mbv3_block_launch_ok(p)) return -1.f;
    return rd_debug_time(iters, [&] { (void)rd::launch_mbv3_block(p, nullptr); });
}
// host only: would mbv3_block_kernel serve this geometry (contiguous, aligned views assumed)?  1 yes, 0 no
int rd_debug_mbv3_block_ok(int N, int H, int W, int cin, int mid, int cout, int K, int S, int act, int shortcut, int xld, int yld) {
    if (S < 1) return 0;
    rd::Mbv3BlockParams p{};
    p.xld = xld; p.N = N; p.H = H; p.W = W; p.cin = cin; p.mid = mid; p.cout = cout; p.yld = yld;
    p.K = K; p.S = S; p.OH = (H - 1) / S + 1; p.OW = (W - 1) / S + 1;
    p.act = act; p.shortcut = shortcut;
    return rd::mbv3_block_launch_ok(p) ? 1 : 0;
}

// developer entry: one MobileNetV3-small depthwise layer through launch_mbv3s_dw (kernels_mbv3s.hip; x NHWC fp32 [N][H][W][xld >= C], w [K*K][C],
// bias [C], y [N][OH][OW][yld >= C], OH = (H - 1) / SH + 1, OW = (W - 1) / SW + 1; pre_act / post_act / max_blocks as rd_debug_mbv3_dw).
// Returns ms per launch, < 0: not served (mbv3s_dw_launch_ok).
float rd_debug_mbv3s_dw(int N, int H, int W, int C, int K, int SH, int SW, int pre_act, int post_act, int xld, int yld, int iters, int max_blocks, float* x,
                        float* w, float* bias, float* y) {
    if (SH < 1 || SW < 1) return -1.f;
    rd::Mbv3sDwParams p{};
    p.x = x; p.xld = xld; p.N = N; p.H = H; p.W = W; p.C = C; p.w = w; p.bias = bias; p.y = y; p.yld = yld;
    p.K = K; p.SH = SH; p.SW = SW; p.OH = (H - 1) / SH + 1; p.OW = (W - 1) / SW + 1;
    p.pre_act = pre_act; p.post_act = post_act; p.max_blocks = max_blocks;
    if (!x || !w || !bias || !y || !rd::mbv3s_dw_launch_ok(p)) return -1.f;
    return rd_debug_time(iters, [&] { (void)rd::launch_mbv3s_dw(p, nullptr); });
}

// developer entry: one MobileNetV3-small inverted-residual block with optional squeeze-excite on caller-supplied FOLDED weights, through the
// operators the engine's plan chains for it (route 0) or through cls_block_kernel, the block as the one-launch classifier runs it (route 1).
// Route 0: fp32 1x1 (launch_conv_igemm; a ReLU block activates in its
// epilogue, a hardswish block in the depthwise kernel's load) -> launch_mbv3s_dw -> [launch_gap_partial -> launch_se_fc with the paddle
// hard-sigmoid -> launch_scale_channels] -> fp32 1x1 (+ x).  x NHWC [N][H][W][xld >= cin], we [mid][cin], be [mid], wd [K*K][mid], bd [mid],
// w1 [mid/4][mid], b1 [mid/4], w2 [mid][mid/4], b2 [mid] (se != 0), wl [cout][mid], bl [cout], y [N][OH][W][yld >= cout]; act 1 ReLU / 2
// hardswish.  Temporaries are allocated per call.  Returns ms per block, < 0: not served (another route, a geometry a kernel declines,
// or no memory).
float rd_debug_mbv3s_block(int route, int N, int H, int W, int cin, int mid, int cout, int K, int SH, int act, int se, int shortcut, int xld, int yld,
                           int iters, float* x, float* we, float* be, float* wd, float* bd, float* w1, float* b1, float* w2, float* b2, float* wl,
                           float* bl, float* y) {
    if ((route != 0 && route != 1) || SH < 1 || N < 1 || H < 1 || W < 1 || cin % 4 != 0 || mid % 8 != 0 || cout % 4 != 0 || mid > 512) return -1.f;
    if (act != rd::MBV3_RELU && act != rd::MBV3_HSWISH) return -1.f;
    if (shortcut && (SH != 1 || cin != cout)) return -1.f;
    if (!x || !we || !be || !wd || !bd || !wl || !bl || !y || (se && (!w1 || !b1 || !w2 || !b2))) return -1.f;
    if (route == 1) {       // the block as cls_line_kernel runs it, one workgroup per image
        rd::ClsBlockParams L{};
        L.we = we; L.be = be; L.wd = wd; L.bd = bd; L.w1 = w1; L.b1 = b1; L.w2 = w2; L.b2 = b2; L.wl = wl; L.bl = bl;
        L.k = K; L.cin = cin; L.mid = mid; L.cout = cout; L.sh = SH; L.se = se ? 1 : 0; L.act = act; L.shortcut = shortcut ? 1 : 0;
        if (!rd::cls_block_plan(L, H, W) || !rd::cls_block_launch_ok(L, N, H, W, xld, yld)) return -1.f;
        float* scratch = nullptr;
        if (hipMalloc((void**)&scratch, (size_t)std::min(N, 512) * rd::cls_block_scratch_floats(L, H, W) * sizeof(float)) != hipSuccess) return -1.f;
        const float t = rd_debug_time(iters, [&] { (void)rd::launch_cls_block(L, x, xld, y, yld, N, H, W, scratch, nullptr); });
        (void)hipFree(scratch);
        return t;
    }
    const int OH = (H - 1) / SH + 1, hw = OH * W;
    const int chunks = std::max(1, std::min(64, hw / 256));
    const size_t ne = (size_t)N * H * W * mid, nd = (size_t)N * OH * W * mid, np = (size_t)N * chunks * mid, ng = (size_t)N * mid;
    float* tmp = nullptr;
    if (hipMalloc((void**)&tmp, (ne + nd + np + ng) * sizeof(float)) != hipSuccess) return -1.f;
    float *e = tmp, *d = e + ne, *partial = d + nd, *gate = partial + np;
    rd::Mbv3sDwParams q{};
    q.x = e; q.xld = mid; q.N = N; q.H = H; q.W = W; q.C = mid; q.w = wd; q.bias = bd; q.y = d; q.yld = mid;
    q.K = K; q.SH = SH; q.SW = 1; q.OH = OH; q.OW = W;
    q.pre_act = act == rd::MBV3_RELU ? rd::MBV3_NONE : rd::MBV3_HSWISH; q.post_act = act;
    if (!rd::mbv3s_dw_launch_ok(q)) {
        (void)hipFree(tmp);
        return -1.f;
    }
    auto pointwise = [&](const float* in, int ild, int pixels_h, int ci, const float* w, const float* b, float* out, int old, int co, int a, const float* res) {
        rd::ConvParams c{};
        c.x = in; c.xld = ild; c.N = N; c.H = pixels_h; c.W = W; c.Cin = ci; c.w = w; c.bias = b; c.y = out; c.yld = old;
        c.OH = pixels_h; c.OW = W; c.Cout = co; c.KH = c.KW = c.SH = c.SW = 1;
        c.res = res; c.rld = res ? xld : 0; c.act = a; c.out_mode = rd::OUT_NHWC;
        c.M = N * pixels_h * W; c.K = ci; c.Ng = co;
        rd::launch_conv_igemm(c, nullptr);
    };
    const float ms = rd_debug_time(iters, [&] {
        pointwise(x, xld, H, cin, we, be, e, mid, mid, act == rd::MBV3_RELU ? rd::ACT_RELU : rd::ACT_NONE, nullptr);
        (void)rd::launch_mbv3s_dw(q, nullptr);
        if (se) {
            rd::launch_gap_partial(d, mid, N, hw, mid, partial, chunks, nullptr);
            rd::SeFcParams f{};
            f.partial = partial; f.chunks = chunks; f.N = N; f.C = mid; f.Cr = mid / 4; f.inv_hw = 1.f / (float)hw;
            f.w1 = w1; f.b1 = b1; f.w2 = w2; f.b2 = b2; f.gate = rd::ACT_HSIG_PADDLE; f.scale = gate; f.H = OH;
            rd::launch_se_fc(f, nullptr);
            rd::launch_scale_channels(d, mid, d, mid, gate, 0.f, N, hw, mid, nullptr);
        }
        pointwise(d, mid, OH, mid, wl, bl, y, yld, cout, rd::ACT_NONE, shortcut ? x : nullptr);
    });
    (void)hipFree(tmp);
    return ms;
}

// developer entry: one PPLCNetV3 depthwise layer in the detector geometry (x NHWC fp32 [N][H][W][C], w [K*K][C], bias [C], y [N][OH][OW][C] with
// OH = (H + 2 (K / 2) - K) / S + 1; aff as above; post_act 0: convolution + bias only).  route 0: launch_lcv3_dw (kernels_lcv3.hip), 1: the
// LDS-staged launch_lcv3_dw2d (kernels_lcv3_det.hip).  Returns ms per launch, < 0: geometry not served by that route.
float rd_debug_lcv3_dw_det(int N, int H, int W, int C, int K, int S, int pre_act, int post_act, int route, int iters, const float* aff, float* x,
                           float* w, float* bias, float* y) {
    if (!aff || N < 1 || H < 1 || W < 1 || (S != 1 && S != 2) || (route != 0 && route != 1)) return -1.f;
    if (route == 0 && !rd::lcv3_dw_shape_ok(K, S, S, C)) return -1.f;
    rd::Lcv3DwParams p{};
    p.x = x; p.xld = C; p.N = N; p.H = H; p.W = W; p.C = C; p.w = w; p.bias = bias; p.y = y; p.yld = C;
    p.K = K; p.SH = p.SW = S;
    p.OH = (H + 2 * (K / 2) - K) / S + 1; p.OW = (W + 2 * (K / 2) - K) / S + 1;
    p.pre_act = pre_act; p.pre_s = aff[0]; p.pre_b = aff[1]; p.post_s = aff[2]; p.post_b = aff[3]; p.post_act = post_act;
    if (route == 1 && !rd::lcv3_dw2d_launch_ok(p)) return -1.f;         // shape, or a grid beyond 2^31 workgroups
    return rd_debug_time(iters, [&] { if (route) (void)rd::launch_lcv3_dw2d(p, nullptr); else rd::launch_lcv3_dw(p, nullptr); });
}

// developer entry: one PPLCNetV3 block (depthwise 3x3 stride 1 -> pointwise) through launch_lcv3_block (kernels_lcv3_block.hip; x NHWC fp32
// [N][H][W][cin], dw_w [9][cin], dw_b [cin], pw_w [cout][cin], pw_b [cout], y [N][H][W][cout]; aff = {pre_s, pre_b, mid_s, mid_b, out_s,
// out_b}; pre_act / out_act: hardswish + affine on load / in the epilogue; split: 1 = split-fp16 product raising *range_flag (a device-
// visible word) on an operand beyond the fp16 range, 0 = fp32 product; line_w int32 [N] valid widths or null).  Returns ms per launch,
// < 0: geometry not served.
float rd_debug_lcv3_block(int N, int H, int W, int cin, int cout, int pre_act, int out_act, int split, int iters, const float* aff, float* x,
                          float* dw_w, float* dw_b, float* pw_w, float* pw_b, float* y, const int32_t* line_w, unsigned* range_flag) {
    if (!rd::lcv3_block_shape_ok(cin, cout) || !aff || N < 1 || H < 1 || W < 1) return -1.f;
    rd::Lcv3BlockParams p{};
    p.x = x; p.xld = cin; p.N = N; p.H = H; p.W = W; p.cin = cin; p.cout = cout;
    p.dw_w = dw_w; p.dw_b = dw_b; p.pw_w = pw_w; p.pw_b = pw_b; p.y = y; p.yld = cout;
    p.pre_act = pre_act; p.pre_s = aff[0]; p.pre_b = aff[1]; p.mid_s = aff[2]; p.mid_b = aff[3];
    p.out_act = out_act; p.out_s = aff[4]; p.out_b = aff[5];
    p.line_w = line_w; p.line_stride = 1; p.split = split; p.range_flag = range_flag;
    return rd_debug_time(iters, [&] { rd::launch_lcv3_block(p, nullptr); });
}

// developer timing of the fused CTC head on prepared weights: wp = W' [C][128] fp32 (bias in column K), wh / wl its fp16 split
// (null: fp32 MFMA kernel); part = workspace of M * 64 * 4 floats.  Returns ms per launch; *nsplit_out = the split count used.
float rd_debug_time_ctc(int M, int K, int Ccls, int iters, float* x, float* wp, void* wh, void* wl, float* part, int32_t* idx, float* prob,
                        int nsplit_override, int* nsplit_out) {
    rd::CtcParams p{};
    p.x = x; p.xld = K; p.w = wp; p.M = M; p.K = K; p.C = Ccls; p.part = part;
    p.nsplit = nsplit_override > 0 ? nsplit_override : rd::ctc_head_nsplit(M, Ccls, wh != nullptr);
    p.idx = idx; p.prob = prob;
    p.wh = (const uint16_t*)wh; p.wl = (const uint16_t*)wl;
    if (nsplit_out) *nsplit_out = p.nsplit;
    return rd_debug_time(iters, [&] { rd::launch_ctc_head(p, nullptr); });
}

// developer timing of the checkbox stage's threshold kernel alone (cb_bin_kernel, the one pass over the 3 B / pixel pages): pages
// [P][H][W][3] u8, bin = room for P * H * ceil(W / 64) 64-bit words.  Returns ms per launch, -1 outside the stage's bounds.
float rd_debug_time_checkbox_mask(int P, int H, int W, int iters, void* pages, void* bin) {
    if (!pages || !bin || P < 1 || P > RD_CHECKBOX_MAX_PAGES || H < 1 || W < 1 || H > RD_CHECKBOX_MAX_SIDE || W > RD_CHECKBOX_MAX_SIDE) return -1.f;
    return rd_debug_time(iters, [&] { rd::launch_checkbox_bin((const uint8_t*)pages, P, H, W, 0, (uint64_t*)bin, nullptr); });
}

// A range-flag word for the developer entries below: pinned, device-mapped host memory, as the engine's own (engine.cpp load_weights).
static unsigned* debug_flag_new() {
    unsigned* flag = nullptr;
    if (hipHostMalloc((void**)&flag, sizeof(unsigned), hipHostMallocMapped) != hipSuccess || !flag) return nullptr;
    *flag = 0;
    return flag;
}
static int debug_finish(unsigned* flag, int* range_out) {
    const bool ok = hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
    if (range_out) *range_out = flag ? (int)*flag : 0;
    if (flag) (void)hipHostFree(flag);
    return ok ? 0 : -1;
}

// developer entry: the self-attention alone on packed qkv [tokens][3 heads hd] fp32 -> o [tokens][heads hd].  seg = int32 [B][2] (first token,
// tokens) on the device, or null: B dense lines of T tokens.  route 0 = launch_attention exactly as the engine calls it (kernel per line),
// 1 = the VALU kernel for every line, 2 = the matrix-core kernel only (lines beyond its limit are left untouched).  One launch, synchronised.
// *range_out (optional) receives 1 when the matrix-core kernel raised its range flag.  Returns 0, or -1 for a head size or route the
// library does not have.
int rd_debug_attention(int B, int T, int heads, int hd, float scale, float* qkv, float* o, const int32_t* seg, int route, int* range_out) {
    if (range_out) *range_out = 0;
    if (B <= 0 || T <= 0 || heads <= 0 || !(hd == 15 || hd == 16 || hd == 32) || route < 0 || route > 2) return -1;
    if (route == 2 && !rd::attention_h3_applies(1, hd)) return -1;
    unsigned* flag = debug_flag_new();
    if (!flag) return -1;
    if (route == 0) rd::launch_attention(qkv, o, B, T, heads, hd, scale, nullptr, seg, flag);
    else if (route == 1) rd::launch_attention_valu(qkv, o, B, T, heads, hd, scale, nullptr, seg);
    else rd::launch_attention_h3(qkv, o, B, T, heads, hd, scale, nullptr, seg, flag);
    return debug_finish(flag, range_out);
}
// developer entry: vit_attention_kernel alone (kernels_vit_attn.hip) on packed qkv [B][T][3 heads 64] fp32 -> o [B][T][heads 64]; one launch,
// synchronised.  Returns 0, or -1 for a head size or length the kernel does not serve (hd = 64, 1 <= T <= 1024).
int rd_debug_vit_attention(int B, int T, int heads, int hd, float scale, float* qkv, float* o) {
    if (B <= 0 || B > 65535 || heads <= 0 || heads > 65535 || !qkv || !o || !rd::vit_attention_applies(T, hd)) return -1;
    rd::launch_vit_attention(qkv, o, B, T, heads, scale, nullptr);
    return debug_finish(nullptr, nullptr);
}
// *h3_max_t = the longest line the matrix-core kernel serves at this head size (0: it has none), *valu_lds_keys = the keys the VALU kernel
// holds in LDS at once (longer lines run over key tiles).  Returns -1 for a head size the library does not have.
int rd_debug_attention_limits(int hd, int* h3_max_t, int* valu_lds_keys) {
    if (!(hd == 15 || hd == 16 || hd == 32)) return -1;
    if (h3_max_t) *h3_max_t = rd::attention_h3_applies(1, hd) ? rd::attention_h3_max_t() : 0;
    if (valu_lds_keys) *valu_lds_keys = rd::attention_lds_keys(hd);
    return 0;
}

// developer entry: LayerNorm over the last dimension, y[M][yld] = (x[M][xld] - mean) * rstd * g + b on the first C columns.  -1 for C > 512,
// except C = 768 (layernorm768_kernel; xld and yld multiples of 4).
int rd_debug_layernorm(int M, int C, float* x, int xld, float* y, int yld, float* g, float* b, float eps) {
    if (M <= 0 || C <= 0 || xld < C || yld < C) return -1;
    if (C == 768) {
        if (xld % 4 || yld % 4) return -1;
        rd::launch_layernorm768(x, xld, y, yld, g, b, M, eps, nullptr);
        return debug_finish(nullptr, nullptr);
    }
    if (C > 512) return -1;
    rd::launch_layernorm(x, xld, y, yld, g, b, M, C, eps, nullptr);
    return debug_finish(nullptr, nullptr);
}

// developer entry: the squeeze-excite chain launch_gap_partial -> launch_se_fc -> launch_scale_channels on caller-owned buffers, synchronised.
// x NHWC fp32 [N][H][W][xld >= C], w1 [Cr][C], b1 [Cr], w2 [C][Cr], b2 [C], partial [N][chunks][C], gate_out [N][C], y [N][H][W][yld >= C] or
// null (no scaling pass: y = x (gate + alpha) otherwise).  fill_partial != 0: the entry fills `partial` from x; 0: the caller has (a
// depthwise launch's SE sums).  line_w int32 [N] or null: image n pools over H x line_w[n] - only with caller-filled sums, as in the engine
// (launch_gap_partial knows no line ends).  Returns 0, -1 on a bad argument or a width se_fc_shape_ok declines (nothing launched).
int rd_debug_se_chain(int N, int H, int W, int C, int Cr, int chunks, int gate_act, float alpha, int xld, int yld, int fill_partial, float* x,
                      float* w1, float* b1, float* w2, float* b2, const int32_t* line_w, float* partial, float* gate_out, float* y) {
    if (N <= 0 || H <= 0 || W <= 0 || !rd::se_fc_shape_ok(C) || Cr <= 0 || Cr > 4096 || chunks <= 0) return -1;
    if (!w1 || !b1 || !w2 || !b2 || !partial || !gate_out || (fill_partial && line_w)) return -1;
    if ((fill_partial || y) && (!x || xld < C || xld % 4 != 0)) return -1;
    if (y && (yld < C || yld % 4 != 0)) return -1;
    const int hw = H * W;
    if (fill_partial) rd::launch_gap_partial(x, xld, N, hw, C, partial, chunks, nullptr);
    rd::SeFcParams f{};
    f.partial = partial; f.chunks = chunks; f.N = N; f.C = C; f.Cr = Cr; f.inv_hw = 1.f / (float)hw;
    f.w1 = w1; f.b1 = b1; f.w2 = w2; f.b2 = b2; f.gate = gate_act; f.scale = gate_out; f.H = H;
    if (line_w) { f.line_w = line_w; f.line_w_stride = 1; }
    rd::launch_se_fc(f, nullptr);
    if (y) rd::launch_scale_channels(x, xld, y, yld, gate_out, alpha, N, hw, C, nullptr);
    return debug_finish(nullptr, nullptr);
}

// developer entry: the ESE gate of PPHGNet_small (kernels_ese.hip) as the engine chains it: launch_gap_partial (ese_gap_chunks(H W) chunks) ->
// launch_ese_gate -> launch_ese_apply, synchronised.  x NHWC [N][H][W][xld >= C], w [C][C], b [C], partial [N][chunks][C] scratch, gate_out
// [N][C], idn [N][H][W][ild >= C] or null, y [N][H][W][yld >= C] (may be x).  *chunks_out (optional) receives the chunk count.  Returns 0,
// -1 on a bad argument or a width ese_shape_ok declines (nothing launched).
int rd_debug_ese(int N, int H, int W, int C, int xld, int ild, int yld, float* x, float* w, float* b, float* idn, float* partial, float* gate_out,
                 float* y, int* chunks_out) {
    if (N <= 0 || H <= 0 || W <= 0 || !rd::ese_shape_ok(C) || !x || !w || !b || !gate_out || !y) return -1;
    if (xld < C || xld % 4 || yld < C || yld % 4 || (idn && (ild < C || ild % 4))) return -1;
    const int hw = H * W, chunks = rd::ese_gap_chunks(hw);
    if (chunks_out) *chunks_out = chunks;
    if (!partial) return chunks_out ? 0 : -1;          // (a size query)
    rd::launch_gap_partial(x, xld, N, hw, C, partial, chunks, nullptr);
    rd::launch_ese_gate(partial, chunks, N, C, 1.f / (float)hw, w, b, gate_out, nullptr);
    rd::launch_ese_apply(x, xld, gate_out, idn, ild, y, yld, N, hw, C, nullptr);
    return debug_finish(nullptr, nullptr);
}

// developer entry: MaxPool2d(3, stride 2, padding 1) (kernels_ese.hip): y [N][(H - 1) / 2 + 1][(W - 1) / 2 + 1][yld >= C] of x [N][H][W][xld >= C]
int rd_debug_maxpool3x3s2(int N, int H, int W, int C, int xld, int yld, float* x, float* y) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 || !x || !y || xld < C || xld % 4 || yld < C || yld % 4) return -1;
    rd::launch_maxpool3x3s2(x, xld, y, yld, N, H, W, C, nullptr);
    return debug_finish(nullptr, nullptr);
}

// developer entries: the small NHWC operators of kernels_misc.hip, one synchronised launch each on caller-owned buffers with explicit leading
// dimensions (multiples of 4, >= C).  Each returns 0, -1 on a bad argument (nothing launched).
// y [N][H][W] = max over the 2 x 2 window at (h, w) of x zero-padded by one row / column
int rd_debug_maxpool2x2s1(int N, int H, int W, int C, int xld, int yld, float* x, float* y) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 || !x || !y || xld < C || xld % 4 || yld < C || yld % 4) return -1;
    rd::launch_maxpool2x2s1(x, xld, y, yld, N, H, W, C, nullptr);
    return debug_finish(nullptr, nullptr);
}
// y [N][H / 3][W / 2] = avg_pool2d((3, 2)) of x [N][H][W]; with line_tab (int32 [N][kLineTabStride], H / 3 == 1) image n writes its
// line_tab[n][2] / 2 tokens at row line_tab[n][3] of y instead
int rd_debug_avgpool3x2(int N, int H, int W, int C, int xld, int yld, float* x, float* y, const int32_t* line_tab) {
    if (N <= 0 || H < 3 || W < 2 || C <= 0 || C % 4 || !x || !y || xld < C || xld % 4 || yld < C || yld % 4 || (line_tab && H / 3 != 1)) return -1;
    rd::launch_avgpool3x2(x, xld, y, yld, N, H, W, C, nullptr, line_tab);
    return debug_finish(nullptr, nullptr);
}
// y [n][:][w >= line_w[n * stride]] = 0
int rd_debug_mask_cols(int N, int H, int W, int C, int yld, float* y, const int32_t* line_w, int stride) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 || !y || yld < C || yld % 4 || !line_w || stride < 1) return -1;
    rd::launch_mask_cols(y, yld, N, H, W, C, line_w, stride, nullptr);
    return debug_finish(nullptr, nullptr);
}
// y [N][H][W] (+)= x [N][H / f][W / f] nearest; H and W are the output's and multiples of f
int rd_debug_upsample(int N, int H, int W, int C, int f, int accumulate, int xld, int yld, float* x, float* y) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 || f < 1 || H % f || W % f || !x || !y || xld < C || xld % 4 || yld < C || yld % 4) return -1;
    rd::launch_upsample(x, xld, y, yld, N, H, W, C, f, accumulate, nullptr);
    return debug_finish(nullptr, nullptr);
}
// y [M][yld] = a [M][ald] + b [M][bld] on the first C columns
int rd_debug_add(int M, int C, int ald, int bld, int yld, float* a, float* b, float* y) {
    if (M <= 0 || C <= 0 || C % 4 || !a || !b || !y || ald < C || ald % 4 || bld < C || bld % 4 || yld < C || yld % 4) return -1;
    rd::launch_add(a, ald, b, bld, y, yld, M, C, nullptr);
    return debug_finish(nullptr, nullptr);
}

// developer entry: the DB head's tail ConvTranspose2d(24, 24, 2, 2) -> ReLU -> ConvTranspose2d(24, 1, 2, 2) -> sigmoid through
// launch_det_head_tail, on the weights in their checkpoint layouts (device pointers: w1 [24][24][2][2], b1 [24], w2 [24][1][2][2], b2 [1]),
// repacked by the engine's own pack_det_head_tail with the identity for the BatchNorm.  x [N][H][W][xld >= 24], y [N][4 H][4 W].  Synchronised;
// returns 0, -1 on a bad argument or no memory.
int rd_debug_det_head_tail(int N, int H, int W, int xld, float* x, float* w1, float* b1, float* w2, float* b2, float* y) {
    constexpr int kC = 24;
    if (N <= 0 || H <= 0 || W <= 0 || !x || !w1 || !b1 || !w2 || !b2 || !y || xld < kC || xld % 4 || !rd::det_head_tail_supported(kC, kC, 1)) return -1;
    std::vector<float> h1((size_t)kC * kC * 4), hb1(kC), h2((size_t)kC * 4), hb2(1);
    if (hipMemcpy(h1.data(), w1, h1.size() * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hb1.data(), b1, hb1.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(h2.data(), w2, h2.size() * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hb2.data(), b2, 4, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    const std::vector<float> one(kC, 1.f), zero(kC, 0.f);
    std::vector<float> wa, ba, wb;
    rd::pack_det_head_tail(h1.data(), hb1.data(), h2.data(), kC, kC, one.data(), zero.data(), wa, ba, wb);
    std::vector<float> img(wa);                 // one upload: wa | ba | wb | b2 (every part a multiple of 4 floats long before b2)
    img.insert(img.end(), ba.begin(), ba.end());
    img.insert(img.end(), wb.begin(), wb.end());
    img.push_back(hb2[0]);
    float* d = nullptr;
    if (hipMalloc((void**)&d, img.size() * 4) != hipSuccess) return -1;
    (void)hipMemcpy(d, img.data(), img.size() * 4, hipMemcpyHostToDevice);
    rd::launch_det_head_tail(x, xld, N, H, W, d, d + wa.size(), d + wa.size() + ba.size(), d + wa.size() + ba.size() + wb.size(), y, nullptr);
    const int rc = debug_finish(nullptr, nullptr);
    (void)hipFree(d);
    return rc;
}

// developer entry: ONE launch of the fused CTC head on prepared weights (as rd_debug_time_ctc), synchronised, with a free row stride of x
// (xld >= K, a multiple of 4: rows are read as float4).  part = workspace of M * 64 * 4 floats.  *nsplit_out = the split count used,
// *range_out = 1 when the split kernel raised its range flag.  Returns 0, or -1 for a shape the kernels do not take.
int rd_debug_ctc_head(int M, int K, int Ccls, float* x, int xld, float* wp, void* wh, void* wl, float* part, int32_t* idx, float* prob,
                      int nsplit_override, int* nsplit_out, int* range_out) {
    if (range_out) *range_out = 0;
    if (M <= 0 || Ccls <= 0 || K <= 0 || K >= 128 || K % 4 || xld < K || xld % 4 || nsplit_override > 64 || (wh == nullptr) != (wl == nullptr)) return -1;
    rd::CtcParams p{};
    p.x = x; p.xld = xld; p.w = wp; p.M = M; p.K = K; p.C = Ccls; p.part = part;
    p.nsplit = nsplit_override > 0 ? nsplit_override : rd::ctc_head_nsplit(M, Ccls, wh != nullptr);
    p.idx = idx; p.prob = prob;
    p.wh = (const uint16_t*)wh; p.wl = (const uint16_t*)wl;
    if (nsplit_out) *nsplit_out = p.nsplit;
    unsigned* flag = debug_flag_new();
    if (!flag) return -1;
    p.range_flag = flag;
    rd::launch_ctc_head(p, nullptr);
    return debug_finish(flag, range_out);
}

// developer entries for the formula decoder's kernels (csrc/formula_decoder.hip): one synchronised launch each through the decode step's own
// routing on caller-provided device buffers.  rd_debug_dec_gemv returns the dec_gemv_kernel instantiation that ran as
// MT * 10000 + CW * 1000 + KPL * 100 + DB * 10 + DX, 0 where the routing declines the shape (nothing launched); the others return 0.
// All return -1 for arguments the launch cannot take.
int rd_debug_dec_gemv(int M, int K, int N, int act, const float* x, const float* w, const float* bias, const float* ln_g, const float* ln_b,
                      const float* res, float* y) {
    return rd::debug_dec_gemv(M, K, N, act, x, w, bias, ln_g, ln_b, res, y);
}
int rd_debug_dec_attention(int route, int self, int B, int T, float* kc, float* vc, int ldkv, long long seq_stride, const float* x,
                           const float* ln_g, const float* ln_b, const float* w, const float* bias, const float* q, int ldq, const float* kcur,
                           const float* vcur, int ldcur, float* out, int ldo) {
    return rd::debug_dec_attention(route, self, B, T, kc, vc, ldkv, seq_stride, x, ln_g, ln_b, w, bias, q, ldq, kcur, vcur, ldcur, out, ldo);
}
int rd_debug_dec_select(int mode, const float* logits, int V, int B, int step, int64_t* ids, int ids_ld, int32_t* unfinished, int n_unfinished,
                        int max_new, const float* emb, const float* pos, const float* g, const float* b, float* x, int32_t* state_out) {
    return rd::debug_dec_select(mode, logits, V, B, step, reinterpret_cast<long long*>(ids), ids_ld, unfinished, n_unfinished, max_new, emb, pos, g,
                                b, x, state_out);
}

// developer entries for the UniTable decoder's kernels (csrc/table_decoder.hip): one synchronised launch each, through the launch functions of
// decode() / decode_stream(), on caller-provided device buffers.  0 = launched; -1 = arguments the launch cannot take (nothing launched, the
// outputs untouched).  The state words - src / pos of rd_debug_td_attention, and finished .. slot_done of rd_debug_td_select - are HOST int32
// arrays of B entries (forced: [B][forced_ld]) that the entry copies into device state of its own and, for select, back out behind the launch.
int rd_debug_td_gemv(int B, int K, int N, int act, const float* x, const float* w, const float* bias, const float* res, float* y) {
    return rd::debug_td_gemv(B, K, N, act, x, w, bias, res, y);
}
int rd_debug_td_attention(int stream_form, int self, int B, int T, float* kc, float* vc, int ldkv, long long seq_stride, const float* q, int ldq,
                          const float* kcur, const float* vcur, int ldcur, float* out, int ldo, const int32_t* src, const int32_t* pos) {
    return rd::debug_td_attention(stream_form, self, B, T, kc, vc, ldkv, seq_stride, q, ldq, kcur, vcur, ldcur, out, ldo, src, pos);
}
int rd_debug_td_select(int stream_form, const float* logits, int B, const rd_table_decode_cfg* cfg, int max_new, int64_t* ids, int ids_ld,
                       const float* emb, const float* pos, float* x, int step, int32_t* finished, int32_t* boxcount, int32_t* tok,
                       const int32_t* forced, int forced_ld, int32_t* chosen, const int32_t* slot_src, int32_t* slot_pos, int32_t* slot_box,
                       int32_t* slot_done, int32_t* lens) {
    if (!cfg) return -1;
    const int c[6] = {cfg->prefix_id, cfg->eos_id, cfg->pad_id, cfg->bbox_close_id, cfg->bbox_first_id, cfg->bbox_last_id};
    return rd::debug_td_select(stream_form, logits, B, c, max_new, reinterpret_cast<long long*>(ids), ids_ld, emb, pos, x, step, finished, boxcount,
                               tok, forced, forced_ld, chosen, slot_src, slot_pos, slot_box, slot_done, lens);
}

}  // extern "C"
