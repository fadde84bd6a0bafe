// extern "C" surface of librapiddoc_mi355.so - see include/rapiddoc_mi355.h for the contract.
#include <algorithm>
#include <mutex>
#include <string>

#include "api_handle.h"

static thread_local std::string g_create_err;

// the kinds of one family share one C surface (rd_rec_*, rd_det_*): the family comes from the model table (engine.h ModelDesc)
static bool is_family(const rd_handle* h, rd::ModelFamily f) { return h->eng && h->eng->model().family == f; }
static bool is_rec(const rd_handle* h) { return is_family(h, rd::ModelFamily::Recogniser); }
static bool is_det(const rd_handle* h) { return is_family(h, rd::ModelFamily::Detector); }

extern "C" {

const char* rd_version(void) { return "rapiddoc_mi355 0.3 (gfx950; fp32 results, split-fp16 + fp32 MFMA kernels)"; }

rd_handle* rd_create(int device_id, const char* model_kind) {
    try {
        if (!model_kind) throw rd::Error("model_kind is NULL");
        auto* h = new rd_handle();
        h->device = device_id;
        h->kind = model_kind;
        if (h->kind == "ppformulanet_head" || h->kind == "unitable_decoder") {
            int count = 0;
            if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device_id < 0 || device_id >= count) {
                delete h;
                throw rd::Error("no HIP device available (MI355X required; there is no CPU fallback)");
            }
        } else {
            h->eng = new rd::Engine(device_id, model_kind);
        }
        g_create_err.clear();
        return h;
    } catch (const std::exception& e) {
        g_create_err = e.what();
        return nullptr;
    }
}
const char* rd_create_error(void) { return g_create_err.c_str(); }

void rd_destroy(rd_handle* h) {
    if (!h) return;
    delete h->eng;
    if (h->dec) rd::formula_decoder_destroy(h->dec);
    if (h->tdec) rd::table_decoder_destroy(h->tdec);
    delete h;
}
const char* rd_last_error(rd_handle* h) { return h ? h->err.c_str() : "null handle"; }

int rd_load_weights(rd_handle* h, const void* img, size_t nbytes) {
    return guarded(h, [&] {
        if (h->kind == "ppformulanet_head") {
            RD_CHECK(!h->dec, "weights already loaded for this handle");
            h->dec = rd::formula_decoder_create(h->device, img, nbytes);
        } else if (h->kind == "unitable_decoder") {
            RD_CHECK(!h->tdec, "weights already loaded for this handle");
            h->tdec = rd::table_decoder_create(h->device, img, nbytes);
        } else {
            h->eng->load_weights(img, nbytes);
        }
    });
}

int rd_query_workspace(rd_handle* h, int B, int H, int W, int flags, size_t* ws_bytes) {
    return guarded(h, [&] {
        RD_CHECK(ws_bytes, "ws_bytes is NULL");
        RD_CHECK(h->eng, "this model kind owns its workspace");
        if (is_rec(h) && !(flags & rd::REC_STAGE_TAIL)) H = 48;
        *ws_bytes = h->eng->workspace_bytes(B, H, W, flags);
    });
}

int rd_det_forward(rd_handle* h, const float* x, int B, int H, int W, float* prob, void* ws, size_t ws_bytes, void* stream) {
    return guarded(h, [&] {
        RD_CHECK(is_det(h), "handle is not a detector (ppocrv6_det / ppocrv5_det_server / ppocrv5_det_mobile / ppocrv3_det_mobile) model");
        RD_CHECK(x && prob && B > 0, "null input/output");
        h->eng->run(B, H, W, 0, {(void*)x, (void*)prob}, ws, ws_bytes, (hipStream_t)stream);
    });
}

int rd_det_forward_ex(rd_handle* h, const float* x, int B, int H, int W, float* prob, int flags, float* aux, void* ws, size_t ws_bytes,
                      void* stream) {
    return guarded(h, [&] {
        RD_CHECK(is_det(h), "handle is not a detector (ppocrv6_det / ppocrv5_det_server / ppocrv5_det_mobile / ppocrv3_det_mobile) model");
        RD_CHECK(x && prob && B > 0, "null input/output");
        RD_CHECK((flags & ~RD_DET_WANT_NECK) == 0, "rd_det_forward_ex: unknown flag");
        if (flags & RD_DET_WANT_NECK) {
            RD_CHECK(h->eng->model().det_want_neck,
                     "RD_DET_WANT_NECK is offered by ppocrv5_det_server, ppocrv5_det_mobile and ppocrv3_det_mobile only");
            RD_CHECK(aux, "aux_dev is NULL");
        }
        h->eng->run(B, H, W, flags, {(void*)x, (void*)prob, (void*)aux}, ws, ws_bytes, (hipStream_t)stream);
    });
}

int rd_cls_forward(rd_handle* h, const float* x, int B, int H, int W, float* prob, int flags, float* aux, void* ws, size_t ws_bytes, void* stream) {
    return guarded(h, [&] {
        RD_CHECK(h->eng && h->eng->kind() == "ppocr_cls_mobile", "handle is not a text-line classifier (ppocr_cls_mobile) model");
        RD_CHECK(x && prob && B > 0, "null input/output");
        RD_CHECK((flags & ~RD_CLS_WANT_AUX) == 0, "rd_cls_forward: unknown flag");
        RD_CHECK(!(flags & RD_CLS_WANT_AUX) || aux, "aux_dev is NULL");
        h->eng->run(B, H, W, flags, {(void*)x, (void*)prob, (void*)aux}, ws, ws_bytes, (hipStream_t)stream);
    });
}

int rd_table_encoder_forward(rd_handle* h, const float* x, int B, int H, int W, float* memory, void* ws, size_t ws_bytes, void* stream) {
    return guarded(h, [&] {
        RD_CHECK(h->eng && h->eng->kind() == "unitable_encoder", "handle is not a table-structure encoder (unitable_encoder) model");
        RD_CHECK(x && memory && B > 0, "null input/output");
        h->eng->run(B, H, W, 0, {(void*)x, (void*)memory}, ws, ws_bytes, (hipStream_t)stream);
    });
}


int rd_table_decode(rd_handle* h, const float* memory, int B, int S, int max_new_tokens, const rd_table_decode_cfg* cfg, int64_t* ids, int32_t* n_tokens,
                    void* stream) {
    return guarded(h, [&] {
        RD_CHECK(h->kind == "unitable_decoder" && h->tdec, "handle is not a loaded table-structure decoder (unitable_decoder)");
        int c[6];
        table_cfg6(cfg, c);
        rd::table_decoder_decode(h->tdec, memory, B, S, max_new_tokens, c, (long long*)ids, (int*)n_tokens, (hipStream_t)stream, nullptr, nullptr, nullptr,
                                 nullptr, nullptr);
    });
}
int rd_table_decode_stream(rd_handle* h, const float* memory, int N, int S, int max_new_tokens, int slots, const rd_table_decode_cfg* cfg, int64_t* ids,
                           int32_t* lens, rd_table_stream_stats* stats, void* stream) {
    return guarded(h, [&] {
        RD_CHECK(h->kind == "unitable_decoder" && h->tdec, "handle is not a loaded table-structure decoder (unitable_decoder)");
        int c[6];
        table_cfg6(cfg, c);
        rd::table_decoder_decode_stream(h->tdec, memory, N, S, max_new_tokens, slots, c, (long long*)ids, (int*)lens, stats, (hipStream_t)stream, nullptr,
                                        nullptr, nullptr, 0);
    });
}

int rd_line_flip180_batch(int device_id, const rd_line_crop_desc* descs, int n, const float* cls_prob, float thresh, uint8_t* scratch,
                          int32_t* flipped_out, void* stream) {
    if (!descs || !cls_prob || !scratch || !flipped_out || n < 0) return 1;
    if (hipSetDevice(device_id) != hipSuccess) return 1;
    if (rd::launch_line_flip180(reinterpret_cast<const rd::LineCropDesc*>(descs), n, cls_prob, thresh, scratch, flipped_out, (hipStream_t)stream) != 0) return 1;
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int rd_rec_forward(rd_handle* h, const float* x, int B, int W, int32_t* idx, float* prob, float* full, int flags, void* ws,
                   size_t ws_bytes, void* stream) {
    return guarded(h, [&] {
        RD_CHECK(is_rec(h), "handle is not a recogniser (ppocrv6_rec / ppocrv5_rec_server / ppocrv5_rec_mobile / ppocr_rec_mv1e) model");
        RD_CHECK(x && idx && prob && B > 0, "null input/output");
        if (flags & (RD_REC_WANT_SOFTMAX | RD_REC_WANT_LOGITS | RD_REC_WANT_NECK)) RD_CHECK(full, "full_btc_dev is NULL");
        RD_CHECK(!((flags & RD_REC_WANT_SOFTMAX) && (flags & RD_REC_WANT_LOGITS)), "choose softmax OR logits");
        RD_CHECK(!(flags & RD_REC_WANT_NECK) || flags == RD_REC_WANT_NECK, "RD_REC_WANT_NECK goes with no other flag");
        h->eng->run(B, 48, W, flags, {(void*)x, (void*)idx, (void*)prob, (void*)full}, ws, ws_bytes, (hipStream_t)stream);
    });
}
int rd_rec_token_dim(rd_handle* h) { return (h && is_rec(h)) ? h->eng->rec_token_dim() : -1; }
int rd_rec_backbone_forward(rd_handle* h, const float* x, int B, int W, float* tokens, void* ws, size_t ws_bytes, void* stream) {
    return guarded(h, [&] {
        RD_CHECK(is_rec(h), "handle is not a recogniser (ppocrv6_rec / ppocrv5_rec_server / ppocrv5_rec_mobile / ppocr_rec_mv1e) model");
        RD_CHECK(x && tokens && B > 0, "null input/output");
        h->eng->run(B, 48, W, rd::REC_STAGE_BACKBONE, {(void*)x, (void*)tokens}, ws, ws_bytes, (hipStream_t)stream);
    });
}
int rd_rec_backbone_forward_lines(rd_handle* h, const float* x, int B, int W, const int32_t* line_tab, float* tokens, void* ws, size_t ws_bytes,
                                  void* stream) {
    return guarded(h, [&] {
        RD_CHECK(is_rec(h), "handle is not a ppocrv6_rec / ppocrv5_rec_mobile / ppocr_rec_mv1e model");
        RD_CHECK(h->eng->model().rec_line_widths, "rd_rec_backbone_forward_lines: per-line widths inside one backbone launch are out of scope for " +
                                                      h->eng->kind() + " (run the backbone stage once per padded width)");
        RD_CHECK(x && tokens && line_tab && B > 0, "null input/output");
        h->eng->run(B, 48, W, rd::REC_STAGE_BACKBONE | rd::REC_LINE_WIDTHS, {(void*)x, (void*)tokens, (void*)line_tab}, ws, ws_bytes,
                    (hipStream_t)stream);
    });
}
int rd_rec_tail_forward(rd_handle* h, const float* tokens, int n_tokens, int n_lines, int max_tokens, const int32_t* seg,
                        const int32_t* tokinfo, int32_t* idx, float* prob, void* ws, size_t ws_bytes, void* stream) {
    return guarded(h, [&] {
        RD_CHECK(is_rec(h), "handle is not a recogniser (ppocrv6_rec / ppocrv5_rec_server / ppocrv5_rec_mobile / ppocr_rec_mv1e) model");
        RD_CHECK(tokens && seg && tokinfo && idx && prob && n_tokens > 0 && n_lines > 0 && max_tokens > 0, "null input/output");
        h->eng->run(n_lines, max_tokens, n_tokens, rd::REC_STAGE_TAIL,
                    {(void*)tokens, (void*)idx, (void*)prob, nullptr, (void*)seg, (void*)tokinfo}, ws, ws_bytes, (hipStream_t)stream);
    });
}
int rd_rec_seq_len(int W) {
    if (W < 16) return 0;
    const int w1 = (W - 1) / 2 + 1, w2 = (w1 - 1) / 2 + 1;
    return (w2 - 2) / 2 + 1;
}
const char* rd_backbone_name(rd_handle* h) { return (h && h->eng) ? h->eng->backbone().c_str() : ""; }
int rd_rec_num_classes(rd_handle* h) { return (h && h->eng) ? h->eng->n_classes() : -1; }

int rd_backbone_forward(rd_handle* h, const float* x, int B, int H, int W, float* const feats[4], void* ws, size_t ws_bytes,
                        void* stream) {
    return guarded(h, [&] {
        RD_CHECK(h->eng && h->eng->kind() == "pphgnetv2_b4", "handle is not a pphgnetv2_b4 model");
        RD_CHECK(x && feats && feats[0] && feats[1] && feats[2] && feats[3], "null input/output");
        h->eng->run(B, H, W, 0, {(void*)x, (void*)feats[0], (void*)feats[1], (void*)feats[2], (void*)feats[3]}, ws, ws_bytes,
                    (hipStream_t)stream);
    });
}

int rd_formula_encoder_forward(rd_handle* h, const float* x, int B, int C, int H, int W, float* enc, void* ws, size_t ws_bytes,
                               void* stream) {
    return guarded(h, [&] {
        RD_CHECK(h->eng && h->eng->kind() == "pphgnetv2_b6_formula", "handle is not a pphgnetv2_b6_formula model");
        RD_CHECK(x && enc && B > 0 && (C == 1 || C == 3), "null input/output or channel count not 1/3");
        h->eng->run(B, H, W, C == 1 ? 1 : 0, {(void*)x, (void*)enc}, ws, ws_bytes, (hipStream_t)stream);
    });
}

int rd_formula_decode(rd_handle* h, const float* enc, int B, int S, int max_new_tokens, int64_t* ids, int32_t* n_cols, void* stream) {
    return guarded(h, [&] {
        RD_CHECK(h->kind == "ppformulanet_head" && h->dec, "handle is not a loaded ppformulanet_head model");
        RD_CHECK(enc && ids && n_cols, "null input/output");
        *n_cols = rd::formula_decoder_decode(h->dec, enc, B, S, max_new_tokens, reinterpret_cast<long long*>(ids), (hipStream_t)stream, nullptr,
                                             nullptr);
    });
}
int rd_formula_decode_stream(rd_handle* h, const float* enc, int N, int S, int max_new_tokens, int slots, int64_t* ids, int32_t* lens,
                             rd_formula_stream_stats* stats, void* stream) {
    return guarded(h, [&] {
        RD_CHECK(h->kind == "ppformulanet_head" && h->dec, "handle is not a loaded ppformulanet_head model");
        RD_CHECK(enc && ids && lens, "null input/output");
        rd::formula_decoder_decode_stream(h->dec, enc, N, S, max_new_tokens, slots, reinterpret_cast<long long*>(ids), (int*)lens, stats,
                                          (hipStream_t)stream, nullptr, nullptr, nullptr, 0);
    });
}
int rd_formula_max_new_tokens(rd_handle* h) { return (h && h->dec) ? rd::formula_decoder_max_new(h->dec) : -1; }

int rd_preproc_resize_norm(int device_id, const uint8_t* src, int H, int W, int OH, int OW, const float mean[3],
                           const float std[3], float scale, int interp, int swap_rb, float* out, void* stream) {
    if (!src || !out || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || (interp != 1 && interp != 2)) return 1;
    if (hipSetDevice(device_id) != hipSuccess) return 1;
    rd::PreprocParams p{};
    p.src = src; p.H = H; p.W = W; p.dst = out; p.OH = OH; p.OW = OW;
    for (int i = 0; i < 3; ++i) { p.mean[i] = mean ? mean[i] : 0.f; p.inv_std[i] = 1.f / (std ? std[i] : 1.f); }
    p.scale = scale; p.interp = interp; p.swap_rb = swap_rb;
    rd::launch_preproc_resize_norm(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int rd_preproc_resize_norm_batch(int device_id, const uint8_t* src, int P, int H, int W, int OH, int OW, const float mean[3],
                                 const float std[3], float scale, int interp, int swap_rb, float* out, void* stream) {
    if (!src || !out || P <= 0 || P > 65535 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || (interp != 1 && interp != 2)) return 1;
    if (hipSetDevice(device_id) != hipSuccess) return 1;
    rd::PreprocParams p{};
    p.src = src; p.H = H; p.W = W; p.dst = out; p.OH = OH; p.OW = OW;
    for (int i = 0; i < 3; ++i) { p.mean[i] = mean ? mean[i] : 0.f; p.inv_std[i] = 1.f / (std ? std[i] : 1.f); }
    p.scale = scale; p.interp = interp; p.swap_rb = swap_rb;
    p.batch = P; p.src_stride = (size_t)H * W * 3; p.dst_stride = (size_t)3 * OH * OW;
    rd::launch_preproc_resize_norm(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int rd_preproc_resize_norm_sources(int device_id, const rd_resize_source_desc* descs_host, const rd_resize_source_desc* descs_dev, int n,
                                   const float mean[3], const float std[3], float scale, int interp, int swap_rb, float* out_dev,
                                   int64_t out_floats, void* stream) {
    std::string err;
    const int rc = rd::launch_preproc_resize_norm_sources(device_id, descs_host, descs_dev, n, mean, std, scale, interp, swap_rb, out_dev,
                                                          out_floats, (hipStream_t)stream, err);
    if (rc != 0) g_create_err = err;
    return rc;
}

int rd_preproc_resize_aa_norm(int device_id, const uint8_t* src, int H, int W, int OH, int OW, const float mean[3], const float std[3],
                              int swap_rb, float* out, uint8_t* out_u8, void* stream) {
    std::string err;
    const int rc = rd::launch_resize_aa_norm(device_id, src, H, W, OH, OW, mean, std, swap_rb, out, out_u8, (hipStream_t)stream, err);
    if (rc != 0) g_create_err = err;        // no handle: the calling thread's rd_create_error() carries the message
    return rc;
}

int rd_formula_margin_boxes(int device_id, const rd_formula_crop* descs_dev, int n, int32_t* boxes_dev, void* stream) {
    std::string err;
    const int rc = rd::launch_formula_margin_boxes(device_id, descs_dev, n, boxes_dev, (hipStream_t)stream, err);
    if (rc != 0) g_create_err = err;
    return rc;
}

int rd_formula_preproc_plan(int w, int h, rd_formula_plan* plan) {
    if (!plan) { g_create_err = "rd_formula_preproc_plan: plan is NULL"; return 1; }
    rd::formula_preproc_plan(w, h, plan);
    return 0;
}

int rd_formula_preproc_batch(int device_id, const rd_formula_crop* descs_host, const int32_t* boxes_host, int n, float* out, uint8_t* out_u8,
                             void* stream) {
    std::string err;
    const int rc = rd::launch_formula_preproc_batch(device_id, descs_host, boxes_host, n, out, out_u8, (hipStream_t)stream, err);
    if (rc != 0) g_create_err = err;
    return rc;
}

size_t rd_checkbox_workspace(int P, int H, int W, int max_runs, int max_cand, size_t* offsets) {
    return rd::checkbox_workspace_bytes(P, H, W, max_runs, max_cand, offsets);
}

int rd_checkbox_detect_device(int device_id, const uint8_t* pages_dev, int P, int H, int W, int bgr, int max_runs, int max_cand, void* ws_dev,
                              size_t ws_bytes, rd_checkbox_page* hdr_dev, rd_checkbox_cand* cands_dev, void* stream) {
    std::string err;
    const int rc = rd::launch_checkbox_detect(device_id, pages_dev, P, H, W, bgr, max_runs, max_cand, ws_dev, ws_bytes, hdr_dev, cands_dev,
                                              (hipStream_t)stream, err);
    if (rc != 0) g_create_err = err;
    return rc;
}

int rd_checkbox_finish(const rd_checkbox_cand* cands, int n, int H, int W, rd_checkbox_box* out, int max_out, int32_t* n_out) {
    std::string err;
    const int rc = rd::checkbox_finish(cands, n, H, W, out, max_out, n_out, err);
    if (rc != 0) g_create_err = err;
    return rc;
}

size_t rd_region_canvases_workspace(int n, int gh, int gw) { return rd::region_canvases_workspace_bytes(n, gh, gw); }

int rd_region_canvases(int device_id, const rd_region_desc* descs_dev, int n, const int32_t* pts_dev, const int32_t* boxes_dev, int gh, int gw,
                       uint8_t* canv_dev, uint8_t* det_canv_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    std::string err;
    const int rc = rd::launch_region_canvases(device_id, descs_dev, n, pts_dev, boxes_dev, gh, gw, canv_dev, det_canv_dev, ws_dev, ws_bytes,
                                              (hipStream_t)stream, err);
    if (rc != 0) g_create_err = err;
    return rc;
}

int rd_stage_canvases(int device_id, const rd_stage_desc* descs_host, const rd_stage_desc* descs_dev, int n, void* stream) {
    std::string err;
    const int rc = rd::launch_stage_canvases(device_id, descs_host, descs_dev, n, (hipStream_t)stream, err);
    if (rc != 0) g_create_err = err;
    return rc;
}

int rd_crop_resize_norm_batch(int device_id, const uint8_t* pages, int P, int H, int W, const rd_crop_desc* descs, int n,
                              int out_h, int out_w_padded, const float mean[3], const float std[3], float scale, int swap_rb,
                              float* out, void* stream) {
    static_assert(sizeof(rd_crop_desc) == sizeof(rd::CropDesc), "rd_crop_desc layout");
    if (!pages || !descs || !out || P <= 0 || n < 0 || out_h <= 0 || out_w_padded <= 0) return 1;
    if (hipSetDevice(device_id) != hipSuccess) return 1;
    rd::CropBatchParams p{};
    p.pages = pages; p.H = H; p.W = W; p.page_stride = (size_t)H * W * 3;
    p.descs = reinterpret_cast<const rd::CropDesc*>(descs); p.n = n;
    p.dst = out; p.OH = out_h; p.OWp = out_w_padded;
    for (int i = 0; i < 3; ++i) { p.mean[i] = mean ? mean[i] : 0.f; p.inv_std[i] = 1.f / (std ? std[i] : 1.f); }
    p.scale = scale; p.swap_rb = swap_rb;
    rd::launch_crop_resize_norm_batch(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int rd_line_crops_batch(int device_id, const uint8_t* pages, int P, int H, int W, const rd_line_crop_desc* descs, int n,
                        int64_t max_crop_pixels, uint8_t* scratch, int out_h, int out_w_padded, int swap_rb, float* out, void* stream) {
    static_assert(sizeof(rd_line_crop_desc) == sizeof(rd::LineCropDesc), "rd_line_crop_desc layout");
    if (!pages || !descs || !out || !scratch || P <= 0 || n < 0 || out_h <= 0 || out_w_padded <= 0 || max_crop_pixels <= 0) return 1;
    if (hipSetDevice(device_id) != hipSuccess) return 1;
    rd::LineCropParams p{};
    p.pages = pages; p.H = H; p.W = W; p.page_stride = (size_t)H * W * 3;
    p.descs = reinterpret_cast<const rd::LineCropDesc*>(descs); p.n = n;
    p.scratch = scratch; p.max_crop_pixels = (long)max_crop_pixels;
    p.dst = out; p.OH = out_h; p.OWp = out_w_padded; p.swap_rb = swap_rb;
    if (rd::launch_line_crops(p, (hipStream_t)stream) != 0) return 1;
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int rd_line_warp_batch(int device_id, const uint8_t* pages, int P, int H, int W, const rd_line_crop_desc* descs, int n,
                       int64_t max_crop_pixels, uint8_t* scratch, void* stream) {
    if (!pages || !descs || !scratch || P <= 0 || n < 0 || max_crop_pixels <= 0) return 1;
    if (hipSetDevice(device_id) != hipSuccess) return 1;
    rd::LineCropParams p{};
    p.pages = pages; p.H = H; p.W = W; p.page_stride = (size_t)H * W * 3;
    p.descs = reinterpret_cast<const rd::LineCropDesc*>(descs); p.n = n;
    p.scratch = scratch; p.max_crop_pixels = (long)max_crop_pixels;
    if (rd::launch_line_warp(p, (hipStream_t)stream) != 0) return 1;
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
int rd_line_warp_sources(int device_id, const rd_line_source_desc* descs_host, const rd_line_source_desc* descs_dev, int n,
                         uint8_t* scratch, int64_t scratch_bytes, void* stream) {
    std::string err;
    const int rc = rd::launch_line_warp_sources(device_id, descs_host, descs_dev, n, scratch, scratch_bytes, (hipStream_t)stream, err);
    if (rc != 0) g_create_err = err;
    return rc;
}
int rd_line_resize_norm_batch(int device_id, const rd_line_crop_desc* descs, int n, const uint8_t* scratch, int out_h, int out_w_padded,
                              int swap_rb, float* out, void* stream) {
    if (!descs || !scratch || !out || n < 0 || out_h <= 0 || out_w_padded <= 0) return 1;
    if (hipSetDevice(device_id) != hipSuccess) return 1;
    rd::LineCropParams p{};
    p.descs = reinterpret_cast<const rd::LineCropDesc*>(descs); p.n = n;
    p.scratch = const_cast<uint8_t*>(scratch);
    p.dst = out; p.OH = out_h; p.OWp = out_w_padded; p.swap_rb = swap_rb;
    if (rd::launch_line_resize_norm(p, (hipStream_t)stream) != 0) return 1;
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int rd_ctc_collapse(int device_id, const int32_t* idx, const float* prob, int B, int T, const uint8_t* ctab, int max_len, int n_classes,
                    uint8_t* out, int row_bytes, void* stream) {
    if (!idx || !prob || !ctab || !out || B < 0 || T <= 0 || max_len <= 0 || n_classes <= 0) return 1;
    if (hipSetDevice(device_id) != hipSuccess) return 1;
    if (rd::launch_ctc_collapse(idx, prob, B, T, nullptr, ctab, max_len, n_classes, out, row_bytes, nullptr, nullptr, (hipStream_t)stream) != 0) return 1;
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int rd_ctc_collapse_lines(int device_id, const int32_t* idx, const float* prob, int n_lines, const int32_t* seg, int max_tokens,
                          const uint8_t* ctab, int max_len, int n_classes, uint8_t* out, int row_bytes, uint16_t* kept_cols, float* kept_conf,
                          void* stream) {
    if (!idx || !prob || !seg || !ctab || !out || n_lines < 0 || max_tokens <= 0 || max_len <= 0 || n_classes <= 0) return 1;
    if (hipSetDevice(device_id) != hipSuccess) return 1;
    if (rd::launch_ctc_collapse(idx, prob, n_lines, max_tokens, seg, ctab, max_len, n_classes, out, row_bytes, kept_cols, kept_conf,
                                (hipStream_t)stream) != 0)
        return 1;
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// ---- RT-DETR-family head operators (preparation only, parity unpinned: include/rapiddoc_mi355.h) ----------------------------------
int rd_msdeform_attn(int device_id, const float* value, const int32_t* shapes, const int32_t* level_start, const float* loc, const float* attn,
                     float* out, int B, int S, int H, int D, int Q, int L, int P, void* stream) {
    if (!value || !shapes || !level_start || !loc || !attn || !out || B < 0 || S <= 0 || H <= 0 || D <= 0 || Q < 0 || L <= 0 || P <= 0 || H * D > 1024)
        return 1;
    if (hipSetDevice(device_id) != hipSuccess) return 1;
    rd::launch_msdeform_attn(value, shapes, level_start, loc, attn, out, B, S, H, D, Q, L, P, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int rd_topk_rows(int device_id, const float* scores, int rows, int n, int k, float* out_vals, int32_t* out_idx, void* stream) {
    if (!scores || !out_vals || !out_idx || rows < 0 || n <= 0 || k <= 0 || k > 1024 || k > n) return 1;
    if (hipSetDevice(device_id) != hipSuccess) return 1;
    rd::launch_topk_rows(scores, rows, n, k, out_vals, out_idx, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

size_t rd_encoder_layer_workspace(int M, int Dm, int F) {
    if (M <= 0 || Dm <= 0 || F <= 0) return 0;
    return ((size_t)M * Dm * 3 /* x + pos, attention output, post-norm-1 */ + (size_t)M * 3 * Dm /* q | k | v */ + (size_t)M * F) * sizeof(float);
}

// One post-norm transformer encoder layer over B sequences of T tokens (M = B * T rows of Dm):
//   a = MHA(q = k = x + pos, v = x);  y1 = LN1(x + a Wo^T + bo);  out = LN2(y1 + W2 act(W1 y1 + b1) + b2)
// in_w [3 Dm][Dm] / in_b [3 Dm] = the packed q | k | v projection (nn.MultiheadAttention's in_proj), head_dim = Dm / heads in {16, 32}.
// Composed from the engine's kernels: fp32-MFMA GEMMs (launch_conv_igemm on raw [N][K] weights), launch_attention, launch_layernorm.
int rd_encoder_layer(int device_id, const float* x, const float* pos, int B, int T, int Dm, int heads, int F, int act, const float* in_w,
                     const float* in_b, const float* out_w, const float* out_b, const float* ln1_g, const float* ln1_b, const float* w1,
                     const float* b1, const float* w2, const float* b2, const float* ln2_g, const float* ln2_b, float eps, float* out, void* ws,
                     size_t ws_bytes, void* stream) {
    const int M = B * T;
    if (!x || !in_w || !out_w || !w1 || !w2 || !ln1_g || !ln1_b || !ln2_g || !ln2_b || !out || !ws || B <= 0 || T <= 0 || heads <= 0 ||
        Dm % heads != 0 || Dm % 4 != 0 || F % 4 != 0 || ws_bytes < rd_encoder_layer_workspace(M, Dm, F))
        return 1;
    const int hd = Dm / heads;
    if (hd != 16 && hd != 32) return 1;
    if (hipSetDevice(device_id) != hipSuccess) return 1;
    hipStream_t s = (hipStream_t)stream;
    float* xp = (float*)ws;
    float* att = xp + (size_t)M * Dm;
    float* y1 = att + (size_t)M * Dm;
    float* qkv = y1 + (size_t)M * Dm;
    float* ff = qkv + (size_t)M * 3 * Dm;
    auto gemm = [&](const float* a, int K, const float* w, const float* b, int N, float* y, int yld, int a_act, const float* res) {
        rd::ConvParams p{};
        p.x = a; p.xld = K; p.N = 1; p.H = 1; p.W = M; p.Cin = K;
        p.w = w; p.bias = b; p.y = y; p.yld = yld; p.OH = 1; p.OW = M; p.Cout = N;
        p.KH = p.KW = p.SH = p.SW = 1;
        p.res = res; p.rld = N;
        p.act = a_act; p.out_mode = rd::OUT_NHWC;
        p.M = M; p.K = K; p.Ng = N;
        rd::launch_conv_igemm(p, s);
    };
    try {
        const float* qk_in = x;
        if (pos) {
            rd::launch_add(x, Dm, pos, Dm, xp, Dm, M, Dm, s);
            qk_in = xp;
        }
        gemm(qk_in, Dm, in_w, in_b, 2 * Dm, qkv, 3 * Dm, rd::ACT_NONE, nullptr);                                   // q | k from x + pos
        gemm(x, Dm, in_w + (size_t)2 * Dm * Dm, in_b ? in_b + 2 * Dm : nullptr, Dm, qkv + 2 * Dm, 3 * Dm, rd::ACT_NONE, nullptr);   // v from x
        rd::launch_attention(qkv, att, B, T, heads, hd, 1.0f / std::sqrt((float)hd), s);
        gemm(att, Dm, out_w, out_b, Dm, xp, Dm, rd::ACT_NONE, x);                                                   // x + a Wo^T + bo
        rd::launch_layernorm(xp, Dm, y1, Dm, ln1_g, ln1_b, M, Dm, eps, s);
        gemm(y1, Dm, w1, b1, F, ff, F, act, nullptr);
        gemm(ff, F, w2, b2, Dm, xp, Dm, rd::ACT_NONE, y1);
        rd::launch_layernorm(xp, Dm, out, Dm, ln2_g, ln2_b, M, Dm, eps, s);
    } catch (...) {
        return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

size_t rd_db_boxes_workspace(int B, int H, int W, int max_runs, int max_candidates) {
    (void)W;
    if (B <= 0 || H <= 0 || max_runs <= 0 || max_candidates <= 0) return 0;
    return rd::db_boxes_workspace_bytes(B, H, max_runs, max_candidates);
}
int rd_db_boxes_device(int device_id, const float* prob, int B, int H, int W, const int32_t* src_hw_dev, float thresh, float box_thresh,
                       float unclip_ratio, int use_dilation, int max_candidates, int max_runs, void* ws, size_t ws_bytes, rd_text_box* out,
                       int max_out, int32_t* n_out, void* stream) {
    if (!prob || !src_hw_dev || !ws || !out || !n_out || B < 0 || H <= 0 || W <= 0) return 1;
    if (hipSetDevice(device_id) != hipSuccess) return 1;
    if (rd::launch_db_boxes(prob, B, H, W, src_hw_dev, thresh, box_thresh, unclip_ratio, use_dilation, max_candidates, max_runs, ws, ws_bytes,
                            out, max_out, n_out, (hipStream_t)stream) != 0)
        return 1;
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int rd_set_precision(rd_handle* h, const char* mode) {
    return guarded(h, [&] {
        RD_CHECK(h->eng, "precision modes apply to the network engines");
        const std::string m = mode ? mode : "";
        RD_CHECK(m == "auto" || m == "fp32" || m == "h3", "precision must be auto, fp32 or h3");
        h->eng->set_precision(m == "h3" ? rd::Engine::PREC_H3 : m == "fp32" ? rd::Engine::PREC_FP32 : rd::Engine::PREC_AUTO);
    });
}
int rd_range_status(rd_handle* h, void* stream) {
    int out = 0;
    const int rc = guarded(h, [&] { if (h->eng) out = h->eng->take_range_flag((hipStream_t)stream); });
    return rc != 0 ? -1 : out;
}

int rd_plan_stats(rd_handle* h, uint64_t* plans_built, uint64_t* graph_captures, uint64_t* graph_replays) {
    if (!h || !h->eng) return 1;
    if (plans_built) *plans_built = h->eng->plans_built();
    if (graph_captures) *graph_captures = h->eng->graph_captures();
    if (graph_replays) *graph_replays = h->eng->graph_replays();
    return 0;
}

int rd_set_profiling(rd_handle* h, int on) {
    return guarded(h, [&] { if (h->eng) h->eng->set_profiling(on != 0); });
}
const char* rd_profile_json(rd_handle* h) {
    if (!h || !h->eng) return "[]";
    h->prof = h->eng->profile_json();
    return h->prof.c_str();
}

}  // extern "C"
