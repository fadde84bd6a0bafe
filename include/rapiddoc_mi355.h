/* rapiddoc_mi355 - C ABI of the MI355X-native page-inference engine (gfx950).
 *
 * Drop-in boundary for RapidDoc's per-page neural forward passes.  Each entry point replaces what one
 * `InferSession.__call__` of the reference does (paths relative to the RapidDoc source tree):
 *
 *   rd_det_forward       <- OCR det session:   rapid_doc/model/ocr/torch.py:171-192 (`maps`),
 *                           called from rapid_doc/model/ocr/rapid_ocr.py:528 (`text_detector.session`)
 *   rd_rec_forward       <- OCR rec session:   rapid_doc/model/ocr/torch.py:171-192 (`softmax(ctc_logits)`),
 *                           called from rapid_doc/model/ocr/rapid_ocr.py:443 (`text_recognizer.session`), plus the
 *                           argmax/max half of rapidocr's CTCLabelDecode (rapid_ocr.py:444-449)
 *   rd_backbone_forward  <- the PPHGNetV2-B4 backbone inside the PP-DocLayout ONNX graph:
 *                           rapid_doc/model/layout/rapid_layout_self/inference_engine/onnxruntime/main.py:61-78
 *                           (network definition: .../formula/rapid_formula_self/networks/backbones/rec_pphgnetv2.py:1445-1477)
 *   rd_preproc_resize_norm <- PPPreProcess: .../model_handler/pp_doclayout/pre_process.py:22-42
 *   rd_preproc_resize_aa_norm <- UniTable's TablePreprocess (PIL Resize + ToTensor + Normalize):
 *                           rapid_doc/model/table/rapid_table_self/table_structure/unitable/pre_process.py
 *   rd_formula_margin_boxes, rd_formula_preproc_plan, rd_formula_preproc_batch <- UniMERNetImgDecode + UniMERNetTestTransform +
 *                           LatexImageFormat: .../model_handler/pp_formulanet_plus/pre_process.py:39-246
 *   rd_region_canvases   <- crop_img + _apply_mask_boxes_to_image for a batch of regions: rapid_doc/utils/model_utils.py:90-124,
 *                           rapid_doc/backend/pipeline/analyze_utils.py:82-103,131-145
 *   rd_stage_pack, rd_stage_canvases <- the numpy crops BatchAnalyze hands to a `custom_model` (batch_analyze.py:258-331) and the white
 *                           canvases of `_run_ocr_det_batch` (analyze_utils.py:150-189), for a whole call: pack, one upload, one launch
 *   rd_line_warp_sources <- get_rotate_crop_image for the text lines of MANY region images at once (rapid_doc/utils/ocr_utils.py:494-537,
 *                           called per line by get_ocr_result_list, :361-432): every line names its own source image, one launch
 *   rd_load_weights      <- `_load_state_dict` + `load_state_dict`: rapid_doc/model/ocr/torch.py:82-110
 *
 * Conventions: every pointer named *_dev is a DEVICE pointer on the handle's GPU (PyTorch-ROCm
 * `tensor.data_ptr()` works); images are NCHW float32 exactly like the numpy arrays the reference hands to
 * its sessions; `stream` is a hipStream_t passed as void* (NULL = default stream); functions return 0 on
 * success, non-zero on failure with the message in rd_last_error(handle).  `ws_dev` may be NULL, in which
 * case the handle owns (and grows) its own workspace.  One handle = one network on one device; a handle is
 * not thread-safe, different handles are independent.  There is no CPU fallback: rd_create fails if no
 * HIP device is present.
 */
#ifndef RAPIDDOC_MI355_H
#define RAPIDDOC_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rd_handle rd_handle;

/* rd_rec_forward flags */
#define RD_REC_UNFUSED_CTC 1  /* materialise logits, then row statistics (validation path)              */
#define RD_REC_WANT_SOFTMAX 2 /* also write softmax probabilities [B,T,C] (the reference session output) */
#define RD_REC_WANT_LOGITS 4  /* also write raw logits [B,T,C]                                          */
#define RD_REC_WANT_NECK 64   /* "ppocrv5_rec_server" / "ppocrv5_rec_mobile" / "ppocr_rec_mv1e" only, instead of the two above: full_btc_dev receives the neck's output
                               * [B,T,120] ("ppocr_rec_mv1e": [B,T,64]) (the CTC classifier's input); idx / prob come from the fused head as with flags 0 */

const char* rd_version(void);
/* model_kind: "ppocrv6_det" | "ppocrv5_det_server" (PPHGNetV2-B4 + LKPAN + PFHeadLocal; rd_det_forward / rd_det_forward_ex) |
 * "ppocrv5_det_mobile" (PPLCNetV3 scale 0.75 + RSEFPN + DBHead; the same two calls) |
 * "ppocrv3_det_mobile" (MobileNetV3 large scale 0.5 without SE + RSEFPN + DBHead - multi_ / en_PP-OCRv3_det_mobile; the same two calls) |
 * "ppocr_cls_mobile" (MobileNetV3 small scale 0.35 with squeeze-excite + ClsHead - ch_ptocr_mobile_v2.0_cls_mobile, the 0 / 180 degree text-line classifier; rd_cls_forward) |
 * "unitable_encoder" (the ViT-B encoder of the UniTable table-structure recogniser; rd_table_encoder_forward) |
 * "unitable_decoder" (its GPT decoder and greedy loop; rd_table_decode) | "ppocrv6_rec" | "ppocrv5_rec_server" (PPHGNetV2-B4 + SVTR neck + CTC; every rd_rec_* call except
 * rd_rec_backbone_forward_lines) | "ppocrv5_rec_mobile" (PPLCNetV3 scale 0.95 + the same SVTR neck + CTC; every rd_rec_* call) | "ppocr_rec_mv1e" (MobileNetV1Enhance scale 0.5 + SVTR neck dims 64 + CTC:
 * the ten multilingual PP-OCRv3 / v4 mobile files latin_ / cyrillic_ / chinese_cht_PP-OCRv3_rec_mobile, arabic_ / korean_ / japan_ / ta_ / te_ / ka_ /
 * devanagari_PP-OCRv4_rec_mobile, which differ in their class count only; every rd_rec_* call) | "pphgnetv2_b4" | "pphgnetv2_b6_formula" | "ppformulanet_head".  NULL on failure -> rd_create_error(). */
rd_handle* rd_create(int device_id, const char* model_kind);
const char* rd_create_error(void);
void rd_destroy(rd_handle* h);
const char* rd_last_error(rd_handle* h);

/* HOST pointer to a .safetensors byte image using the reference's tensor names (a leading "model." is ignored). */
int rd_load_weights(rd_handle* h, const void* safetensors_image, size_t nbytes);

/* bytes of device workspace one call with this geometry needs (H is ignored for rec: always 48) */
int rd_query_workspace(rd_handle* h, int B, int H, int W, int flags, size_t* ws_bytes);

/* Text detector ("ppocrv6_det", "ppocrv5_det_server", "ppocrv5_det_mobile" or "ppocrv3_det_mobile"): x [B,3,H,W] (H, W multiples of 32; the server detector: >= 64) -> DB probability
 * map [B,1,H,W] (the reference session's `maps`) */
int rd_det_forward(rd_handle* h, const float* x_nchw_dev, int B, int H, int W, float* prob_b1hw_dev, void* ws_dev,
                   size_t ws_bytes, void* stream);
/* The same forward with debug outputs.  flags 0: exactly rd_det_forward (aux_dev may be NULL).  RD_DET_WANT_NECK ("ppocrv5_det_server",
 * "ppocrv5_det_mobile" and "ppocrv3_det_mobile"): aux_dev also receives the neck's output `fuse` as NCHW [B,256,H/4,W/4] (server) or [B,96,H/4,W/4] (both mobile kinds).  rd_query_workspace takes the same flags. */
#define RD_DET_WANT_NECK 1
int rd_det_forward_ex(rd_handle* h, const float* x_nchw_dev, int B, int H, int W, float* prob_b1hw_dev, int flags, float* aux_dev,
                      void* ws_dev, size_t ws_bytes, void* stream);

/* PP-OCRv6 rec: x [B,3,48,W] (any W >= 16) -> per time step (T = rd_rec_seq_len(W): two stride-2 convs and the (3,2)
 * average pool, W/8 when W is a multiple of 8) argmax class and its softmax probability; full_btc_dev is only written with RD_REC_WANT_SOFTMAX / RD_REC_WANT_LOGITS (else may be NULL). */
int rd_rec_forward(rd_handle* h, const float* x_nchw_dev, int B, int W, int32_t* idx_bt_dev, float* prob_bt_dev,
                   float* full_btc_dev, int flags, void* ws_dev, size_t ws_bytes, void* stream);
int rd_rec_num_classes(rd_handle* h);
/* The backbone the loaded weights picked, for the two kinds that serve two: "ppocrv5_det_server" and "ppocrv5_rec_server" return
 * "pphgnetv2_b4" (the PP-OCRv5 server files) or "pphgnet_small" (the PP-OCRv4 server files, ch_PP-OCRv4_det_server / _rec_server, handed
 * over as a state dict: their tensors resolve to these kinds).  "" for every other kind and before rd_load_weights; never NULL. */
const char* rd_backbone_name(rd_handle* h);
/* The same network in two stages, for a pipeline that recognises the lines of many batches (rapid_ocr.py:430-449 loops over
 * `rec_batch_num` chunks and calls the session once per chunk): the neck and the CTC head of one chunk are ~25 launches on a few
 * thousand tokens - launch latency - so the chunks run only the backbone, each writing its tokens into ONE buffer, and the tail
 * runs once over all of them.  The results are those of rd_rec_forward chunk by chunk.
 *   rd_rec_backbone_forward: x [B,3,48,W] -> tokens [B][T = rd_rec_seq_len(W)][rd_rec_token_dim()] float32
 *   rd_rec_tail_forward:     tokens [n_tokens][dim] of n_lines text lines (any mix of lengths) -> idx / prob [n_tokens];
 *                            seg_dev = int32 [n_lines][2] (first token, tokens) per line, tokinfo_dev = int32 [n_tokens]
 *                            (position in its line | tokens of the line << 16), max_tokens = the longest line (< 32768)
 * rd_query_workspace(h, B, 0, W, RD_REC_STAGE_BACKBONE) resp. (h, n_lines, max_tokens, n_tokens, RD_REC_STAGE_TAIL) size them. */
#define RD_REC_STAGE_BACKBONE 8
#define RD_REC_STAGE_TAIL 16
int rd_rec_token_dim(rd_handle* h);
int rd_rec_backbone_forward(rd_handle* h, const float* x_nchw_dev, int B, int W, float* tokens_btd_dev, void* ws_dev, size_t ws_bytes,
                            void* stream);
int rd_rec_tail_forward(rd_handle* h, const float* tokens_dev, int n_tokens, int n_lines, int max_tokens, const int32_t* seg_dev,
                        const int32_t* tokinfo_dev, int32_t* idx_dev, float* prob_dev, void* ws_dev, size_t ws_bytes, void* stream);
/* The backbone stage over text lines of DIFFERENT reference padded widths in one launch.  The reference pads every line to the
 * width of its own chunk of `rec_batch_num` = 6 lines (rapid_ocr.py:404-449: imgW = int(48 * max w/h of the chunk)) and the
 * network's output for a line depends on that width (conv borders, SE pooling extent, LightSVTR attention over the padded columns),
 * so GPU-sized batches of mixed chunks must still give every line ITS width: x [B,3,48,W] holds line b in columns [0, w_b) (zeros
 * beyond), line_tab_dev = int32 [B][4] = (w_b, (w_b - 1) / 2 + 1, ((w_b - 1) / 2) / 2 + 1, first token of the line in tokens_dev);
 * line b writes rd_rec_seq_len(w_b) tokens there.  Results per line == rd_rec_backbone_forward on [1,3,48,w_b].
 * rd_query_workspace(h, B, 0, W, RD_REC_STAGE_BACKBONE | RD_REC_LINE_WIDTHS) sizes the workspace.
 * Served by "ppocrv6_rec", "ppocrv5_rec_mobile" and "ppocr_rec_mv1e"; "ppocrv5_rec_server" returns an error that says so. */
#define RD_REC_LINE_WIDTHS 32
int rd_rec_backbone_forward_lines(rd_handle* h, const float* x_nchw_dev, int B, int W, const int32_t* line_tab_dev, float* tokens_dev,
                                  void* ws_dev, size_t ws_bytes, void* stream);
/* number of CTC time steps the rec network emits for input width W (stride-2 stem x2, then avg-pool (3,2)) */
int rd_rec_seq_len(int W);

/* PPHGNetV2-B4 (PP-DocLayout backbone): x [B,3,H,W] -> 4 NCHW feature maps, strides 4/8/16/32,
 * channels 128/512/1024/2048. */
int rd_backbone_forward(rd_handle* h, const float* x_nchw_dev, int B, int H, int W, float* const feats_dev[4],
                        void* ws_dev, size_t ws_bytes, void* stream);

/* PP-FormulaNet_plus encoder (PPHGNetV2_B6_Formula): x [B,C,H,W], C = 1 (grey, replicated to 3 channels like
 * rapid_doc/model/formula/rapid_formula_self/networks/backbones/rec_pphgnetv2.py:1626-1628) or 3; H, W multiples of 32.
 * enc_dev: [B, (H/32)*(W/32), 2048] = `last_hidden_state` of the reference backbone (:1629-1633).
 * model_kind "pphgnetv2_b6_formula". */
int rd_formula_encoder_forward(rd_handle* h, const float* x_nchw_dev, int B, int C, int H, int W, float* enc_dev,
                               void* ws_dev, size_t ws_bytes, void* stream);

/* PP-FormulaNet_plus decoder head (model_kind "ppformulanet_head"; load the full model's .safetensors / state dict, only
 * `head.*` tensors are used): greedy decode with KV cache of all B formulas at once.  Replaces PPFormulaNet_Head.forward ->
 * generate_export (rapid_doc/model/formula/rapid_formula_self/networks/heads/rec_ppformulanet_head.py:1054-1176,1367-1380).
 * enc_dev [B,S,2048] = encoder states; ids_dev [B][max_new_tokens+1] int64 (start token 0 first, pad 1 after EOS 2);
 * *n_cols = number of leading columns the reference would return (it stops when every sequence has produced EOS). */
int rd_formula_decode(rd_handle* h, const float* enc_dev, int B, int S, int max_new_tokens, int64_t* ids_dev, int32_t* n_cols,
                      void* stream);
/* The same decode through refilled slots (model_kind "ppformulanet_head"): the N formulas of enc_dev [N,S,2048] run through `slots` decode
 * rows; a row whose formula ends (EOS, or max_new_tokens reached) takes the next waiting formula on the device, inside the captured step, so
 * no row waits for the longest formula of a batch.  Row i of ids_dev [N][max_new_tokens+1] is what rd_formula_decode writes for formula i
 * in a batch of `slots` formulas: start token 0, the tokens, EOS 2, pad 1 behind it; lens_dev[i] = the columns that count, EOS included
 * (max_new_tokens + 1 for a formula that reached the limit: it has no EOS).
 * Limits: 1 <= slots <= RD_FORMULA_STREAM_MAX_SLOTS (the decode rows of the fused step kernels), N >= 1, and
 * N * S <= RD_FORMULA_STREAM_MAX_TOKENS: every encoder token keeps its projection and its cross-attention K | V of every layer on the
 * device for the whole call, 6 layers x 2 x 512 x 4 B + 512 x 4 B = 26 KiB per token, 1.6 GiB at the limit.  Outside the limits the call
 * returns non-zero with a message in rd_last_error, launches nothing and leaves the outputs untouched.
 * stats (host, may be NULL) is filled before the call returns; the call synchronises `stream`. */
#define RD_FORMULA_STREAM_MAX_SLOTS 32
#define RD_FORMULA_STREAM_MAX_TOKENS 65536
typedef struct rd_formula_stream_stats {
    int32_t steps;           /* step launches, the host loop's run-ahead included (it looks at the device state every 8 steps) */
    int32_t live_slot_steps; /* slot-steps that produced a token = sum over the formulas of lens - 1 */
    int32_t slots;
    int32_t admitted;        /* formulas that were given a slot (= N) */
} rd_formula_stream_stats;
int rd_formula_decode_stream(rd_handle* h, const float* enc_dev, int N, int S, int max_new_tokens, int slots, int64_t* ids_dev,
                             int32_t* lens_dev, rd_formula_stream_stats* stats, void* stream);
/* largest max_new_tokens the loaded positional table supports (2560 for the shipped PP-FormulaNet_plus-M) */
int rd_formula_max_new_tokens(rd_handle* h);

/* u8 HWC (3 channels) device image -> resize to OHxOW -> (v*scale - mean[c]) / std[c] -> CHW float32.
 * interp: 1 = cv2.INTER_LINEAR, 2 = cv2.INTER_CUBIC, both in OpenCV's 8-bit fixed-point arithmetic (11-bit coefficients,
 * uint8 result) - bit-equal to oracle/cv2_ops.py; against cv2 itself parity is unpinned (package absent at build time). */
int rd_preproc_resize_norm(int device_id, const uint8_t* hwc_u8_dev, int H, int W, int OH, int OW, const float mean[3],
                           const float std[3], float scale, int interp, int swap_rb, float* out_chw_dev, void* stream);

/* The same for P images of one size in ONE launch: pages_u8_dev [P][H][W][3] -> out [P][3][OH][OW] (the reference's per-page
 * loop over PPPreProcess / DetPreProcess, rapid_layout_self/main.py:41-56, rapid_ocr.py:474-536). */
int rd_preproc_resize_norm_batch(int device_id, const uint8_t* pages_u8_dev, int P, int H, int W, int OH, int OW, const float mean[3],
                                 const float std[3], float scale, int interp, int swap_rb, float* out_nchw_dev, void* stream);

/* rd_preproc_resize_norm for n source images of ANY sizes, each to its own output size, in ONE launch (the pages of a batch whose sizes
 * differ: the reference slices the pages of many documents into one batch, pipeline_analyze.py:135,197-201).  Source k: u8 [H][W][3] at
 * `src`, ANY byte address, rows `pitch` >= 3 * W bytes apart (a window of a larger image); its [3][OH][OW] float32 planes are written to
 * out_dev + out_off - bit for bit what rd_preproc_resize_norm writes for a contiguous copy of the source with the same mean, std, scale,
 * interp and swap_rb (which all sources of a call share).  No byte outside [src + y * pitch, src + y * pitch + 3 * W) of a row y < H is
 * read, nothing outside the slots is written.  descs_host and descs_dev hold the same n descriptors on the host and on the device
 * (uploaded on `stream` by the caller): the checks read the host copy, so nothing is read back and the stream is not synchronised.
 * Return 0 = ok, 1 = bad arguments - a NULL array or NULL out_dev, n outside 1 .. 65535, a NULL src, pitch < 3 * W, a side outside
 * 1 .. 32768, interp other than 1 / 2, a negative out_off, a slot that overruns out_floats, two slots that overlap: nothing launched,
 * the message is rd_create_error()'s. */
typedef struct rd_resize_source_desc {
    const uint8_t* src;       /* device address of pixel (0, 0), 3-channel uint8 HWC, any byte alignment */
    int64_t pitch;            /* bytes between rows, >= 3 * W */
    int64_t out_off;          /* offset in floats of this source's [3][OH][OW] planes inside out_dev */
    int32_t W, H, OW, OH;
    int32_t reserved[2];      /* 0 */
} rd_resize_source_desc;
int rd_preproc_resize_norm_sources(int device_id, const rd_resize_source_desc* descs_host, const rd_resize_source_desc* descs_dev, int n,
                                   const float mean[3], const float std[3], float scale, int interp, int swap_rb, float* out_dev,
                                   int64_t out_floats, void* stream);

/* u8 HWC (3 channels) device image -> Pillow's antialiased bilinear resample to OHxOW -> ((v / 255) - mean[c]) / std[c] -> CHW float32:
 * transforms.Resize((OH, OW)) on a PIL image, ToTensor and Normalize, as UniTable's TablePreprocess runs them
 * (rapid_table_self/table_structure/unitable/pre_process.py).  The resample is Pillow's 8-bit path bit for bit (Resample.c): per axis
 * scale = in / out, support = max(scale, 1), triangle weights normalised in double and rounded to 22-bit fixed point (computed on the
 * host, cached per (in, out), uploaded on `stream`), the horizontal pass first into a uint8 intermediate the library owns, then the
 * vertical pass; a pass whose in == out does not run.  The normalisation is fp32 in that operation order with IEEE division.
 * swap_rb = 1 reads the source as BGR (cv2.cvtColor(BGR2RGB) in front).  out_u8_hwc_dev (may be NULL): the resampled bytes [OH][OW][3].
 * Bound: 1 <= H, W, OH, OW <= RD_RESIZE_AA_MAX_SIDE (any ratio between them: the tap count 2 ceil(max(in / out, 1)) + 1 is a loop bound,
 * not a tile).  A size outside it, or a NULL image pointer, returns non-zero WITHOUT a launch; the message is in rd_create_error() (the
 * calling thread's handle-less error string).  The first call with a new (in, out) pair or a larger intermediate allocates device
 * memory (not capturable into a hipGraph); calls on one stream are ordered, calls on different streams use different intermediates. */
#define RD_RESIZE_AA_MAX_SIDE 16384
int rd_preproc_resize_aa_norm(int device_id, const uint8_t* hwc_u8_dev, int H, int W, int OH, int OW, const float mean[3],
                              const float std[3], int swap_rb, float* out_chw_dev, uint8_t* out_u8_hwc_dev, void* stream);

/* The formula pre-process of PP-FormulaNet_plus on the device, bit for bit as the reference runs it with Pillow
 * (pp_formulanet_plus/pre_process.py:39-246: margin crop, Image.resize(BILINEAR) to a short side of 384, Image.thumbnail((384, 384)) =
 * reduce + BICUBIC over a float32 box, centre pad with 0, (v / 255 - 0.7931) / 0.1738, grey = .114 c0 + .587 c1 + .299 c2).  Three calls:
 *   1. rd_formula_margin_boxes: one launch for n crops.  descs_dev: n device-resident crop descriptors, each a 3-channel uint8 HWC view
 *      (any base, any row pitch: a window of a page); boxes_dev int32 [n][4] = (x0, y0, x1, y1) of the pixels whose normalised grey
 *      (L - min) * 255 < 200 * (max - min), L = Pillow's convert("L"); the whole crop when it is uniform.
 *   2. the caller copies the boxes to the host (the ONE device-to-host copy of a batch: every later size follows from the box) and may
 *      ask rd_formula_preproc_plan, host only, what follows from a box of w x h pixels.  served = 0: a side of a stage lies outside
 *      1 .. RD_RESIZE_AA_MAX_SIDE and the crop has to take the host path.
 *   3. rd_formula_preproc_batch: descs_host / boxes_host are the same n descriptors and their boxes in HOST memory; out_dev float32
 *      [n][384][384] (= [n, 1, 384, 384]); out_u8_dev (may be NULL) uint8 [n][384][384][3], the padded image in front of the normalisation.
 *      Enqueues everything on `stream` and returns; a crop's bits do not depend on the batch it rides in (crops are processed one after
 *      the other).  The workspace is the library's, per (device, stream) and grown on demand, as that of rd_preproc_resize_aa_norm
 *      (no caller-given workspace, no size query): intermediates, and the batch's coefficient tables, which are computed on the host and
 *      uploaded with one asynchronous copy from a pinned staging buffer.  A first call with larger crops allocates (not capturable
 *      into a hipGraph); calls on one stream are ordered, calls on different streams use different workspaces.
 * Bad arguments (NULL, n < 1, a box outside its crop, a crop whose plan is not served) return non-zero WITHOUT a launch; the message is
 * in rd_create_error(). */
#define RD_RESAMPLE_BILINEAR 2 /* Pillow's Image.BILINEAR / Image.BICUBIC */
#define RD_RESAMPLE_BICUBIC 3
#define RD_FORMULA_SIDE 384
typedef struct rd_formula_crop {
    const uint8_t* base; /* device address of pixel (0, 0), channel 0 */
    int64_t pitch;       /* bytes from one row to the next */
    int32_t w, h;
} rd_formula_crop;
typedef struct rd_formula_plan {
    int32_t served;           /* 1: every stage fits the device bound */
    int32_t resize_w, resize_h; /* Image.resize(BILINEAR) target: short side 384, long side int(384 * long / short) */
    int32_t thumb;            /* 1: thumbnail resamples (a side above 384) */
    int32_t final_w, final_h; /* size in front of the pad */
    int32_t fx, fy;           /* reduce factors (1, 1: reduce does not run) */
    int32_t reduced_w, reduced_h;
    float box_w, box_h;       /* the bicubic resample's box (0, 0, box_w, box_h), float32 as Pillow's C side takes it */
    int32_t pad_x, pad_y;     /* paste offsets: (384 - final) / 2, floored */
} rd_formula_plan;
int rd_formula_margin_boxes(int device_id, const rd_formula_crop* descs_dev, int n, int32_t* boxes_dev, void* stream);
int rd_formula_preproc_plan(int w, int h, rd_formula_plan* plan);
int rd_formula_preproc_batch(int device_id, const rd_formula_crop* descs_host, const int32_t* boxes_host, int n, float* out_dev,
                             uint8_t* out_u8_dev, void* stream);

/* Text-line crops for one rec batch (replaces per-line cv2.warpPerspective + rapidocr resize_norm_img:
 * rapid_doc/utils/ocr_utils.py:494-536, rapid_doc/model/ocr/rapid_ocr.py:436-440).  pages_u8_dev: [P][H][W][3];
 * descs_dev: n device-resident rd_crop_desc; out: [n][3][out_h][out_w_padded] float32, zero right-padded. */
typedef struct rd_crop_desc {
    int32_t page;          /* page index in the batch */
    int32_t out_w;         /* resized width of this line (<= out_w_padded) */
    float crop_w, crop_h;  /* size of the rectified crop in page pixels */
    float m[9];            /* crop (x, y, 1) -> page (x, y, w) homography, row-major */
    int32_t rot90;         /* rotate the crop 90 deg CCW first (tall boxes) */
    int32_t pad_;
} rd_crop_desc;
int rd_crop_resize_norm_batch(int device_id, const uint8_t* pages_u8_dev, int P, int H, int W,
                              const rd_crop_desc* descs_dev, int n, int out_h, int out_w_padded, const float mean[3],
                              const float std[3], float scale, int swap_rb, float* out_nchw_dev, void* stream);

/* Reference-shaped text-line crops for one rec batch, in OpenCV's 8-bit arithmetic: cv2.warpPerspective(INTER_CUBIC,
 * BORDER_REPLICATE) of every line to its integer-sized uint8 crop (rapid_doc/utils/ocr_utils.py:494-536), np.rot90 for tall
 * crops, then rapidocr's resize_norm_img (linear resize to height out_h, /255, (x - 0.5) / 0.5, zero right-padding; called
 * from rapid_doc/model/ocr/rapid_ocr.py:436-440).  scratch_u8_dev: device buffer holding the packed uint8 crops
 * (desc.scratch_off, crop_w * crop_h * 3 bytes each); max_crop_pixels: largest crop_w * crop_h among the n lines.
 * out: [n][3][out_h][out_w_padded] float32.  swap_rb = 1 when the pages are RGB (rapidocr works on BGR). */
typedef struct rd_line_crop_desc {
    int32_t page;          /* page index in the batch */
    int32_t out_w;         /* resized width of this line (<= out_w_padded) */
    int32_t crop_w, crop_h;/* rectified crop size in page pixels (before the optional rotation) */
    int32_t rot90;         /* rotate the crop 90 deg CCW first (tall boxes) */
    int32_t scratch_off;   /* byte offset of this crop in scratch_u8_dev */
    double m[9];           /* crop (x, y, 1) -> page (X, Y, W) homography, row-major, float64 like cv2's */
} rd_line_crop_desc;
int rd_line_crops_batch(int device_id, const uint8_t* pages_u8_dev, int P, int H, int W, const rd_line_crop_desc* descs_dev,
                        int n, int64_t max_crop_pixels, uint8_t* scratch_u8_dev, int out_h, int out_w_padded, int swap_rb,
                        float* out_nchw_dev, void* stream);

/* The two stages of rd_line_crops_batch as separate calls, for callers whose text lines come from SEVERAL source images of
 * different sizes but are recognised together (the reference pools every line of a page batch per language before it sorts
 * and chunks them, rapid_doc/backend/pipeline/analyze_utils.py:216-252): rd_line_warp_batch once per source image array
 * (stage 1: cubic warp of its lines into the shared scratch buffer), then rd_line_resize_norm_batch once per rec batch
 * (stage 2: rot90 / linear resize to out_h / normalise / zero right-pad; reads the scratch buffer only). */
int rd_line_warp_batch(int device_id, const uint8_t* pages_u8_dev, int P, int H, int W, const rd_line_crop_desc* descs_dev, int n,
                       int64_t max_crop_pixels, uint8_t* scratch_u8_dev, void* stream);
int rd_line_resize_norm_batch(int device_id, const rd_line_crop_desc* descs_dev, int n, const uint8_t* scratch_u8_dev, int out_h,
                              int out_w_padded, int swap_rb, float* out_nchw_dev, void* stream);

/* rd_line_warp_batch for lines that come from MANY source images of different sizes (the region images behind RapidDoc's OCR-model
 * seam, rapiddoc_amd/ocr_model.py: every text region is an image of its own): each line names its source, so ONE launch warps all lines
 * of a rec launch.  Line k: the crop_w x crop_h crop whose pixel (x, y, 1) maps to source position m * (x, y, 1) is written, packed
 * [crop_h][crop_w][3], to scratch_u8_dev + scratch_off - the arithmetic of rd_line_warp_batch (1/32-pixel positions, the 15-bit cubic
 * weight table, border replicate), byte for byte.  The source is u8 [H][W][3] at `src`, ANY byte address, rows `pitch` >= 3 * W bytes
 * apart (a window of a larger image).  No byte outside [src + y * pitch, src + y * pitch + 3 * W) of a row y < H is read, nothing outside
 * the crops is written.  descs_host and descs_dev hold the same n descriptors on the host and on the device (uploaded on `stream` by the
 * caller): the checks read the host copy, so nothing is read back and the stream is not synchronised.  Return 0 = ok, 1 = bad arguments -
 * a NULL array or scratch, n outside 1 .. 65535, a NULL src, pitch < 3 * W, a source or crop size that is not positive, a negative
 * scratch_off, a crop that overruns scratch_bytes: nothing launched, the message is rd_create_error()'s. */
typedef struct rd_line_source_desc {
    const uint8_t* src;       /* device address of the source's pixel (0,0), channel 0 */
    int64_t pitch;            /* bytes per source row */
    int32_t W, H;             /* source size */
    int32_t crop_w, crop_h;   /* rectified crop size */
    int32_t scratch_off;      /* byte offset of this crop in scratch_u8_dev */
    int32_t reserved;         /* 0 */
    double m[9];              /* crop (x, y, 1) -> source (X, Y, W) homography, row-major, float64 like cv2's */
} rd_line_source_desc;
int rd_line_warp_sources(int device_id, const rd_line_source_desc* descs_host, const rd_line_source_desc* descs_dev, int n,
                         uint8_t* scratch_u8_dev, int64_t scratch_bytes, void* stream);

/* Text-line direction classifier ("ppocr_cls_mobile"): x [B,3,H,W] (rapidocr's classifier pre-process gives 48 x 192) -> the head's softmax
 * [B,2] = (P(0 deg), P(180 deg)), the tensor the reference session returns for this graph.  flags 0, or RD_CLS_WANT_AUX: aux_dev also
 * receives per line [2 logits | 200 pooled features] (B x 202 floats).  An H, W that leaves an empty map in front of the 2 x 2 max-pool
 * (H < 33 or W < 3) fails, and rd_last_error says so.  rd_query_workspace takes the same B, H, W, flags. */
#define RD_CLS_WANT_AUX 1
int rd_cls_forward(rd_handle* h, const float* x_nchw_dev, int B, int H, int W, float* prob_b2_dev, int flags, float* aux_dev, void* ws_dev,
                   size_t ws_bytes, void* stream);
/* Table-structure encoder ("unitable_encoder": UniTable's ViT-B - 16 x 16 patches, learned positions, 12 pre-norm encoder layers of d = 768,
 * 12 heads of 64, FFN 3072, final LayerNorm): x [B,3,H,W], already normalised (H, W multiples of 16, (H / 16) (W / 16) <= 1024 patches; the
 * product shape is 448 x 448, T = 784) -> memory [B,T,768], the tensor the reference's decoder attends over.  A shape outside those
 * limits fails, and rd_last_error says so.  rd_query_workspace takes the same B, H, W with flags 0. */
int rd_table_encoder_forward(rd_handle* h, const float* x_nchw_dev, int B, int H, int W, float* memory_bt768_dev, void* ws_dev, size_t ws_bytes,
                             void* stream);
/* Table-structure decoder ("unitable_decoder": UniTable's GPTFastDecoder - 4 pre-norm blocks of d = 768 with a 1024-row KV cache and
 * cross-attention over `memory`, generator 768 -> 960) with the reference's greedy loop, for B <= 8 tables at once (a larger B fails with a
 * message); every table gets exactly the ids it gets alone.  memory [B,S,768] as rd_table_encoder_forward wrote it.  Per step the next token
 * is the argmax over the module's whitelist (ids 1 and 12 .. 509); a token inside [bbox_first_id, bbox_last_id] raises the table's counter,
 * and when the counter exceeds 4 the token is replaced by bbox_close_id and the counter returns to 0 (no other token resets it).  The ids
 * come from the vocabulary file, so they are the caller's.  ids_dev int64 [B][max_new_tokens + 1]: column 0 = prefix_id, then the emitted
 * tokens; a table that emitted eos_id keeps its slot and writes pad_id behind it.  n_tokens (HOST int32 [B], may be NULL): tokens of
 * every table with the prefix and the EOS (max_new_tokens + 1 where it never stopped).  1 <= max_new_tokens <= 1024.  Synchronises the stream. */
typedef struct {
    int32_t prefix_id, eos_id, pad_id, bbox_close_id, bbox_first_id, bbox_last_id;
} rd_table_decode_cfg;
int rd_table_decode(rd_handle* h, const float* memory_dev, int B, int S, int max_new_tokens, const rd_table_decode_cfg* cfg, int64_t* ids_dev,
                    int32_t* n_tokens, void* stream);
/* The same decode through refilled slots (model_kind "unitable_decoder"): the N tables of memory_dev [N,S,768] run through `slots` decode
 * rows; a row whose table ends (eos_id, or max_new_tokens reached) takes the next waiting table on the device, inside the captured step -
 * at position 0 and with the bbox counter at 0 -, so no row waits for the longest table of a batch.  Row i of ids_dev
 * [N][max_new_tokens + 1] is exactly what rd_table_decode writes for table i alone: prefix_id, the emitted tokens, eos_id, pad_id behind
 * it; lens_dev[i] (DEVICE int32 [N]) = the columns that count, prefix and EOS included (max_new_tokens + 1 for a table that never stopped).
 * Limits: 1 <= slots <= RD_TABLE_STREAM_MAX_SLOTS (the rows of the decoder's weight-streaming GEMV), N >= 1, 1 <= S <= 1024,
 * 1 <= max_new_tokens <= 1024, the id checks of rd_table_decode, and N * S <= RD_TABLE_STREAM_MAX_TOKENS: every memory row keeps its
 * cross-attention K and V of the 4 layers on the device for the whole call, 4 x 2 x 768 x 4 B = 24 KiB per row, 1.5 GiB at the limit.
 * Outside the limits the call returns non-zero with a message in rd_last_error that names the limit, launches nothing and leaves the
 * outputs untouched.  stats (host, may be NULL) is filled before the call returns; the call synchronises `stream`. */
#define RD_TABLE_STREAM_MAX_SLOTS 8
#define RD_TABLE_STREAM_MAX_TOKENS 65536
typedef struct rd_table_stream_stats {
    int32_t steps;           /* step launches, the host loop's run-ahead included (it looks at the device state every 8 steps) */
    int32_t live_slot_steps; /* slot-steps that produced a token = sum over the tables of lens - 1 */
    int32_t slots;
    int32_t admitted;        /* tables that were given a slot (= N) */
} rd_table_stream_stats;
int rd_table_decode_stream(rd_handle* h, const float* memory_dev, int N, int S, int max_new_tokens, int slots, const rd_table_decode_cfg* cfg,
                           int64_t* ids_dev, int32_t* lens_dev, rd_table_stream_stats* stats, void* stream);
/* The classifier's verdict applied on the device, between rd_line_warp_batch and rd_line_resize_norm_batch: every line with
 * prob[1] > prob[0] and prob[1] >= thresh has its packed uint8 crop in scratch_u8_dev turned by 180 degrees in place
 * (cv2.rotate(ROTATE_180): the pixel order reversed); flipped_out_dev[i] = 1 for those lines, 0 for the others.  The scratch holds the
 * crop BEFORE the optional rot90; two rotations commute, so this equals turning the crop the classifier saw. */
int rd_line_flip180_batch(int device_id, const rd_line_crop_desc* descs_dev, int n, const float* cls_prob_n2_dev, float thresh,
                          uint8_t* scratch_u8_dev, int32_t* flipped_out_dev, void* stream);

/* CTC greedy decode on the device (replaces rapidocr CTCLabelDecode's per-line loop, called from
 * rapid_doc/model/ocr/rapid_ocr.py:444-449): idx / prob [B][T] as rd_rec_forward wrote them -> per line, at out + b * row_bytes:
 * int32 n_text_bytes, float32 confidence (the float32 np.mean of the kept max-probabilities, bit for bit), int32 n_kept,
 * int32 0, then the UTF-8 text.  char_table_dev: [n_classes][1 + max_len] bytes = (length, UTF-8 bytes) of every dictionary
 * entry, entry 0 = blank.  row_bytes >= 16 + T * max_len. */
int rd_ctc_collapse(int device_id, const int32_t* idx_bt_dev, const float* prob_bt_dev, int B, int T, const uint8_t* char_table_dev,
                    int max_len, int n_classes, uint8_t* out_dev, int row_bytes, void* stream);
/* The same over RAGGED lines as rd_rec_tail_forward leaves them: line b = seg_dev[2 b + 1] tokens (<= max_tokens <= 65535) starting at
 * token seg_dev[2 b] of idx_dev / prob_dev.  kept_cols_dev / kept_conf_dev (each may be NULL): uint16 / float32 [n_lines][max_tokens],
 * the time step and the probability of every kept character in order (n_kept of them, header field 2) - the `selection` and the
 * `conf_list` rapidocr's CTCLabelDecode hands to get_word_info / WordInfo when return_word_box is set (RapidDoc's patched
 * get_word_info and cal_ocr_word_box: rapid_doc/model/ocr/ocr_patch.py:264-389; table OCR default, analyze_utils.py:308). */
int rd_ctc_collapse_lines(int device_id, const int32_t* idx_dev, const float* prob_dev, int n_lines, const int32_t* seg_dev, int max_tokens,
                          const uint8_t* char_table_dev, int max_len, int n_classes, uint8_t* out_dev, int row_bytes, uint16_t* kept_cols_dev,
                          float* kept_conf_dev, void* stream);
/* Host: n rows of rd_ctc_collapse / rd_ctc_collapse_lines (HOST memory, row_bytes apart) -> text_out = the lines' UTF-8 texts back to
 * back (line b = bytes byte_off_out[b] .. byte_off_out[b + 1], byte_off_out has n + 1 entries), n_chars_out[b] = its number of code
 * points, conf_out[b] = the confidence as double, conf3_out[b] = float(f"{conf:.3f}") of it (analyze_utils.py:280).  text_cap =
 * capacity of text_out in bytes (n * (row_bytes - 16) always suffices).  Returns 0, 1 = bad arguments / a corrupt row, 2 = capacity. */
int rd_ctc_rows_text(const uint8_t* rows_host, int n, int row_bytes, uint8_t* text_out, int64_t text_cap, int64_t* byte_off_out,
                     int32_t* n_chars_out, double* conf_out, double* conf3_out);

/* DB post-process (HOST pointers, runs on the host like the reference's): probability maps [B][H][W] -> text boxes.
 * Replaces rapidocr DBPostProcess.__call__ as patched in rapid_doc/model/ocr/ocr_patch.py:223-241 (box_type "quad",
 * score_mode "fast"), called from rapid_doc/model/ocr/rapid_ocr.py:537-538.  src_hw[b] = (height, width) of the image
 * the boxes are scaled to.  out[b*max_out + i], i < n_out[b]: corners tl,tr,br,bl in source pixels + score. */
typedef struct rd_text_box {
    float pts[8];
    float score;
} rd_text_box;
int rd_db_postprocess(const float* prob_host, int B, int H, int W, const int32_t* src_hw, float thresh, float box_thresh,
                      float unclip_ratio, int use_dilation, int max_candidates, rd_text_box* out, int max_out,
                      int32_t* n_out, int n_threads);

/* The same post-process with NOTHING on the host (round 3): rows -> runs in raster order -> regions (union-find over
 * row-adjacent runs) -> convex hull of each region's row extremes -> min-area rectangle -> box_score_fast -> unclip / rescale /
 * filter_det_res, all on `stream`; the caller needs one device-to-host copy of n_out_dev and out_dev.  Boxes and their order
 * equal rd_db_postprocess's.  src_hw_dev: int32 [B][2] on the device.  n_out_dev: int32 [B + 1]; entry B is an overflow flag
 * (a page had more than max_runs bitmap runs: repeat that batch with rd_db_postprocess).  ws_dev: rd_db_boxes_workspace()
 * bytes of device scratch.  The scores are sums in double precision reduced in a fixed tree order; the host path adds the same
 * terms serially, so a candidate whose score sits within one ulp of box_thresh may be kept on one path and dropped on the other. */
size_t rd_db_boxes_workspace(int B, int H, int W, int max_runs, int max_candidates);
int rd_db_boxes_device(int device_id, const float* prob_dev, int B, int H, int W, const int32_t* src_hw_dev, float thresh, float box_thresh,
                       float unclip_ratio, int use_dilation, int max_candidates, int max_runs, void* ws_dev, size_t ws_bytes,
                       rd_text_box* out_dev, int max_out, int32_t* n_out_dev, void* stream);

/* Host: what follows the DB post-process for a whole page batch (rapid_doc/utils/ocr_utils.py:105-127 sorted_boxes, then
 * merge_det_boxes :16-67,130-317).  boxes: [B][max_in] records as rd_db_postprocess / rd_db_boxes_device leave them (HOST memory; the
 * first counts[b] of page b are read, the scores are not).  Coordinates are truncated toward zero to integers; reading order = stable
 * sort by (y, x) of the first corner + adjacent swaps inside a row (top-left y closer than 10); merge = axis-aligned boxes sorted by
 * top y, grouped into lines by y-overlap > 0.6 with the box before, lines wider than 4 x their height fused where their x intervals
 * touch, tilted boxes (diagonal extent outside 0.8 .. 1.2 of the mean side height) appended unchanged.  float32 arithmetic, bit for bit
 * what rapiddoc_amd.ocr_host.merge_det_boxes(sorted_boxes(.)) returns.  quads_out: float32 [B][max_in][4][2], n_out: int32 [B]. */
int rd_text_boxes_order_merge(const rd_text_box* boxes, const int32_t* counts, int B, int max_in, float* quads_out, int32_t* n_out);

/* PP-DocLayout post-process, rectangle mode (HOST pointers).  Replaces PPPostProcess.__call__ with
 * layout_shape_mode="rect": rapid_doc/model/layout/rapid_layout_self/model_handler/pp_doclayout/post_process.py:20-243.
 * boxes: [n][ncol] float32 rows (cls, score, x0, y0, x1, y1[, order...]) in original-image pixels (ncol 6, 7 or 8).
 * out: [n][6] kept rows, out_order[i] = the reference's 1-based "order" field, *n_out = kept count. */
typedef struct rd_layout_post_cfg {
    int32_t n_classes;
    int32_t image_index, formula_index; /* index of the "image" / "formula" label, -1 if absent          */
    int32_t thresh_is_dict;             /* 0: thresh[0] for every class; 1: thresh[class] (0.5 if missing) */
    const float* thresh;
    int32_t layout_nms;
    int32_t merge_kind;                 /* 0 none/"union", 1 "large", 2 "small", 3 per-class table         */
    const int8_t* merge_per_class;      /* [n_classes]: 0 union, 1 large, 2 small (merge_kind 3)            */
    int32_t unclip_kind;                /* 0 none, 1 one (w, h) ratio pair, 2 per-class pairs               */
    const float* unclip;                /* [2] or [n_classes][2]                                           */
    const uint8_t* unclip_present;      /* [n_classes] (unclip_kind 2)                                     */
} rd_layout_post_cfg;
int rd_layout_postprocess(const float* boxes, int n, int ncol, int img_w, int img_h, const rd_layout_post_cfg* cfg,
                          float* out, int32_t* out_order, int32_t* n_out);
/* The rows of `boxes` that reach the polygon stage of PPPostProcess.__call__ (post_process.py:213-218: after threshold / NMS /
 * big-image filter / containment merge / reading-order sort, before unclip and clip): sel_boxes [n][6], sel_src[i] = row index in
 * `boxes` (the detector's masks follow the boxes through those steps, :46-211).  Position i is out_order[k] - 1 of the row
 * rd_layout_postprocess writes for the same box. */
int rd_layout_postprocess_select(const float* boxes, int n, int ncol, int img_w, int img_h, const rd_layout_post_cfg* cfg,
                                 float* sel_boxes, int32_t* sel_src, int32_t* n_sel);

/* RT-DETR-family head operators - PREPARATION ONLY, PARITY UNPINNED (rapiddoc_amd/csrc/kernels_rtdetr.hip).  PP-DocLayout's neck / decoder
 * are ONNX files that are not part of the offline reference tree (rapid_layout_self/inference_engine/onnxruntime/main.py:61-78 only loads
 * them), so the graph cannot be read: these three entries implement operators whose definition does not depend on it, are tested against
 * fp64 restatements of their published definitions (tests/test_gpu_rtdetr_ops.py), and are wired into nothing.  Device pointers.
 *   rd_msdeform_attn   multi-scale deformable attention sampling (Deformable DETR eq. 3): value [B][S][H][D], shapes int32 [L][2] = (h, w),
 *                      level_start int32 [L], loc [B][Q][H][L][P][2] = (x, y) in [0, 1], attn [B][Q][H][L][P] -> out [B][Q][H * D];
 *                      bilinear samples as grid_sample(align_corners = False, zero padding); H * D <= 1024
 *   rd_topk_rows       per row of n scores: the k <= 1024 largest, descending, equal values in ascending index order, NaN above +inf
 *                      (the (queries x classes) selection in front of PPPostProcess, pp_doclayout/main.py:88-139)
 *   rd_encoder_layer   one post-norm transformer encoder layer (AIFI): MHA(q = k = x + pos, v = x) + residual + LayerNorm, FFN + residual +
 *                      LayerNorm over B sequences of T tokens; in_w [3 Dm][Dm] packed q | k | v; head_dim 16 or 32; `act` = rd activation
 *                      code (2 = GELU, 1 = ReLU); workspace of rd_encoder_layer_workspace(B * T, Dm, F) bytes */
int rd_msdeform_attn(int device_id, const float* value, const int32_t* shapes, const int32_t* level_start, const float* loc, const float* attn,
                     float* out, int B, int S, int H, int D, int Q, int L, int P, void* stream);
int rd_topk_rows(int device_id, const float* scores, int rows, int n, int k, float* out_vals, int32_t* out_idx, void* stream);
size_t rd_encoder_layer_workspace(int M, int Dm, int F);
int rd_encoder_layer(int device_id, const float* x, const float* pos, int B, int T, int Dm, int heads, int F, int act, const float* in_w,
                     const float* in_b, const float* out_w, const float* out_b, const float* ln1_g, const float* ln1_b, const float* w1,
                     const float* b1, const float* w2, const float* b2, const float* ln2_g, const float* ln2_b, float eps, float* out, void* ws,
                     size_t ws_bytes, void* stream);

/* Raster / polygon primitives of the polygon branch (HOST pointers; rapiddoc_amd/csrc/polygon_ops.cpp).  Each replaces one
 * OpenCV / shapely call of the reference (PARITY UNPINNED: neither library is available offline; restated from their published
 * algorithms):
 *   rd_find_external_contours  cv2.findContours(mask, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)        post_process.py:409
 *   rd_contour_area            cv2.contourArea                                                     :414
 *   rd_arc_length              cv2.arcLength(cnt, closed)                                          :415
 *   rd_approx_poly_dp          cv2.approxPolyDP(cnt, epsilon, closed)                              :416
 *   rd_min_area_rect_points    cv2.boxPoints(cv2.minAreaRect(points))  (corner order unspecified)  :553-554
 *   rd_polygon_area / rd_polygon_intersection_area   shapely Polygon.area / intersection(...).area :704-711
 *   rd_fill_poly               cv2.fillPoly(mask, [polygon], value), u8 single channel    rapid_doc/utils/model_utils.py:114
 * Points are [n][2] (x, y).  Return 0 = ok, 1 = bad arguments, 2 = output capacity (the needed counts are written). */
int rd_find_external_contours(const uint8_t* mask, int h, int w, int32_t* pts_out, int max_pts, int32_t* counts_out, int max_contours,
                              int32_t* n_contours, int32_t* n_pts);
double rd_contour_area(const int32_t* pts, int n);
double rd_arc_length(const int32_t* pts, int n, int closed);
int rd_approx_poly_dp(const int32_t* pts, int n, double epsilon, int closed, int32_t* out, int32_t* n_out);
int rd_min_area_rect_points(const float* pts, int n, float* out8);
double rd_polygon_area(const double* a, int na);
double rd_polygon_intersection_area(const double* a, int na, const double* b, int nb);
int rd_fill_poly(uint8_t* img, int h, int w, const int32_t* pts, int n, int value);

/* cv2.findContours(mask, RETR_EXTERNAL, CHAIN_APPROX_NONE): the same components in the same order as rd_find_external_contours, every
 * border-following point written (a pixel the walk passes twice appears twice).  Same arguments and return values. */
int rd_find_external_contours_none(const uint8_t* mask, int h, int w, int32_t* pts_out, int max_pts, int32_t* counts_out, int max_contours,
                                   int32_t* n_contours, int32_t* n_pts);

/* Checkbox detection, rapid_doc/utils/checkbox_det_cls.py checkbox_predict (called at batch_analyze.py:207-219), on the device
 * (csrc/kernels_checkbox.hip, csrc/checkbox_host.cpp; docs/notebook/checkbox.md).  OpenCV is restated from its published algorithms,
 * PARITY UNPINNED as for the polygon primitives above; tests/checkbox_reference.py is the yardstick.
 *   1. rd_checkbox_workspace: bytes of device scratch for a batch, 0 on bad arguments.  offsets (may be NULL) receives the byte offset of
 *      every part, in this order: threshold bits, line mask, dilated line mask (each [P][H][ceil(W / 64)] 64-bit words, bit i of word j =
 *      pixel 64 j + i), row counts [P][H], row offsets [P][H + 1], runs [P][max_runs] of int16 (y, x0, x1, 0), then six int32
 *      [P][max_runs] arrays: parent (a run whose parent is itself is a component's root), and at the roots block key, min x, max x,
 *      min y, max y; last the staged candidates.
 *   2. rd_checkbox_detect_device: every kernel of the stage on `stream`, nothing copied.  pages_dev: [P][H][W][3] u8, `bgr` non-zero
 *      when the channel order is B, G, R.  hdr_dev [P] and cands_dev [P * max_cand] are DEVICE memory.  The caller then copies hdr_dev
 *      (32 bytes a page) and, knowing the counts, the first sum(min(n_cand, max_cand)) records of cands_dev (584 bytes a candidate):
 *      two device-to-host copies per batch, neither proportional to the page area.  A page's records start at its cand_off.  A page
 *      whose flags are non-zero holds no usable records: repeat it with max_runs = H * ceil(W / 2) (RD_CHECKBOX_RUNS_OVERFLOW) or
 *      max_cand = its n_cand (RD_CHECKBOX_CANDS_OVERFLOW).
 *   3. rd_checkbox_finish (HOST pointers, one page): re-checks every record against the size filter and the ROI rectangle in double,
 *      orders the records by label order (`key`), applies the contour rule to the ROI and classifies by the tick count.  out [max_out].
 * Return 0 = ok, 1 = bad arguments (nothing launched; the message is rd_create_error()'s), 2 = max_out too small (*n_out holds the
 * need), 3 = a record disagrees with the host's arithmetic. */
#define RD_CHECKBOX_MAX_SIDE 16384
#define RD_CHECKBOX_MAX_PAGES 1024
#define RD_CHECKBOX_ROI_ROWS 70
#define RD_CHECKBOX_WS_PARTS 13
#define RD_CHECKBOX_RUNS_OVERFLOW 1
#define RD_CHECKBOX_CANDS_OVERFLOW 2
typedef struct rd_checkbox_page {
    int32_t n_runs;       /* runs of the complement of the dilated line mask */
    int32_t flags;        /* RD_CHECKBOX_*_OVERFLOW */
    int32_t n_comp;       /* 8-connected components of that complement */
    int32_t n_cand;       /* components that pass the size filter, the first in label order left out */
    int32_t first_key;    /* key of the first component in label order (the one stats[2:] drops), -1 without components */
    int32_t cand_off;     /* index of the page's first record */
    int32_t reserved[2];
} rd_checkbox_page;
typedef struct rd_checkbox_cand {
    int32_t key;                          /* label order: (min y / 2) << 16 | x / 2 of the component's first 2 x 2 block */
    int32_t tick;                         /* countNonZero of the opened adaptive threshold of image[y : y + h, x : x + w] */
    int16_t x, y, w, h;                   /* the component's bounding box */
    int16_t rx, ry, rw, rh;               /* the ROI of the contour rule */
    uint64_t roi[RD_CHECKBOX_ROI_ROWS];   /* its rows of the dilated line mask, bit i = column rx + i; rows >= rh are zero */
} rd_checkbox_cand;
typedef struct rd_checkbox_box { int32_t x, y, w, h, ticked; } rd_checkbox_box;
size_t rd_checkbox_workspace(int P, int H, int W, int max_runs, int max_cand, size_t* offsets);
int rd_checkbox_detect_device(int device_id, const uint8_t* pages_dev, int P, int H, int W, int bgr, int max_runs, int max_cand, void* ws_dev,
                              size_t ws_bytes, rd_checkbox_page* hdr_dev, rd_checkbox_cand* cands_dev, void* stream);
int rd_checkbox_finish(const rd_checkbox_cand* cands, int n, int H, int W, rd_checkbox_box* out, int max_out, int32_t* n_out);

/* Region composition on the device (csrc/kernels_region.hip, csrc/region_geom.h; docs/notebook/region_compose.md): the canvases that the
 * OCR and table stages hand to the detector and the recogniser - crop_img (rapid_doc/utils/model_utils.py:90-124) with its polygon mask and
 * _apply_mask_boxes_to_image (analyze_utils.py:82-103) - for n regions in one launch.  Every region names its own page, so the pages of a
 * launch may differ in size.  Canvas k of canv_dev [n][gh][gw][3] u8 is
 *     255 everywhere;
 *     the page pixel where the canvas pixel maps into the region rectangle clipped to the page: x0c = max(0, x0), x1c = min(page_w, x1),
 *     the same for y, at canvas offset paste + (clipped - unclipped);
 *     with a polygon, 255 again wherever cv2.fillPoly's raster of the polygon - translated by the UNclipped (x0, y0), on a window of the
 *     clipped size [y1c - y0c][x1c - x0c] - is not set (rd_fill_poly's pixels exactly; vertices are int32, truncated by the caller).
 * det_canv_dev (may be NULL: not written) is the same canvas with every mask box of the region at 255.
 * ws_dev: rd_region_canvases_workspace bytes of device scratch (0 on bad arguments) when any region has a polygon, else unused and may be
 * NULL; pts_dev / boxes_dev may be NULL when no region has a polygon / a box.  The descriptors and the boxes are read back on `stream` and
 * checked before anything is launched (64 bytes a region, 16 a box; the stream is synchronised).  Return 0 = ok, 1 = bad arguments -
 * NULL pointers, n < 1, gh or gw outside 1 .. 16384, a polygon above RD_REGION_MAX_POLY, a box that is empty or leaves its canvas,
 * coordinates beyond +-2^28, a workspace that is too small: nothing launched, the message is rd_create_error()'s. */
#define RD_REGION_MAX_POLY 64
typedef struct rd_region_desc {
    const uint8_t* page;      /* device address of the page's pixel (0,0), channel 0 (3-channel u8 HWC) */
    int64_t pitch;            /* bytes per page row (a page may be a window of a larger buffer) */
    int32_t page_w, page_h;
    int32_t x0, y0, x1, y1;   /* region rectangle in page coordinates, UNclipped (may overhang or miss the page) */
    int32_t paste_x, paste_y; /* canvas position of (x0, y0) */
    int32_t poly_off, poly_n; /* vertices in pts_dev (int32 x, y pairs, page coordinates); poly_n = 0: none */
    int32_t box_off, box_n;   /* mask boxes in boxes_dev (int32 x0, y0, x1, y1 in CANVAS coordinates, already clipped, non-empty) */
} rd_region_desc;
size_t rd_region_canvases_workspace(int n, int gh, int gw);
int rd_region_canvases(int device_id, const rd_region_desc* descs_dev, int n, const int32_t* pts_dev, const int32_t* boxes_dev,
                       int gh, int gw, uint8_t* canv_dev, uint8_t* det_canv_dev /* may be NULL */, void* ws_dev, size_t ws_bytes, void* stream);

/* Host images behind the plugin seam (csrc/stage_pack.cpp, csrc/kernels_stage.hip; docs/notebook/plugin_seams.md): the crops an
 * unmodified RapidDoc hands to a `custom_model` are numpy arrays in pageable host memory.  rd_stage_pack gathers them into ONE pinned
 * buffer, the caller uploads that buffer with one copy, rd_stage_canvases composes the detector canvases of every size group of the
 * call from the uploaded bytes in ONE launch.
 *
 * rd_stage_pack (host only, no device call): image i is u8 [hs[i]][ws[i]][3] at srcs[i], rows pitches[i] bytes apart, pixels 3 bytes
 * apart, channels 1 byte apart; its rows are copied, packed (row pitch 3 * ws[i]), to dst + offsets[i].  The rows of all images are
 * shared out by bytes among at most n_threads threads (capped at 16; fewer for a small total).  Everything is checked before the first
 * byte is written.  Return 0 = ok (n = 0 included), 1 = bad arguments - a NULL array or dst, n < 0, dst_bytes < 0, a negative size or
 * offset, an image with pixels whose source is NULL or whose pitch is below 3 * ws[i] while it has more than one row, an image that
 * overruns dst_bytes: nothing written.  Images may not overlap in dst; that is the caller's layout and is not checked. */
int rd_stage_pack(const uint8_t* const* srcs, const int64_t* pitches, const int32_t* hs, const int32_t* ws, const int64_t* offsets, int n,
                  uint8_t* dst, int64_t dst_bytes, int n_threads);

/* rd_stage_canvases: canvas k (u8 [gh][gw][3] at `canvas`, a device address that is a multiple of 4) is 255 everywhere and crop k
 * (u8 [h][w][3] at `src`, any byte address, rows `pitch` bytes apart) at (0, 0), its first and third channel exchanged when bit 0 of
 * `flags` is set - the canvases analyze.RegionTextModel hands to the detector.  Every canvas byte is written exactly once, nothing
 * outside the canvases is written, and no byte outside [src + y * pitch, src + y * pitch + 3 * w) of a row y < h is read.  The canvases
 * of a launch may differ in size.  descs_host and descs_dev hold the same n descriptors, on the host and on the device (uploaded on
 * `stream` by the caller): the checks read the host copy, so nothing is read back and the stream is not synchronised.  Return 0 = ok,
 * 1 = bad arguments - a NULL array, n outside 1 .. 65535, a NULL or misaligned canvas, gh or gw outside 1 .. 16384, gw % 4 != 0,
 * w > gw, h > gh, a negative size, a crop with pixels whose src is NULL or whose pitch is below 3 * w while it has more than one row:
 * nothing launched, the message is rd_create_error()'s. */
#define RD_STAGE_SWAP_RB 1u
typedef struct rd_stage_desc {
    const uint8_t* src;       /* device address of the crop's pixel (0,0), channel 0 */
    int64_t pitch;            /* bytes per crop row */
    uint8_t* canvas;          /* device address of this crop's canvas */
    int32_t w, h;             /* crop size */
    int32_t gh, gw;           /* canvas size */
    uint32_t flags;           /* RD_STAGE_SWAP_RB */
    uint32_t reserved;        /* 0 */
} rd_stage_desc;
int rd_stage_canvases(int device_id, const rd_stage_desc* descs_host, const rd_stage_desc* descs_dev, int n, void* stream);

/* Host: chunk sizes of the recogniser's THROUGHPUT mode (the engine's own scheduling; rapidocr's fixed rec_batch_num chunks,
 * rapid_doc/model/ocr/rapid_ocr.py:430-440, are the `strict` mode of rapiddoc_amd.pipeline.PagePipeline).  wpad_sorted[i] = padded
 * width of the i-th line of the aspect-sorted list (int(48 * max(320/48, w/h)) rounded up to the width multiple); a chunk is a run of
 * that list padded to its last line.  rd_rec_plan_chunks cuts the list so that the summed rd_rec_chunk_cost (estimated microseconds
 * of a backbone forward: whole rounds of workgroup tiles on n_cu compute units per persistent kernel + a linear term + a per-forward
 * constant) is minimal; candidate sizes n_min, n_min + n_step, ... <= n_max, the last chunk any size.  Returns 0 on success. */
double rd_rec_chunk_cost(int n_lines, int wpad, int n_cu);
int rd_rec_plan_chunks(const int32_t* wpad_sorted, int n, int n_min, int n_max, int n_step, int n_cu, int32_t* sizes_out, int max_out,
                       int32_t* n_out);
/* Host, strict mode: all of the line bookkeeping between the crop sizes and the launches in one call.  ratios[n] = w/h of the pooled
 * lines, order[n] = their sort order (the caller's np.argsort, the reference's own call: rapid_ocr.py:414).  Chunks of rec_batch_num
 * lines of that order give line i of the SORTED list its reference width line_w_out[i] = int(img_h * max(img_w / img_h, chunk max ratio))
 * (double arithmetic) and line_ratio_out[i] = that maximum (CTCLabelDecode's max_wh_ratio); the widths rounded up to launch_multiple go
 * through rd_rec_plan_chunks: sizes_out / launch_w_out [*n_out <= max_out] = lines and tensor width of every launch.  Returns 0 on
 * success, 1 on bad arguments (an index of `order` outside [0, n), a ratio that is not finite). */
int rd_rec_plan_lines(const double* ratios, const int64_t* order, int n, int rec_batch_num, int img_h, int img_w, int launch_multiple,
                      int n_min, int n_max, int n_step, int n_cu, int64_t* line_w_out, double* line_ratio_out, int32_t* sizes_out,
                      int32_t* launch_w_out, int max_out, int32_t* n_out);

/* Arithmetic of the dense layers of a network handle; every mode returns fp32 tensors with fp32-level error
 * (the reference runs the same layers through onnxruntime / torch fp32: rapid_doc/model/ocr/.../torch.py:58-76).
 *   "auto" (default)  split-fp16 matrix cores ((hi, lo) operand splitting, 3 fp16 MFMAs per product, fp32 accumulate,
 *                     measured error vs fp64 at or below the fp32 MFMA path's) for the fused PPLCNetV4 channel mixers,
 *                     the CTC head, 1x1 convs with K >= 96 and N >= 96, k x k convs with K >= 96 and N >= 24 and the
 *                     small-K stem layers; fp32 MFMA for the rest (narrow / short layers, M < 2048).
 *   "fp32"            native fp32 MFMA only.
 *   "h3"              every dense layer split (experimental; needs RD_PRECISION=h3 in the environment at rd_load_weights).
 * Split operands must stay inside the fp16 range (|v| < 65504).  The kernels never return a silently wrong answer:
 * they raise a flag instead, which rd_range_status() returns (1) and clears after synchronising `stream`; the caller
 * then switches the handle to "fp32" and repeats the forward call.  rd_range_status returns -1 on error. */
int rd_set_precision(rd_handle* h, const char* mode);
int rd_range_status(rd_handle* h, void* stream);

/* Cache behaviour of a handle since rd_create: per-shape plans built, hipGraph captures and hipGraph replays (each may be NULL).
 * A forward on a new (B, H, W, flags) builds a plan on the host; the second time a (plan, pointers, stream) triple shows up it is
 * captured, from the third on replayed.  bench.py reports the plans a non-repeating document stream builds inside its timed region. */
int rd_plan_stats(rd_handle* h, uint64_t* plans_built, uint64_t* graph_captures, uint64_t* graph_replays);

/* per-op HIP-event timing of the NEXT forward calls; rd_profile_json returns the last call's table as a JSON
 * array [{"name","kind","cfg","flops","bytes","ms"}, ...] owned by the handle. */
int rd_set_profiling(rd_handle* h, int on);
const char* rd_profile_json(rd_handle* h);

#ifdef __cplusplus
}
#endif
#endif
