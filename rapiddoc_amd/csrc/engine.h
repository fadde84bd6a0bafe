// Host-side runtime of the MI355X page-inference engine: weight store (safetensors image), folded
// parameter block, static memory planner, op list ("plan") per input shape, executor with optional
// per-op HIP-event profiling.  One Engine = one network on one device; not thread-safe.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "rd_kernels.h"

namespace rd {

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};
#define RD_CHECK(cond, msg)                                                          \
    do {                                                                             \
        if (!(cond)) throw ::rd::Error(std::string(msg) + " [" #cond "]");           \
    } while (0)
#define RD_HIP(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) throw ::rd::Error(std::string(#expr ": ") + hipGetErrorString(_e));          \
    } while (0)

// ------------------------------------------------------------------------------------------------
struct HostTensor {
    std::vector<int64_t> shape;
    std::string dtype;
    const uint8_t* data = nullptr;
    size_t nbytes = 0;
    size_t numel() const {
        size_t n = 1;
        for (auto d : shape) n *= (size_t)d;
        return n;
    }
    const float* f32() const { return reinterpret_cast<const float*>(data); }
};

class WeightStore {
   public:
    void load_safetensors(const void* blob, size_t nbytes);  // copies the image; strips a leading "model."
    bool has(const std::string& name) const { return map_.count(name) != 0; }
    const HostTensor& get(const std::string& name) const;
    size_t size() const { return map_.size(); }
    void clear() { map_.clear(); blob_.clear(); blob_.shrink_to_fit(); derived_.clear(); }
    // a tensor computed from loaded ones at load time (a folded multi-branch convolution): served by get() like a tensor of the file
    void add_derived(const std::string& name, const std::vector<int64_t>& shape, std::vector<float>&& data);

   private:
    std::vector<uint8_t> blob_;
    std::unordered_map<std::string, HostTensor> map_;
    std::vector<std::unique_ptr<std::vector<float>>> derived_;
};

// Folded, re-laid-out parameters in one device allocation.
class ParamBlock {
   public:
    ~ParamBlock();
    size_t add(const std::string& key, const std::vector<float>& v);
    size_t add_u16(const std::string& key, const std::vector<uint16_t>& v);  // packed into the same block
    bool has(const std::string& key) const { return off_.count(key) != 0; }
    void upload();
    const float* ptr(const std::string& key) const;
    const float* host_ptr(const std::string& key) const;   // before upload(): the folded host copy
    size_t bytes() const { return host_.size() * sizeof(float); }

   private:
    std::vector<float> host_;
    std::unordered_map<std::string, size_t> off_;
    float* dev_ = nullptr;
};

// ------------------------------------------------------------------------------------------------
struct Buf {
    int n = 0, h = 0, w = 0, c = 0;
    size_t off = 0, bytes = 0;
    int external = -1;  // >= 0: slot in the run-time external pointer table
    bool live = false;
};
struct TView {  // channel slice [coff, coff+c) of an NHWC buffer
    int buf = -1, coff = 0;
    int n = 0, h = 0, w = 0, c = 0;
    long pixels() const { return (long)n * h * w; }
};

struct RunCtx {
    uint8_t* arena = nullptr;
    std::vector<void*> ext;
    hipStream_t stream = nullptr;
};

struct OpRecord {
    std::string name, kind, cfg, shape;
    double flops = 0, bytes = 0;
    std::function<void(const struct Plan&, const RunCtx&)> run;
};

// One captured replay of a plan: valid for exactly these external pointers, this workspace and this stream (the kernel
// arguments inside the graph are raw addresses).
struct GraphSlot {
    std::vector<void*> ext;
    uint8_t* arena = nullptr;
    hipStream_t stream = nullptr;
    hipGraphExec_t exec = nullptr;
    uint64_t last_use = 0;
};

struct Plan {
    ~Plan();
    std::vector<Buf> bufs;
    std::vector<OpRecord> ops;
    size_t arena_bytes = 0;
    mutable uint64_t last_use = 0;   // Engine::plan_for's LRU clock
    mutable std::vector<GraphSlot> graphs;   // Engine::run: hipGraph replays of this plan (at most kMaxGraphSlots)
    mutable bool graph_broken = false;       // a capture of this plan failed once: launch directly from then on
    mutable unsigned graph_evictions = 0;    // slots dropped for newer pointer sets: past kMaxGraphEvictions the plan stops capturing
    std::vector<TView> outputs;  // model specific
    float* vptr(const TView& v, const RunCtx& c) const {
        const Buf& b = bufs[v.buf];
        uint8_t* base = b.external >= 0 ? (uint8_t*)c.ext[b.external] : c.arena + b.off;
        return reinterpret_cast<float*>(base) + v.coff;
    }
    int ld(const TView& v) const { return bufs[v.buf].c; }
};

struct ProfileEntry {
    std::string name, kind, cfg, shape;
    double flops, bytes;
    float ms;
};

enum class Mode { PREPARE, PLAN };

// Network description helper shared by every model builder.  In PREPARE mode it folds weights into the
// parameter block; in PLAN mode it allocates buffers and records kernel launches for one input shape.
class Builder {
   public:
    Builder(Mode m, const WeightStore* ws, ParamBlock* pb, Plan* plan, bool h3 = false, bool mixer_h3 = false,
            unsigned* range_flag = nullptr)
        : mode_(m), h3_(h3), mixer_h3_(mixer_h3), range_flag_(range_flag), ws_(ws), pb_(pb), plan_(plan) {}
    bool h3() const { return h3_; }
    Mode mode() const { return mode_; }
    bool planning() const { return mode_ == Mode::PLAN; }

    // --- memory
    TView alloc(int n, int h, int w, int c);
    TView external(int slot, int n, int h, int w, int c);
    TView slice(const TView& v, int coff, int c) const;
    TView reshape(const TView& v, int n, int h, int w) const;  // same pixel count, full-width view only
    void release(const TView& v);
    TView alloc_raw(size_t nfloats);  // scratch as [1,1,1,n]

    // The recogniser's per-line width table (rd_kernels.h LineTab, an int32 external [B][4]): from here on stem_front, dwconv,
    // se_gate and avgpool3x2 treat image n as line_tab[n]-wide (REC_LINE_WIDTHS plans only).
    void set_line_table(const TView& t) { lt_ = t; has_lt_ = true; }
    // zero the columns >= line_tab[n][col] of v (no-op without a line table): the separate-kernel stem of the fp32 mode
    void mask_cols(const TView& v, int col);

    // --- layers.  `key` = reference state-dict prefix of the layer.
    struct ConvGeom {
        int kh = 1, kw = 1, sh = 1, sw = 1, pt = 0, pl = 0, pb = 0, pr = 0;
    };
    // conv weight `wname` [Cout,Cin,kh,kw] (+ optional bias `bname`) (+ optional BatchNorm `bn` prefix, folded)
    TView conv(const std::string& wname, const std::string& bname, const std::string& bn, const TView& x,
               const ConvGeom& g, int act, const TView* out = nullptr, const TView* res = nullptr,
               const TView* ascale = nullptr);
    // fused PPLCNetV4 residual channel mixer (prefix.channel_conv1/2); gate = optional SE gate [N,1,1,C]
    // `dw_key`: (round 6) x is the block's INPUT and the mixer computes the block's depthwise 3x3 / stride 1 itself from the weights
    // Builder::dwconv folded under that key (only where mixer_takes_dw says so)
    TView mixer_fused(const std::string& prefix, const TView& x, const TView* gate, const std::string* dw_key = nullptr);
    // true when, in THIS plan, the channel mixer of `prefix` will run on the kernel that can take the block's depthwise conv along
    bool mixer_takes_dw(const std::string& prefix, int C) const;
    static std::string dw_key(const std::string& wname, const std::string& bn) { return wname + "|" + bn + "|dw"; }
    void fold_conv(const std::string& wname, const std::string& bname, const std::string& bn, int row0 = 0, int nrows = 0);
    // From here on (until set back to 0, 0) Builder::conv computes output channels [row0, row0 + nrows) of its layer only: weight rows, BatchNorm
    // and bias of that piece, folded under their own key; `out` is the piece's channel slot.  A wide 3x3 layer as two launches of the
    // <= 96-channel direct kernel (PPHGNet_small's 160- and 192-channel layers: docs/notebook/v4_server.md)
    void set_conv_rows(int row0, int nrows) { rows_0_ = row0; rows_n_ = nrows; }
    static std::string conv_rows_suffix(int row0, int nrows);
    TView linear(const std::string& prefix, const TView& x, int act, const TView* out = nullptr,
                 const TView* res = nullptr);
    // ConvTranspose2d(2, 2) + BN + ReLU -> ConvTranspose2d(2, 2) to ONE channel -> sigmoid, fused when the widths allow (DB head tail)
    bool deconv_pair_to_prob(const std::string& w1n, const std::string& b1n, const std::string& bn1, const std::string& w2n,
                             const std::string& b2n, const TView& x, const TView& out);
    TView deconv2x2(const std::string& wname, const std::string& bname, const std::string& bn, const TView& x, int act,
                    const TView* out = nullptr);
    TView stem3x3s2(const std::string& wname, const std::string& bn, const TView& x_nchw, int act);
    // stem1 -> [max-pool | stem2a -> stem2b] -> the 2 c1-channel concat buffer at half resolution (StemBlock front).  One fused
    // kernel in the split-fp16 precision modes (kernels_stem_fused.hip), the four separate kernels otherwise.
    TView stem_front(const std::string& w1, const std::string& bn1, const std::string& w2a, const std::string& bn2a,
                     const std::string& w2b, const std::string& bn2b, const TView& x_nchw);
    // stem3 (3x3 / stride 2 / pad 1 + BN + act) -> stem4 (1x1 + BN + act): one fused kernel in the split-fp16 precision modes
    // (kernels_stem34.hip, round 6), the two convolutions otherwise.  `out`: where stem4's output goes (a channel slot of a concat buffer)
    // `s3`: stride of stem3 (2; 1 in the text-recognition geometry of PPHGNetV2 - the fused kernel is a stride-2 kernel, stride 1 takes
    // the two convolutions)
    TView stem_tail(const std::string& w3, const std::string& bn3, const std::string& w4, const std::string& bn4, const TView& x, int act3,
                    int act4, const TView* out = nullptr, int s3 = 2);
    // 1 x 3 sequence convolution over token rows (kernels_seqconv.hip): weight `wname` [Cout][C0 + C1][1 | 3][3] (of a 3 x 3 only the middle
    // row: the map is one row high, the other two only ever meet padding) + BatchNorm `bn`; x0 / x1 = the two K segments (x1 may be null).
    // Uniform form: x0 is [B][1][T][C0]; ragged form: [1][1][W][C0] with tokinfo (as Builder::dwconv)
    TView seqconv(const std::string& wname, const std::string& bn, const TView& x0, const TView* x1, int act, const TView* tokinfo = nullptr);
    struct GapOut { TView partial; int chunks = 0; };  // per-image partial sums of a layer's output (SE pooling)
    TView dwconv(const std::string& wname, const std::string& bname, const std::string& bn, const TView& x,
                 const ConvGeom& g, int act, const TView* out = nullptr, const TView* res = nullptr, GapOut* gap = nullptr,
                 const TView* tokinfo = nullptr);   // tokinfo: ragged rows (DwParams::tokinfo), an int32 external of x.pixels() entries
    // PFHeadLocal's local tail in one kernel (kernels_det_local.hip): out = 0.5 (shrink + sigmoid(last_1(relu(bn(last_3(cat[shrink, up2(f)]))))));
    // f [N][H/2][W/2][64], shrink [N][H][W][1], out [N][H][W][1].  No full-resolution 64- or 65-channel tensor is written
    void det_local_tail(const std::string& w3n, const std::string& bn3, const std::string& w1n, const std::string& b1n, const TView& f,
                        const TView& shrink, const TView& out);
    // PPLCNetV3 (kernels_lcv3.hip).  A scalar affine y = s x + b (LearnableAffineBlock); `pre` (when given) = the act.lab of the pointwise
    // layer that produced x: that layer wrote conv + bias only and its consumer applies hardswish + act.lab on load; `post` = the layer's own.  lt_in / lt_out: LineTab columns of the valid
    // input / output width under a line table
    struct Affine { float s = 1.f, b = 0.f; };
    Affine affine(const std::string& prefix) const;      // prefix.scale / prefix.bias
    // `strip`: route of a 5x5 layer that the LDS-staged strip kernel serves (kernels_mv1e.hip, dw5_strip_launch_ok).  0: the direct kernel;
    // 1: the strip kernel under RD_LCV3_DW_STRIP=1 only (opt-in, ppocrv5_rec_mobile); 2: the per-geometry default mv1e_dw_strip_default,
    // RD_MV1E_DW_STRIP=0|1 forcing one route for every layer the strip kernel serves (ppocr_rec_mv1e).  Read per plan
    TView lcv3_dw(const std::string& wname, const std::string& bname, const TView& x, int k, int sh, int sw, const Affine* pre, Affine post, int lt_in,
                  int lt_out, int strip = 0);
    // MobileNetV1Enhance's end (kernels_mv1e.hip): the deferred hardswish, AvgPool2d(2, 2) over rows 0-1 of the 3-row map
    TView mv1e_pool(const TView& x, const TView* out = nullptr);
    // the detector geometry: `post` null = convolution + bias only (a stride-2 layer); `level` = log2 of the input map's reduction of the
    // page (1 = H/2 ... 5 = H/32), which with (k, stride, C) picks the direct or the LDS-staged kernel (lcv3_dw2d_default; RD_LCV3_DW2D=0|1
    // forces one route for every layer the staged kernel serves)
    TView lcv3_dw_det(const std::string& wname, const std::string& bname, const TView& x, int k, int stride, const Affine* pre, const Affine* post,
                      int level);
    bool lcv3_dw_common(const std::string& wname, const std::string& bname, const TView& x, int k, int sh, int sw, const Affine* pre, const Affine* post,
                        TView* y, Lcv3DwParams* p, OpRecord* r);   // shared by the two builders above; false in PREPARE mode
    // shared by mbv3_dw (P = Mbv3DwParams, net "mbv3") and mbv3s_dw (P = Mbv3sDwParams, net "mbv3s") below, in the same way (builder_mobile.cpp)
    template <typename P>
    bool mbv3_dw_common(const std::string& net, const std::string& wname, const std::string& bname, const TView& x, int k, int sh, int sw, int pre_act,
                        int post_act, TView* y, P* p, OpRecord* r);
    TView lcv3_act(const TView& x, Affine a);             // a hardswish(x) + b, elementwise (kernels_lcv3_det.hip)
    // MobileNetV3 in the detector geometry (kernels_mbv3.hip).  The depthwise layer alone: pre_act = the producer's activation, applied on
    // load inside the map; post_act = the layer's own (Mbv3Act)
    // `level` = log2 of the input map's reduction of the page: with (k, stride, C) it picks, for a hardswish layer of C % 16 == 0, the
    // LDS-staged lcv3_dw2d_kernel (mbv3_dw2d_default; RD_MBV3_DW2D=0|1 forces one route for every layer that kernel serves)
    TView mbv3_dw(const std::string& wname, const std::string& bname, const TView& x, int k, int stride, int pre_act, int post_act, int level);
    // One inverted-residual block `prefix`.{expand,bottleneck,linear}_conv.fold.* in one launch; in_hswish: x is conv1's convolution + bias,
    // activated on load.  `level` = log2 of the input map's reduction of the page.  Taken where mbv3_block_launch_ok serves the geometry AND
    // (RD_MBV3_FUSED=0|1, read per plan, forcing one route for every such block) mbv3_fused_default says so.  false: not taken (always in
    // PREPARE mode: the parameters are those the separate operators fold), the caller emits expand -> depthwise -> linear
    bool mbv3_block(const std::string& prefix, const TView& x, int k, int stride, int act, bool in_hswish, bool shortcut, int level, TView* y);
    // MobileNetV3 small in the text-line geometry (kernels_mbv3s.hip): the depthwise layer with separate row / column strides, C % 8 == 0;
    // pre_act / post_act as mbv3_dw
    TView mbv3s_dw(const std::string& wname, const std::string& bname, const TView& x, int k, int sh, int sw, int pre_act, int post_act);
    // the classifier's end: x = conv2's convolution + bias -> hardswish -> MaxPool2d(2, 2) -> global average -> Linear `prefix` (C -> 2) ->
    // softmax into prob_ext [B,2]; aux_ext (optional) [B, 2 + C] = logits | pooled features
    void cls_tail(const std::string& prefix, const TView& x, const TView& prob_ext, const TView* aux_ext);
    // The whole classifier in ONE launch (cls_line_kernel, kernels_mbv3s.hip): conv1 `stem_w` / `stem_bn`, the blocks, conv2 `conv2` (folded
    // weight / bias names), the head `head`.  Reads the parameters the separate operators fold, so it is never taken in PREPARE mode.  Taken
    // where cls_line_plan holds the shape AND RD_CLS_FUSED=0|1 (read per plan) or, without it, cls_fused_default says so.  false: not
    // taken, the caller emits the separate operators.  stages: four externals for the outputs of blocks stage_block[0..3] (developer), or null
    struct ClsBlockDesc { std::string prefix; int k, cin, mid, cout, sh; bool se; int act; };
    bool cls_line(const std::string& stem_w, const std::string& stem_bn, const std::vector<ClsBlockDesc>& blocks, const std::string& conv2,
                  const std::string& head, const TView& x, const TView& prob_ext, const TView* aux_ext, const TView* stages, const int* stage_block);
    // one block without SE (3x3, stride 1) in one launch (kernels_lcv3_block.hip), writing the pointwise layer's convolution + bias as the separate
    // route does.  Taken under RD_LCV3_FUSED=1 in the split precisions; false: not taken (and always in PREPARE mode, where it only adds its
    // parameters), the caller emits the separate operators
    void prepare_lcv3_block(const std::string& key, const HostTensor& w, const std::string& pw_b);
    bool lcv3_block(const std::string& dw_w, const std::string& pw_w, const std::string& pw_b, const TView& x, const Affine* pre, Affine mid, int lt_col,
                    TView* y);
    GapOut lcv3_gap(const TView& x, int lt_col);          // SE pooling partial sums of x, one chunk per row
    TView lcv3_pool(const TView& x, Affine post, const TView* out = nullptr);   // the deferred hardswish, avg_pool2d([3, 2]), the deferred affine
    void maxpool2x2s1(const TView& x, const TView& out);
    TView maxpool3x3s2(const TView& x, const TView* out = nullptr);                // MaxPool2d(3, stride 2, padding 1), -inf padding (kernels_ese.hip)
    // ESE gate of an HG_Block (kernels_ese.hip): out = x sigmoid(conv1x1(mean_hw(x)) + bias) (+ idn); `prefix`.weight [C][C][1][1], `prefix`.bias;
    // out may be x itself or a channel slot of another buffer
    void ese(const std::string& prefix, const TView& x, const TView& out, const TView* idn = nullptr);
    // From here on (until switched off again) the 3x3 layers that conv3x3_wide_shape_ok serves get that kernel's weight image and ask for
    // its route in the "auto" precision.  A builder-side opt-in (PPHGNet_small): no layer moves onto the kernel by its shape alone
    void set_conv3x3_wide(bool on) { wide3x3_ = on; }
    TView avgpool3x2(const TView& x, const TView* out = nullptr);
    // squeeze-excite gate s[n][c]; `w1/b1/w2/b2` full tensor names
    TView se_gate(const std::string& w1, const std::string& b1, const std::string& w2, const std::string& b2,
                  const TView& x, int gate_act, const GapOut* pre = nullptr, int lt_col = 2);   // lt_col: LineTab column of x's valid width
    void scale(const TView& x, const TView& gate, float alpha, const TView& out);
    void upsample(const TView& x, const TView& out, int f, bool accumulate);
    TView layernorm(const std::string& prefix, const TView& x, float eps);
    // seg: ragged batch - int32 external [B][2] = (first token, tokens) of every sequence; T = the longest sequence
    TView attention(const TView& qkv, int B, int T, int heads, int hd, const TView* seg = nullptr);
    // ViT pieces (kernels_vit_attn.hip).  vit_attention: head dimension 64, dense [B][T] batches, T <= 1024, every precision mode alike
    TView vit_attention(const TView& qkv, int B, int T, int heads);
    TView vit_patchify(const TView& x_nchw);                       // [B,H,W,3]-described NCHW external -> [B,1,T,768] patch rows
    void add_pos(const std::string& wname, const TView& x, int B, int T);   // x [B][T][C] += rows 0..T-1 of the embedding table `wname`, in place
    TView add(const TView& a, const TView& b);
    void to_nchw(const TView& x, const TView& out_ext);
    void copy(const TView& x, const TView& out);   // same geometry, possibly different channel strides
    void ctc_stats(const TView& logits, const TView& idx_ext, const TView& prob_ext);
    void softmax_rows(const TView& logits, const TView& out_ext, const TView* idx_ext = nullptr, const TView* prob_ext = nullptr);
    void ctc_head(const std::string& prefix, const TView& x, const TView& idx_ext, const TView& prob_ext);

    const HostTensor& weight(const std::string& name) const { return ws_->get(name); }
    bool has_weight(const std::string& name) const { return ws_ && ws_->has(name); }
    int weight_dim(const std::string& name, int d) const;

   private:
    void emit(OpRecord&& r) { plan_->ops.push_back(std::move(r)); }
    std::vector<float> bn_scale_shift(const std::string& bn, int c, std::vector<float>& shift) const;
    // the kernel the channel mixer of `prefix` runs on in this plan (mixer_fused launches it, mixer_takes_dw asks about it)
    enum MixerRoute { MIXER_F32, MIXER_H3, MIXER_WS, MIXER_RES };
    MixerRoute mixer_route(const std::string& prefix, int C) const;
    Mode mode_;
    bool h3_ = false;        // every dense layer on the fp16 matrix cores with hi/lo operand splitting (fp32-accurate)
    bool mixer_h3_ = false;  // only the fused channel mixers (the default "auto" precision)
    unsigned* range_flag_ = nullptr;   // device word the split kernels raise when an operand leaves the fp16 range
    const WeightStore* ws_;
    ParamBlock* pb_;
    Plan* plan_;
    struct Block { size_t off, size; bool free; };
    std::vector<Block> blocks_;
    TView lt_;
    bool has_lt_ = false;
    bool wide3x3_ = false;
    int rows_0_ = 0, rows_n_ = 0;
};

// ------------------------------------------------------------------------------------------------
// The model table (models.cpp): every engine kind is described ONCE, in the row next to its builder.  The Engine and the C surface look
// a kind up here; nothing else lists the kinds.  (The two autoregressive decoders, "ppformulanet_head" and "unitable_decoder", are not
// Engines and are not in the table.)
enum class ModelFamily { Detector, Recogniser, Classifier, TableEncoder, Backbone, FormulaEncoder };
struct ModelDesc {
    const char* kind;
    ModelFamily family;
    void (*build)(Builder& b, int B, int H, int W, int flags);
    void (*derive)(WeightStore& ws);       // adds the tensors `build` reads that are not in the file; null: there are none
    // PREPARE mode folds the weights by building these geometries (the smallest legal ones; only weight names / shapes matter there)
    struct Geom { int B, H, W, flags; };
    std::vector<Geom> prepare;
    // recognisers: n_classes = shape[0] of the first tensor, rec_token_dim = shape[1] of the second
    const char* n_classes_tensor;
    const char* token_dim_tensor;
    // what the C surface offers for the kind
    bool rec_line_widths;    // rd_rec_backbone_forward_lines (REC_LINE_WIDTHS)
    bool det_want_neck;      // rd_det_forward_ex with RD_DET_WANT_NECK
    bool derived_tensors;    // rd_debug_derived_tensor
};
const std::vector<ModelDesc>& model_table();
const ModelDesc* find_model(const std::string& kind);   // null: not an engine kind

class Engine {
   public:
    explicit Engine(int device, const std::string& kind);
    ~Engine();
    const std::string& kind() const { return kind_; }
    const ModelDesc& model() const { return *model_; }   // the kind's row of the model table, resolved by the constructor
    void load_weights(const void* blob, size_t nbytes);
    bool loaded() const { return loaded_; }

    // shape key -> plan (built lazily, cached)
    // flags: model-specific plan variants (RD_REC_* bits)
    const Plan& plan_for(int B, int H, int W, int flags = 0);
    size_t workspace_bytes(int B, int H, int W, int flags = 0) { return plan_for(B, H, W, flags).arena_bytes; }
    // run with caller-provided externals (model specific order); ws may be null (internal arena)
    void run(int B, int H, int W, int flags, const std::vector<void*>& ext, void* ws, size_t ws_bytes, hipStream_t s);

    // plans built / hipGraph captures / hipGraph replays since the handle was created (a document stream keeps meeting new shapes:
    // bench.py reports how many of them fell into its timed region)
    uint64_t plans_built() const { return plans_built_; }
    uint64_t graph_captures() const { return graph_captures_; }
    uint64_t graph_replays() const { return graph_replays_; }
    void set_profiling(bool on) { profiling_ = on; }
    const std::vector<ProfileEntry>& last_profile() const { return profile_; }
    std::string profile_json() const;
    int n_classes() const { return n_classes_; }
    int rec_token_dim() const { return rec_token_dim_; }   // channels of the rec backbone's pooled tokens (two-stage form)
    // the backbone the loaded weights picked, for the kinds that serve two ("ppocrv5_det_server", "ppocrv5_rec_server": "pphgnetv2_b4" or
    // "pphgnet_small", the PP-OCRv4 server files); "" for every other kind and before load_weights
    const std::string& backbone() const { return backbone_; }
    bool h3() const { return precision_ == PREC_H3; }
    int device() const { return device_; }
    // Arithmetic of the dense layers.  Every mode returns fp32 results with fp32-level error:
    //   PREC_AUTO  fp32 MFMA everywhere except the fused PPLCNetV4 channel mixers, which run on the fp16 matrix cores with
    //              (hi, lo) operand splitting (3 MFMAs per product, fp32 accumulate; measured error vs fp64 is BELOW the
    //              fp32 MFMA path's).  Split operands must stay inside the fp16 range (|v| < 65504): the kernels raise
    //              the range flag otherwise and the caller re-runs in PREC_FP32 (take_range_flag()).
    //   PREC_FP32  native fp32 MFMA only (the self-attention: the fp32 VALU kernel for every line).      PREC_H3  every dense layer split (experimental; needs RD_PRECISION=h3 at load)
    enum Precision : int { PREC_AUTO = 0, PREC_FP32 = 1, PREC_H3 = 2 };
    void set_precision(int p);
    int precision() const { return precision_; }
    // 1 if a split kernel saw an out-of-range operand since the last call (synchronises the stream); clears the flag
    int take_range_flag(hipStream_t s);

    std::string last_error;

   private:
    int device_;
    std::string kind_;
    const ModelDesc* model_ = nullptr;
    bool loaded_ = false;
    bool profiling_ = false;
    int precision_ = PREC_AUTO;
    bool h3_prepared_ = false;
    unsigned* range_flag_ = nullptr;          // device address of ...
    unsigned* range_flag_host_ = nullptr;     // ... this word of pinned, mapped host memory
    int n_classes_ = 0;
    int rec_token_dim_ = 0;
    std::string backbone_;
    ParamBlock params_;
    WeightStore store_;
    std::map<std::tuple<int, int, int, int>, std::unique_ptr<Plan>> plans_;
    uint64_t plan_clock_ = 0;
    uint64_t plans_built_ = 0, graph_captures_ = 0, graph_replays_ = 0;
    static constexpr size_t kMaxPlans = 512;   // least recently used plans are dropped beyond this
    static constexpr size_t kMaxGraphSlots = 8;
    static constexpr unsigned kMaxGraphEvictions = 32;   // a plan whose external pointers keep changing never replays: stop capturing it
    // Captured execs that lost their slot.  An exec may have been launched microseconds ago on an asynchronous stream, so it is
    // parked with an event recorded on that stream and destroyed only once the event has completed (sweep_retired_graphs).
    struct RetiredGraph { hipGraphExec_t exec; hipEvent_t done; };
    std::vector<RetiredGraph> retired_graphs_;
    void retire_graph(hipGraphExec_t exec, hipStream_t s);
    void sweep_retired_graphs(bool wait);
    bool graphs_ = true;                       // RD_GRAPHS=0 switches the hipGraph replays off
    uint8_t* arena_ = nullptr;
    size_t arena_bytes_ = 0;
    std::vector<ProfileEntry> profile_;
    std::vector<hipEvent_t> events_;
};

// model builders (models.cpp), all behind the one signature of ModelDesc::build
void build_ppocrv6_det(Builder& b, int B, int H, int W, int flags);   // (no plan variants: flags is ignored)
// REC_STAGE_BACKBONE: image -> pooled tokens only (ext[1] = [B][T][C] out).  REC_STAGE_TAIL: the LightSVTR neck + CTC head over
// the tokens of MANY batches at once (B = text lines, H = longest line in tokens, W = all tokens; ext: 0 tokens, 1 idx,
// 2 prob, 4 seg int32 [B][2], 5 tokinfo int32 [W]) - see build_ppocrv6_rec
// REC_LINE_WIDTHS (with REC_STAGE_BACKBONE): ext[2] = LineTab int32 [B][4] (rd_kernels.h) - every line is computed at ITS OWN padded
// width inside the shared [B,3,48,W] tensor and writes its own number of tokens at its own offset of ext[1]
enum RecFlags : int { REC_UNFUSED_CTC = 1, REC_WANT_SOFTMAX = 2, REC_WANT_LOGITS = 4, REC_STAGE_BACKBONE = 8, REC_STAGE_TAIL = 16, REC_LINE_WIDTHS = 32, REC_WANT_NECK = 64 };
void build_ppocrv6_rec(Builder& b, int B, int H, int W, int flags);
// PP-OCRv5 server recogniser (PPHGNetV2-B4 text_rec + SVTR neck + CTC): same externals, flags and stages; REC_LINE_WIDTHS is refused
void build_ppocrv5_rec_server(Builder& b, int B, int H, int W, int flags);
// PP-OCRv5 mobile recogniser (PPLCNetV3 scale 0.95 + the same SVTR neck + CTC): same externals, flags and stages; REC_LINE_WIDTHS is served
void build_ppocrv5_rec_mobile(Builder& b, int B, int H, int W, int flags);
// tensors build_ppocrv5_rec_mobile reads that are not in the file: every LearnableRepLayer folded into one convolution + bias
void derive_ppocrv5_rec_mobile_weights(WeightStore& ws);
// Multilingual PP-OCRv3 / v4 mobile recognisers (MobileNetV1Enhance scale 0.5 + SVTR neck dims 64 + CTC; ten weight files, one graph):
// same externals, flags and stages; REC_LINE_WIDTHS is served
void build_ppocr_rec_mv1e(Builder& b, int B, int H, int W, int flags);
// tensors build_ppocr_rec_mv1e reads that are not in the file: every Conv + BatchNorm of the backbone's blocks folded into weight + bias
void derive_ppocr_rec_mv1e_weights(WeightStore& ws);
// default route of one 5x5 depthwise layer of that backbone: true = the LDS-staged strip kernel (from the per-geometry A/B of tools/mb_rec_mv1e.py)
bool mv1e_dw_strip_default(int sh, int sw, int c);
// PP-OCRv5 server detector (PPHGNetV2-B4 + LKPAN with IntraCL + PFHeadLocal): ext[0] = x NCHW, ext[1] = maps [B,1,H,W];
// DET_WANT_NECK: ext[2] = the neck output `fuse` NCHW [B,256,H/4,W/4]
enum DetFlags : int { DET_WANT_NECK = 1, DET_WANT_STAGES = 2 };   // DET_WANT_STAGES: ppocrv3_det_mobile only, developer (rd_debug_det_forward_stages): ext[3..6] = its four stage features NCHW
void build_ppocrv5_det_server(Builder& b, int B, int H, int W, int flags);
// The two server kinds take their backbone from the weights: PPHGNet_small (the PP-OCRv4 server files, rec_hgnet.py) when this tensor is
// among them, PPHGNetV2-B4 otherwise
inline const char* pphgnet_small_marker() { return "backbone.stages.0.blocks.0.att.conv.weight"; }
// tensors build_ppocrv5_det_server reads that are not in the file: the three branches of every IntraCL level folded into one k x k convolution
void derive_ppocrv5_det_server_weights(WeightStore& ws);
// PP-OCRv5 mobile detector (PPLCNetV3 scale 0.75 det + RSEFPN 96 + DBHead): externals as the server detector; DET_WANT_NECK: ext[2] = `fuse`
// NCHW [B,96,H/4,W/4]
void build_ppocrv5_det_mobile(Builder& b, int B, int H, int W, int flags);
// tensors build_ppocrv5_det_mobile reads that are not in the file: every LearnableRepLayer folded into one convolution + bias, and
// layer_list[i] followed by ins_conv[i].in_conv as one 1x1 convolution + bias
void derive_ppocrv5_det_mobile_weights(WeightStore& ws);
// default route of one depthwise layer of that backbone: true = the LDS-staged kernel (set from the per-layer A/B table of tools/mb_det_mobile.py)
bool lcv3_dw2d_default(int k, int stride, int c, int level);
// PP-OCRv3 multilingual detector (multi_ / en_PP-OCRv3_det_mobile: MobileNetV3 large scale 0.5 without SE + RSEFPN 96 + DBHead): externals as
// the v5 mobile detector, DET_WANT_NECK included.  Its DBHead has no fix_nan; the shared ACT_SIGMOID maps NaN to 0, which is the identity
// on finite input, so the head tail is the v5 mobile detector's
void build_ppocrv3_det_mobile(Builder& b, int B, int H, int W, int flags);
// tensors build_ppocrv3_det_mobile reads that are not in the file: every Conv + BatchNorm of the backbone's blocks and conv_last folded into
// weight + bias (in double, rounded once)
void derive_ppocrv3_det_mobile_weights(WeightStore& ws);
// default route of one inverted-residual block of that backbone: true = mbv3_block_kernel (set from the per-block A/B table of
// tools/mb_det_v3_mobile.py --routes; a geometry that was not measured stays unfused)
bool mbv3_fused_default(int k, int stride, int cin, int mid, int level);
// default route of one hardswish depthwise layer (C % 16 == 0) of that backbone: true = the LDS-staged lcv3_dw2d_kernel (same table, same rule)
bool mbv3_dw2d_default(int k, int stride, int c, int level);
// Text-line direction classifier (ch_ptocr_mobile_v2.0_cls_mobile: MobileNetV3 small scale 0.35 with SE + ClsHead): ext[0] = x NCHW
// [B,3,H,W], ext[1] = softmax probabilities [B,2].  CLS_WANT_AUX: ext[2] = [B][2 logits | 200 pooled features].  CLS_WANT_STAGES
// (developer, rd_debug_cls_forward_stages): ext[3..6] = the outputs of blocks 0, 3, 8, 10 as NCHW
enum ClsFlags : int { CLS_WANT_AUX = 1, CLS_WANT_STAGES = 2 };
void build_ppocr_cls_mobile(Builder& b, int B, int H, int W, int flags);
// tensors build_ppocr_cls_mobile reads that are not in the file: every Conv + BatchNorm of the blocks and conv2 folded into weight + bias
void derive_ppocr_cls_mobile_weights(WeightStore& ws);
// the four map sizes CLS_WANT_STAGES hands out for an H x W input (rows; the width is (W - 1) / 2 + 1 for all), and whether every map of
// the graph down to the 2 x 2 pooling window is non-empty
bool cls_mobile_geometry(int H, int W, int rows[4], int* cols);
// default route of the classifier: true = cls_line_kernel (from the alternating A/B of tools/mb_cls_mobile.py at B = 6 and B = 1440,
// docs/notebook/cls_mobile.md); the route goes by the network, never by the batch
bool cls_fused_default();
// UniTable table-structure encoder (ViT-B: Conv2d(3, 768, 16, stride 16) patches + learned positions, 12 pre-norm encoder layers of 12 heads
// of 64 and FFN 3072 with erf GELU, final LayerNorm eps 1e-6): ext[0] = x NCHW [B,3,H,W] (H, W multiples of 16, T = HW / 256 <= 1024),
// ext[1] = memory [B,T,768].  VIT_WANT_TAPS (developer, rd_debug_table_encoder_taps): ext[2..4] = the patch embedding (before the
// position rows), the outputs of layers 0 and 11, each [B,T,768]
enum VitFlags : int { VIT_WANT_TAPS = 1 };
void build_unitable_encoder(Builder& b, int B, int H, int W, int flags);
// the tensor build_unitable_encoder reads that is not in the file: conv_proj's weight as a [768][768] matrix
void derive_unitable_encoder_weights(WeightStore& ws);
void build_pphgnetv2_b4(Builder& b, int B, int H, int W, int flags);   // (no plan variants: flags is ignored)
// PP-FormulaNet_plus encoder; flags bit 0: the caller's image has 1 channel (replicated to 3 like the reference)
void build_pphgnetv2_b6_formula(Builder& b, int B, int H, int W, int flags);

}  // namespace rd
