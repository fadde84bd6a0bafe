// What api.cpp (the product C surface) and api_debug.cpp (the developer entries) share: the handle, the guard that turns exceptions into
// return codes, and the decoders' internal interface (formula_decoder.hip, table_decoder.hip).  Not installed; include/rapiddoc_mi355.h is the contract.
#pragma once
#include "../../include/rapiddoc_mi355.h"

#include <string>

#include "engine.h"

namespace rd {
class FormulaDecoder;
FormulaDecoder* formula_decoder_create(int device, const void* blob, size_t nbytes);
void formula_decoder_destroy(FormulaDecoder* d);
int formula_decoder_decode(FormulaDecoder* d, const float* enc, int B, int S, int max_new, long long* ids, hipStream_t s, float* trace_logits,
                           float* trace_hidden);
// the decode through refilled slots (rd_formula_decode_stream); the traces (rd_debug_formula_decode_stream) may each be null
void formula_decoder_decode_stream(FormulaDecoder* d, const float* enc, int N, int S, int max_new, int slots, long long* ids, int* lens,
                                   rd_formula_stream_stats* stats, hipStream_t s, float* trace_logits, float* trace_hidden, int* trace_sched,
                                   int sched_steps);
int debug_dec_gemv(int M, int K, int N, int act, const float* x, const float* w, const float* bias, const float* ln_g, const float* ln_b,
                   const float* res, float* y);
int debug_dec_attention(int route, int self, int B, int T, float* kc, float* vc, int ldkv, long long seq_stride, const float* x, const float* ln_g,
                        const float* ln_b, const float* w, const float* bias, const float* q, int ldq, const float* kcur, const float* vcur,
                        int ldcur, float* out, int ldo);
int debug_dec_select(int mode, const float* logits, int V, int B, int step, long long* ids, int ids_ld, int* unfinished, int n_unfinished, int max_new,
                     const float* emb, const float* pos, const float* g, const float* b, float* x, int* state_out);
int formula_decoder_max_new(FormulaDecoder* d);
class TableDecoder;
TableDecoder* table_decoder_create(int device, const void* blob, size_t nbytes);
void table_decoder_destroy(TableDecoder* d);
int table_decoder_decode(TableDecoder* d, const float* memory, int B, int S, int max_new, const int* cfg6, long long* ids, int* n_tokens, hipStream_t s,
                         const int* forced, float* trace_hidden, float* trace_logits, int* trace_chosen, int* trace_emitted);
// the decode through refilled slots (rd_table_decode_stream); the traces (rd_debug_table_decode_stream) may each be null
void table_decoder_decode_stream(TableDecoder* d, const float* memory, int N, int S, int max_new, int slots, const int* cfg6, long long* ids, int* lens,
                                 rd_table_stream_stats* stats, hipStream_t s, float* trace_logits, float* trace_hidden, int* trace_sched,
                                 int sched_steps);
// one synchronised launch of a decode step's kernel on caller-provided buffers (rd_debug_td_*; table_decoder.hip)
int debug_td_gemv(int B, int K, int N, int act, const float* x, const float* w, const float* bias, const float* res, float* y);
int debug_td_attention(int stream_form, int self, int B, int T, float* kc, float* vc, int ldkv, long long seq_stride, const float* q, int ldq,
                       const float* kcur, const float* vcur, int ldcur, float* out, int ldo, const int* src, const int* pos);
int debug_td_select(int stream_form, const float* logits, int B, const int* cfg6, int max_new, long long* ids, int ids_ld, const float* emb,
                    const float* pos, float* x, int step, int* finished, int* boxcount, int* tok, const int* forced, int forced_ld, int* chosen,
                    const int* slot_src, int* slot_pos, int* slot_box, int* slot_done, int* lens);
}  // namespace rd

struct rd_handle {
    rd::Engine* eng = nullptr;           // convolutional networks (plan-based)
    rd::FormulaDecoder* dec = nullptr;   // "ppformulanet_head": autoregressive decoder
    rd::TableDecoder* tdec = nullptr;    // "unitable_decoder": autoregressive decoder
    int device = 0;
    std::string kind;
    std::string err;
    std::string prof;
};

template <typename F>
static int guarded(rd_handle* h, F&& f) {
    if (!h || (!h->eng && h->kind != "ppformulanet_head" && h->kind != "unitable_decoder")) return 2;
    try {
        f();
        h->err.clear();
        return 0;
    } catch (const std::exception& e) {
        h->err = e.what();
        return 1;
    }
}

static inline void table_cfg6(const rd_table_decode_cfg* cfg, int out[6]) {
    RD_CHECK(cfg, "cfg is NULL");
    out[0] = cfg->prefix_id; out[1] = cfg->eos_id; out[2] = cfg->pad_id; out[3] = cfg->bbox_close_id; out[4] = cfg->bbox_first_id; out[5] = cfg->bbox_last_id;
}
