// UniTable table-structure decoder (unitable_modules.py GPTFastDecoder + UniTableStructure.loop_decode): greedy autoregressive decode of B <= 8
// tables at once over the encoder's `memory`, D = 768, 12 heads of 64, FFN 3072, 4 pre-norm blocks, no final norm, generator 768 -> 960.
// Structure as formula_decoder.hip: the fused weights per load; K and V of `memory` for the 4 layers once per table batch (the fp32 MFMA
// GEMM at M = B S); per token step a chain of launches with constant arguments (the step index lives in device memory), captured once into
// a hipGraph and replayed; the host looks at the per-table EOS flags every 8 steps.
//   td_gemv_kernel    weight-streaming GEMV at M = B: one wavefront per output column streams its weight row once and serves all B rows;
//                     a (row, column) sum has the same order whatever B is
//   td_attn_kernel    one workgroup per (table, head): scores into LDS, max, exp, sum, P V; the self form appends the step's K / V row to
//                     the cache (1024 rows, fp32) and attends rows 0 .. step (the causal mask at input_pos)
//   td_select_kernel  whitelist argmax (ids 1 and 12 .. 509; every other id sits at -1e9; NaN counts as -inf; the lowest id wins among
//                     equals - so the winner is always an id below 960, and a row whose whitelisted logits are ALL NaN or -inf names
//                     id 0, outside the whitelist, because -1e9 beats -inf: tests/test_gpu_td_select.py pins both), the bbox rule
//                     (a counter per table that ONLY a bbox token raises and only its overflow clears), the per-table EOS latch (a
//                     finished table keeps its slot and writes `pad`), and the next step's embedding + position row
// No atomics: every table has its own flag, counter and token word.
// rd_table_decode_stream (decode_stream below) runs N tables through `slots` <= 8 rows of the same step: per-slot state in device memory (the
// table a slot holds, its position, its bbox counter), and a row whose table ended takes the next waiting table inside the captured step.
//   td_stream_attn_kernel / td_stream_select_kernel   td_attn_kernel / td_select_kernel reading the slot's state where those read `step`
//   td_stream_admit_kernel   one workgroup in td_advance_kernel's place: finished slots take the waiting tables in slot order, or go idle
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "engine.h"
#include "rd_device.h"

namespace rd {

namespace {
constexpr int TD_D = 768, TD_HEADS = 12, TD_HD = 64, TD_FFN = 3072, TD_LAYERS = 4, TD_VOCAB = 960, TD_MAXPOS = 1024, TD_MAXB = 8;
}

struct TdCfg { int prefix, eos, pad, close_id, bbox_lo, bbox_hi; };
struct TdState { int step; };

__device__ __forceinline__ bool td_whitelisted(int v) { return v == 1 || (v >= 12 && v <= 509); }

// x[b] = emb[tok] + pos[p]
__device__ __forceinline__ void td_embed_row(const float* emb, const float* pos, int tok, int p, float* x) {
    for (int c = threadIdx.x; c < TD_D; c += blockDim.x) x[c] = emb[(size_t)tok * TD_D + c] + pos[(size_t)p * TD_D + c];
}

__global__ void __launch_bounds__(256) td_init_kernel(TdState* st, int* finished, int* boxcount, int* tok, long long* ids, int ids_ld, TdCfg cfg,
                                                      const int* forced, int forced_ld, const float* emb, const float* pos, float* x) {
    const int b = blockIdx.x;
    const int t0 = min(max(forced ? forced[(size_t)b * forced_ld] : cfg.prefix, 0), TD_VOCAB - 1);     // (an embedding row: clamped as every later token)
    if (threadIdx.x == 0) {
        if (b == 0) st->step = 0;
        finished[b] = 0;
        boxcount[b] = 0;
        tok[b] = t0;
    }
    for (int c = threadIdx.x; c < ids_ld; c += blockDim.x) ids[(size_t)b * ids_ld + c] = c == 0 ? t0 : cfg.pad;
    td_embed_row(emb, pos, t0, 0, x + (size_t)b * TD_D);
}

__global__ void td_advance_kernel(TdState* st) { st->step += 1; }

__global__ void __launch_bounds__(256) td_trace_kernel(const float* src, float* dst, long long n, long long step_stride, const TdState* st) {
    float* d = dst + (size_t)st->step * step_stride;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) d[i] = src[i];
}

// y[b][n] = act(x[b] . w[n] + bias[n]) (+ res[b][n]); K % 256 == 0; grid N / 4, wavefront per column
__global__ void __launch_bounds__(256) td_gemv_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ res, float* __restrict__ y, int B, int K, int N, int act) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float acc[TD_MAXB];
#pragma unroll
    for (int b = 0; b < TD_MAXB; ++b) acc[b] = 0.f;
    const float* wr = w + (size_t)n * K;
    for (int k = 4 * lane; k < K; k += 256) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + k);
#pragma unroll
        for (int b = 0; b < TD_MAXB; ++b)
            if (b < B) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (size_t)b * K + k);
                acc[b] = fmaf(wv[0], xv[0], acc[b]);
                acc[b] = fmaf(wv[1], xv[1], acc[b]);
                acc[b] = fmaf(wv[2], xv[2], acc[b]);
                acc[b] = fmaf(wv[3], xv[3], acc[b]);
            }
    }
#pragma unroll
    for (int b = 0; b < TD_MAXB; ++b)
        if (b < B) {
            float v = acc[b];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) {
                v = rd_act(v + (bias ? bias[n] : 0.f), act);
                if (res) v += res[(size_t)b * N + n];
                y[(size_t)b * N + n] = v;
            }
        }
}

struct TdAttn {
    const float* q; int ldq;            // [B][ldq], head h at column 64 h
    float* kc; float* vc;               // rows [b * seq_stride + j * ldkv + 64 h]
    int ldkv; long long seq_stride;
    const float* kcur; const float* vcur; int ldcur;   // self form: the step's K / V rows (appended at row `step`), else null
    const TdState* st; int fixed_T;     // keys = fixed_T, or step + 1 in the self form
    float* out; int ldo;
};

__global__ void __launch_bounds__(256) td_attn_kernel(TdAttn p) {
    __shared__ float sc[TD_MAXPOS];
    __shared__ float qs[TD_HD];
    __shared__ float red[4];
    __shared__ float part[4][TD_HD];
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool self = p.kcur != nullptr;
    const int pos = self ? min(p.st->step, TD_MAXPOS - 1) : 0;
    const int T = self ? pos + 1 : p.fixed_T;
    float* kb = p.kc + (size_t)b * p.seq_stride + h * TD_HD;
    float* vb = p.vc + (size_t)b * p.seq_stride + h * TD_HD;
    const float* kcur = self ? p.kcur + (size_t)b * p.ldcur + h * TD_HD : nullptr;
    const float* vcur = self ? p.vcur + (size_t)b * p.ldcur + h * TD_HD : nullptr;
    if (tid < TD_HD) {
        qs[tid] = p.q[(size_t)b * p.ldq + h * TD_HD + tid] * 0.125f;
        if (self) {       // append to the cache; this launch reads the row from kcur / vcur, later steps from the cache
            kb[(size_t)pos * p.ldkv + tid] = kcur[tid];
            vb[(size_t)pos * p.ldkv + tid] = vcur[tid];
        }
    }
    __syncthreads();
    float m = -INFINITY;
    for (int j = tid; j < T; j += 256) {
        const float* kr = (self && j == pos) ? kcur : kb + (size_t)j * p.ldkv;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;      // four partial sums: one chain of 64 roundings put few-hot scores outside the fp64 bound
#pragma unroll
        for (int d = 0; d < TD_HD; d += 4) {
            const f32x4 kv = *reinterpret_cast<const f32x4*>(kr + d);
            s0 = fmaf(qs[d], kv[0], s0); s1 = fmaf(qs[d + 1], kv[1], s1); s2 = fmaf(qs[d + 2], kv[2], s2); s3 = fmaf(qs[d + 3], kv[3], s3);
        }
        const float s = (s0 + s1) + (s2 + s3);
        sc[j] = s;
        m = fmaxf(m, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float l = 0.f;
    for (int j = tid; j < T; j += 256) {
        const float e = expf(sc[j] - m);
        sc[j] = e;
        l += e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) l += __shfl_xor(l, o, 64);
    if (lane == 0) red[wave] = l;
    __syncthreads();
    l = (red[0] + red[1]) + (red[2] + red[3]);
    float acc = 0.f;
    for (int j = wave; j < T; j += 4) {
        const float* vr = (self && j == pos) ? vcur : vb + (size_t)j * p.ldkv;
        acc = fmaf(sc[j], vr[lane], acc);
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (tid < TD_HD) p.out[(size_t)b * p.ldo + h * TD_HD + tid] = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) / l;
}

struct TdSelect {
    const float* logits; long long* ids; int ids_ld; int* finished; int* boxcount; int* tok; const TdState* st; TdCfg cfg; int max_new;
    const int* forced; int forced_ld;          // developer: the tokens fed to steps 0 .. (the EOS latch is off)
    int* trace_chosen; int* trace_emitted; int B;
    const float* emb; const float* pos; float* x;
};

__global__ void __launch_bounds__(1024) td_select_kernel(TdSelect p) {
    __shared__ float bv[1024];
    __shared__ int bi[1024];
    __shared__ int next_tok;
    const int b = blockIdx.x, tid = threadIdx.x, step = p.st->step;
    float v = -INFINITY;
    if (tid < TD_VOCAB) {
        v = td_whitelisted(tid) ? p.logits[(size_t)b * TD_VOCAB + tid] : -1e9f;
        if (!(v == v)) v = -INFINITY;          // NaN never wins
    }
    bv[tid] = v;
    bi[tid] = tid < TD_VOCAB ? tid : TD_VOCAB - 1;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {        // the larger value, the lower id among equals
        if (tid < s) {
            const float a = bv[tid], c = bv[tid + s];
            if (c > a || (c == a && bi[tid + s] < bi[tid])) { bv[tid] = c; bi[tid] = bi[tid + s]; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int chosen = bi[0];
        int emitted = chosen;
        if (chosen >= p.cfg.bbox_lo && chosen <= p.cfg.bbox_hi) {
            int c = p.boxcount[b] + 1;
            if (c > 4) { emitted = p.cfg.close_id; c = 0; }
            p.boxcount[b] = c;
        }
        if (p.trace_chosen) p.trace_chosen[(size_t)step * p.B + b] = chosen;
        if (p.trace_emitted) p.trace_emitted[(size_t)step * p.B + b] = emitted;
        const bool was_done = p.finished[b] != 0;
        if (step + 1 < p.ids_ld) p.ids[(size_t)b * p.ids_ld + step + 1] = was_done ? p.cfg.pad : emitted;
        if (!p.forced && !was_done && emitted == p.cfg.eos) p.finished[b] = 1;
        int nt = (was_done || emitted == p.cfg.eos) ? p.cfg.eos : emitted;
        if (p.forced) nt = step + 1 < p.forced_ld ? p.forced[(size_t)b * p.forced_ld + step + 1] : p.cfg.eos;
        nt = min(max(nt, 0), TD_VOCAB - 1);
        p.tok[b] = nt;
        next_tok = nt;
    }
    __syncthreads();
    if (step + 1 < TD_MAXPOS) td_embed_row(p.emb, p.pos, next_tok, step + 1, p.x + (size_t)b * TD_D);
}

// ---- rd_table_decode_stream: the launches of a step that read per-row state.  Row b is a decode SLOT with a state of its own in device
// memory: the table it holds (src, -1 = idle), that table's position (pos = its cached length) and its bbox counter.  The kernels above keep
// their text (a body shared with them changed their generated code in the formula decoder: docs/notebook/formula_stream.md s2), so the
// three below are copies with the per-slot reads put in; layernorm768 and td_gemv_kernel run unchanged at M = slots (a row's sums never see
// another row, so an idle slot's row is computed, finite, and never looked at).
struct TdStream {          // written by one lane with plain stores; cross-block reads only across a kernel boundary
    int next;              // first table not yet admitted
    int n_live;            // slots that hold a table
    int steps;             // step launches so far
    int live_slot_steps;   // slot-steps that produced a token
    int src[TD_MAXB];      // table of the slot, -1 = idle
    int pos[TD_MAXB];      // tokens generated so far for that table
    int done[TD_MAXB];     // the select launch of this step ended the slot's table (cleared by the admission launch)
    int box[TD_MAXB];      // the bbox counter of the slot's table
};

// td_attn_kernel with b = the slot: the self cache is the slot's (rows 0 .. pos - 1 were all written by the table that holds the slot now:
// a refilled slot starts at length 0 and never reads its predecessor's rows), the cross K | V block is table src's.  An idle slot returns at once.
__global__ void __launch_bounds__(256) td_stream_attn_kernel(TdAttn p, const TdStream* ss) {
    __shared__ float sc[TD_MAXPOS];
    __shared__ float qs[TD_HD];
    __shared__ float red[4];
    __shared__ float part[4][TD_HD];
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int src = ss->src[b];
    if (src < 0) return;               // idle (uniform over the block)
    const bool self = p.kcur != nullptr;
    const int pos = self ? min(ss->pos[b], TD_MAXPOS - 1) : 0;
    const int T = self ? pos + 1 : p.fixed_T;
    const int blk = self ? b : src;    // the block of the K / V buffers this row reads (and, self, appends to)
    float* kb = p.kc + (size_t)blk * p.seq_stride + h * TD_HD;
    float* vb = p.vc + (size_t)blk * p.seq_stride + h * TD_HD;
    const float* kcur = self ? p.kcur + (size_t)b * p.ldcur + h * TD_HD : nullptr;
    const float* vcur = self ? p.vcur + (size_t)b * p.ldcur + h * TD_HD : nullptr;
    if (tid < TD_HD) {
        qs[tid] = p.q[(size_t)b * p.ldq + h * TD_HD + tid] * 0.125f;
        if (self) {
            kb[(size_t)pos * p.ldkv + tid] = kcur[tid];
            vb[(size_t)pos * p.ldkv + tid] = vcur[tid];
        }
    }
    __syncthreads();
    float m = -INFINITY;
    for (int j = tid; j < T; j += 256) {
        const float* kr = (self && j == pos) ? kcur : kb + (size_t)j * p.ldkv;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;      // four partial sums: one chain of 64 roundings put few-hot scores outside the fp64 bound
#pragma unroll
        for (int d = 0; d < TD_HD; d += 4) {
            const f32x4 kv = *reinterpret_cast<const f32x4*>(kr + d);
            s0 = fmaf(qs[d], kv[0], s0); s1 = fmaf(qs[d + 1], kv[1], s1); s2 = fmaf(qs[d + 2], kv[2], s2); s3 = fmaf(qs[d + 3], kv[3], s3);
        }
        const float s = (s0 + s1) + (s2 + s3);
        sc[j] = s;
        m = fmaxf(m, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float l = 0.f;
    for (int j = tid; j < T; j += 256) {
        const float e = expf(sc[j] - m);
        sc[j] = e;
        l += e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) l += __shfl_xor(l, o, 64);
    if (lane == 0) red[wave] = l;
    __syncthreads();
    l = (red[0] + red[1]) + (red[2] + red[3]);
    float acc = 0.f;
    for (int j = wave; j < T; j += 4) {
        const float* vr = (self && j == pos) ? vcur : vb + (size_t)j * p.ldkv;
        acc = fmaf(sc[j], vr[lane], acc);
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (tid < TD_HD) p.out[(size_t)b * p.ldo + h * TD_HD + tid] = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) / l;
}

struct TdStreamSelect {
    const float* logits; long long* ids; int ids_ld; int* lens; TdStream* ss; TdCfg cfg; int max_new;
    const float* emb; const float* pos; float* x;
};

// td_select_kernel's whitelist argmax and bbox rule for the slot's table: ids[src][pos + 1]; EOS or the table's last column ends it
// (lens[src], done[slot]); otherwise the position advances and the next step's input row is embedded.  Block `slot` is the only one that
// touches the slot's words in this launch.
__global__ void __launch_bounds__(1024) td_stream_select_kernel(TdStreamSelect p) {
    __shared__ float bv[1024];
    __shared__ int bi[1024];
    __shared__ int next_tok;
    const int slot = blockIdx.x, tid = threadIdx.x, src = p.ss->src[slot];
    if (src < 0) return;               // idle (uniform over the block)
    const int t = p.ss->pos[slot];
    float v = -INFINITY;
    if (tid < TD_VOCAB) {
        v = td_whitelisted(tid) ? p.logits[(size_t)slot * TD_VOCAB + tid] : -1e9f;
        if (!(v == v)) v = -INFINITY;          // NaN never wins
    }
    bv[tid] = v;
    bi[tid] = tid < TD_VOCAB ? tid : TD_VOCAB - 1;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {        // the larger value, the lower id among equals
        if (tid < s) {
            const float a = bv[tid], c = bv[tid + s];
            if (c > a || (c == a && bi[tid + s] < bi[tid])) { bv[tid] = c; bi[tid] = bi[tid + s]; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int chosen = bi[0];
        int emitted = chosen;
        if (chosen >= p.cfg.bbox_lo && chosen <= p.cfg.bbox_hi) {
            int c = p.ss->box[slot] + 1;
            if (c > 4) { emitted = p.cfg.close_id; c = 0; }
            p.ss->box[slot] = c;
        }
        p.ids[(size_t)src * p.ids_ld + t + 1] = emitted;
        const bool end = emitted == p.cfg.eos || t + 1 >= p.max_new;
        if (end) {
            p.lens[src] = t + 2;
            p.ss->done[slot] = 1;
        } else {
            p.ss->pos[slot] = t + 1;
        }
        next_tok = end ? -1 : min(max(emitted, 0), TD_VOCAB - 1);
    }
    __syncthreads();
    if (next_tok < 0) return;          // the admission launch behind this one writes the row of whatever takes the slot
    td_embed_row(p.emb, p.pos, next_tok, t + 1, p.x + (size_t)slot * TD_D);
}

// Admission, one workgroup, in the launch behind the select launch (the kernel boundary is what makes every select block's stores visible
// here).  In slot order every finished slot takes the first waiting table - position 0, bbox counter 0, input row = the prefix token's (x0) -
// or goes idle: which slot a table lands in follows from the lengths alone (tests/stream_reference.py).  An idle slot's input row is put
// back to x0 at every step, so the row the linears compute for it stays the same finite one however long the call runs.
__global__ void __launch_bounds__(256) td_stream_admit_kernel(TdStream* ss, int N, int slots, const float* x0, float* x) {
    __shared__ int reset[TD_MAXB];
    const int tid = threadIdx.x;
    if (tid == 0) {
        int next = ss->next, n_live = ss->n_live, live = 0;
        for (int s = 0; s < slots; ++s) {
            reset[s] = 1;
            if (ss->src[s] < 0) continue;
            ++live;
            if (!ss->done[s]) { reset[s] = 0; continue; }
            ss->done[s] = 0;
            ss->pos[s] = 0;
            ss->box[s] = 0;
            if (next < N) {
                ss->src[s] = next++;
            } else {
                ss->src[s] = -1;
                --n_live;
            }
        }
        ss->next = next;
        ss->n_live = n_live;
        ss->steps += 1;
        ss->live_slot_steps += live;
    }
    __syncthreads();
    for (int s = 0; s < slots; ++s)
        if (reset[s])
            for (int c = tid; c < TD_D; c += 256) x[(size_t)s * TD_D + c] = x0[c];
}

// Once per call: the state (tables 0 .. min(N, slots) - 1 sit in the slots of their number), ids = prefix | pad, and the prefix token's
// input row emb[prefix] + pos[0] into x0 and into every slot's row (block 0)
__global__ void __launch_bounds__(256) td_stream_init_kernel(TdStream* ss, long long* ids, int ids_ld, int N, int slots, TdCfg cfg, const float* emb,
                                                             const float* pos, float* x, float* x0) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int t0 = min(max(cfg.prefix, 0), TD_VOCAB - 1);
    if (i == 0) { ss->next = min(N, slots); ss->n_live = min(N, slots); ss->steps = 0; ss->live_slot_steps = 0; }
    if (i < TD_MAXB) { ss->src[i] = (i < slots && i < N) ? i : -1; ss->pos[i] = 0; ss->done[i] = 0; ss->box[i] = 0; }
    for (long long k = i; k < (long long)N * ids_ld; k += (long long)gridDim.x * blockDim.x) ids[k] = (k % ids_ld == 0) ? t0 : cfg.pad;
    if (blockIdx.x == 0)
        for (int r = 0; r <= slots; ++r) td_embed_row(emb, pos, t0, 0, r < slots ? x + (size_t)r * TD_D : x0);
}

// developer traces (rd_debug_table_decode_stream): dst[(src * max_new + pos) * row_ld + i] = src_rows[slot][i], i < n
__global__ void __launch_bounds__(256) td_stream_trace_kernel(const float* src_rows, float* dst, int n, long long row_ld, int max_new, const TdStream* ss) {
    const int slot = blockIdx.x, src = ss->src[slot];
    if (src < 0) return;
    float* d = dst + ((size_t)src * max_new + ss->pos[slot]) * row_ld;
    const float* r = src_rows + (size_t)slot * n;
    for (int i = threadIdx.x; i < n; i += 256) d[i] = r[i];
}
// sched [sched_steps][slots][2] = (src, pos) of every slot at the start of step ss->steps
__global__ void td_stream_sched_kernel(const TdStream* ss, int* sched, int sched_steps, int slots) {
    const int s = threadIdx.x, t = ss->steps;
    if (s >= slots || t >= sched_steps) return;
    sched[((size_t)t * slots + s) * 2] = ss->src[s];
    sched[((size_t)t * slots + s) * 2 + 1] = ss->pos[s];
}

// The launches of a step: decode(), decode_stream() and the developer entries rd_debug_td_* (below) all launch through these four.
// `ss` given = the stream form (per-slot state), null = the batch form (p.st).
static void launch_td_gemv(const float* x, const float* w, const float* bias, const float* res, float* y, int B, int K, int N, int act, hipStream_t s) {
    hipLaunchKernelGGL(td_gemv_kernel, dim3((N + 3) / 4), dim3(256), 0, s, x, w, bias, res, y, B, K, N, act);
}
static void launch_td_attention(const TdAttn& p, int B, const TdStream* ss, hipStream_t s) {
    if (ss) hipLaunchKernelGGL(td_stream_attn_kernel, dim3(TD_HEADS, B), dim3(256), 0, s, p, ss);
    else hipLaunchKernelGGL(td_attn_kernel, dim3(TD_HEADS, B), dim3(256), 0, s, p);
}
static void launch_td_select(const TdSelect& p, hipStream_t s) { hipLaunchKernelGGL(td_select_kernel, dim3(p.B), dim3(1024), 0, s, p); }
static void launch_td_stream_select(const TdStreamSelect& p, int slots, hipStream_t s) {
    hipLaunchKernelGGL(td_stream_select_kernel, dim3(slots), dim3(1024), 0, s, p);
}

// =================================================================================================
class TableDecoder {
   public:
    explicit TableDecoder(int device) : device_(device) {}
    ~TableDecoder() {
        (void)hipSetDevice(device_);
        if (buf_) (void)hipFree(buf_);
    }
    void load(const WeightStore& ws);
    int decode(const float* memory, int B, int S, int max_new, const TdCfg& cfg, long long* ids_out, int* n_tokens, hipStream_t s, const int* forced,
               float* trace_hidden, float* trace_logits, int* trace_chosen, int* trace_emitted);
    // memory [N,S,768] through `slots` refilled decode rows -> ids [N][max_new+1], lens [N] (device); stats (host) may be null.  Traces (each
    // may be null): logits [N][max_new][960], hidden [N][max_new][4][768], sched int [sched_steps][slots][2]
    void decode_stream(const float* memory, int N, int S, int max_new, int slots, const TdCfg& cfg, long long* ids_out, int* lens_out,
                       rd_table_stream_stats* stats, hipStream_t s, float* trace_logits, float* trace_hidden, int* trace_sched, int sched_steps);

   private:
    void gemm(const float* x, int M, int K, const std::string& key, int N, float* y, hipStream_t s);
    void gemv(const float* x, int B, int K, const std::string& key, int N, float* y, int act, const float* res, hipStream_t s) {
        launch_td_gemv(x, params_.ptr(key + "#w"), params_.ptr(key + "#b"), res, y, B, K, N, act, s);
    }
    void ln(const float* x, const std::string& key, float* y, int M, hipStream_t s) {
        launch_layernorm768(x, TD_D, y, TD_D, params_.ptr(key + ".weight"), params_.ptr(key + ".bias"), M, 1e-5f, s);
    }
    int device_;
    ParamBlock params_;
    uint8_t* buf_ = nullptr;
    size_t buf_bytes_ = 0;
};

static std::vector<float> td_vec(const HostTensor& t) { return std::vector<float>(t.f32(), t.f32() + t.numel()); }

void TableDecoder::load(const WeightStore& ws) {
    auto shape2 = [&](const std::string& n, int a, int b) {
        const HostTensor& t = ws.get(n);
        RD_CHECK(t.shape.size() == 2 && t.shape[0] == a && t.shape[1] == b, "table decoder: unexpected shape of " + n);
    };
    shape2("token_embed.embedding.weight", TD_VOCAB, TD_D);
    shape2("pos_embed.embedding.weight", TD_MAXPOS, TD_D);
    shape2("generator.weight", TD_VOCAB, TD_D);
    params_.add("emb", td_vec(ws.get("token_embed.embedding.weight")));
    params_.add("pos", td_vec(ws.get("pos_embed.embedding.weight")));
    auto lin = [&](const std::string& name, const std::string& key, int n, int k) {
        shape2(name + ".weight", n, k);
        params_.add(key + "#w", td_vec(ws.get(name + ".weight")));
        params_.add(key + "#b", td_vec(ws.get(name + ".bias")));
    };
    auto add_ln = [&](const std::string& name, const std::string& key) {
        params_.add(key + ".weight", td_vec(ws.get(name + ".weight")));
        params_.add(key + ".bias", td_vec(ws.get(name + ".bias")));
    };
    for (int l = 0; l < TD_LAYERS; ++l) {
        const std::string L = "layers." + std::to_string(l) + ".", K = "l" + std::to_string(l) + ".";
        add_ln(L + "norm1", K + "ln1");
        add_ln(L + "norm2", K + "ln2");
        add_ln(L + "norm3", K + "ln3");
        lin(L + "self_attn.wqkv", K + "qkv", 3 * TD_D, TD_D);
        lin(L + "self_attn.wo", K + "wo", TD_D, TD_D);
        lin(L + "multihead_attn.query", K + "cq", TD_D, TD_D);
        lin(L + "multihead_attn.key", K + "ck", TD_D, TD_D);
        lin(L + "multihead_attn.value", K + "cv", TD_D, TD_D);
        lin(L + "multihead_attn.out", K + "co", TD_D, TD_D);
        lin(L + "linear1", K + "fc1", TD_FFN, TD_D);
        lin(L + "linear2", K + "fc2", TD_D, TD_FFN);
    }
    lin("generator", "gen", TD_VOCAB, TD_D);
    params_.upload();
}

// y [M][N] = x [M][K] . W^T + b on the fp32 MFMA GEMM (the once-per-batch projections of `memory`)
void TableDecoder::gemm(const float* x, int M, int K, const std::string& key, int N, float* y, hipStream_t s) {
    ConvParams p{};
    p.x = x; p.xld = K; p.N = 1; p.H = 1; p.W = M; p.Cin = K;
    p.w = params_.ptr(key + "#w");
    p.bias = params_.ptr(key + "#b");
    p.y = y; p.yld = N; p.OH = 1; p.OW = M; p.Cout = N;
    p.KH = p.KW = p.SH = p.SW = 1;
    p.act = ACT_NONE; p.out_mode = OUT_NHWC;
    p.M = M; p.K = K; p.Ng = N;
    launch_conv_igemm(p, s);
}

int TableDecoder::decode(const float* memory, int B, int S, int max_new, const TdCfg& cfg, long long* ids_out, int* n_tokens, hipStream_t s,
                         const int* forced, float* trace_hidden, float* trace_logits, int* trace_chosen, int* trace_emitted) {
    RD_HIP(hipSetDevice(device_));
    RD_CHECK(memory && ids_out, "table decode: null input/output");
    RD_CHECK(B >= 1 && B <= TD_MAXB, "table decode: this build serves batches of 1 .. 8 tables; got B = " + std::to_string(B));
    RD_CHECK(S >= 1 && S <= TD_MAXPOS, "table decode: 1 <= S <= 1024 memory rows per table");
    RD_CHECK(max_new >= 1 && max_new <= TD_MAXPOS, "table decode: 1 <= max_new_tokens <= 1024");
    auto in_vocab = [](int v) { return v >= 0 && v < TD_VOCAB; };
    RD_CHECK(in_vocab(cfg.prefix) && in_vocab(cfg.eos) && in_vocab(cfg.close_id), "table decode: prefix, eos and close ids must lie in 0 .. 959");
    RD_CHECK(cfg.bbox_lo <= cfg.bbox_hi, "table decode: empty bbox id range");
    const int ids_ld = max_new + 1;
    auto al = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t f = sizeof(float);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al(bytes); return o; };
    const size_t o_state = take(sizeof(TdState)), o_fin = take(TD_MAXB * sizeof(int)), o_box = take(TD_MAXB * sizeof(int)), o_tok = take(TD_MAXB * sizeof(int));
    const size_t o_ck = take((size_t)TD_LAYERS * B * S * TD_D * f), o_cv = take((size_t)TD_LAYERS * B * S * TD_D * f);
    const size_t o_kc = take((size_t)TD_LAYERS * B * TD_MAXPOS * TD_D * f), o_vc = take((size_t)TD_LAYERS * B * TD_MAXPOS * TD_D * f);
    const size_t o_x = take((size_t)B * TD_D * f), o_x2 = take((size_t)B * TD_D * f), o_h = take((size_t)B * TD_D * f);
    const size_t o_qkv = take((size_t)B * 3 * TD_D * f), o_a = take((size_t)B * TD_D * f), o_f = take((size_t)B * TD_FFN * f);
    const size_t o_lg = take((size_t)B * TD_VOCAB * f);
    if (off > buf_bytes_) {
        RD_HIP(hipStreamSynchronize(s));
        if (buf_) RD_HIP(hipFree(buf_));
        buf_ = nullptr;
        buf_bytes_ = 0;
        RD_HIP(hipMalloc((void**)&buf_, off));
        buf_bytes_ = off;
    }
    TdState* st = reinterpret_cast<TdState*>(buf_ + o_state);
    int* fin = reinterpret_cast<int*>(buf_ + o_fin);
    int* box = reinterpret_cast<int*>(buf_ + o_box);
    int* tok = reinterpret_cast<int*>(buf_ + o_tok);
    float* ck = reinterpret_cast<float*>(buf_ + o_ck);
    float* cv = reinterpret_cast<float*>(buf_ + o_cv);
    float* kc = reinterpret_cast<float*>(buf_ + o_kc);
    float* vc = reinterpret_cast<float*>(buf_ + o_vc);
    float* x = reinterpret_cast<float*>(buf_ + o_x);
    float* x2 = reinterpret_cast<float*>(buf_ + o_x2);
    float* h = reinterpret_cast<float*>(buf_ + o_h);
    float* qkv = reinterpret_cast<float*>(buf_ + o_qkv);
    float* a = reinterpret_cast<float*>(buf_ + o_a);
    float* ff = reinterpret_cast<float*>(buf_ + o_f);
    float* lg = reinterpret_cast<float*>(buf_ + o_lg);
    const int forced_ld = max_new;

    hipLaunchKernelGGL(td_init_kernel, dim3(B), dim3(256), 0, s, st, fin, box, tok, ids_out, ids_ld, cfg, forced, forced_ld, params_.ptr("emb"),
                       params_.ptr("pos"), x);
    // once per table batch: every layer's cross-attention K and V of `memory`
    for (int l = 0; l < TD_LAYERS; ++l) {
        const std::string K = "l" + std::to_string(l) + ".";
        gemm(memory, B * S, TD_D, K + "ck", TD_D, ck + (size_t)l * B * S * TD_D, s);
        gemm(memory, B * S, TD_D, K + "cv", TD_D, cv + (size_t)l * B * S * TD_D, s);
    }
    auto enqueue_step = [&]() {
        float* cur = x;
        float* nxt = x2;
        for (int l = 0; l < TD_LAYERS; ++l) {
            const std::string K = "l" + std::to_string(l) + ".";
            ln(cur, K + "ln1", h, B, s);
            gemv(h, B, TD_D, K + "qkv", 3 * TD_D, qkv, ACT_NONE, nullptr, s);
            TdAttn sp{};
            sp.q = qkv; sp.ldq = 3 * TD_D;
            sp.kc = kc + (size_t)l * B * TD_MAXPOS * TD_D; sp.vc = vc + (size_t)l * B * TD_MAXPOS * TD_D; sp.ldkv = TD_D; sp.seq_stride = (long long)TD_MAXPOS * TD_D;
            sp.kcur = qkv + TD_D; sp.vcur = qkv + 2 * TD_D; sp.ldcur = 3 * TD_D;
            sp.st = st; sp.fixed_T = 0; sp.out = a; sp.ldo = TD_D;
            launch_td_attention(sp, B, nullptr, s);
            gemv(a, B, TD_D, K + "wo", TD_D, nxt, ACT_NONE, cur, s);
            std::swap(cur, nxt);
            ln(cur, K + "ln2", h, B, s);
            gemv(h, B, TD_D, K + "cq", TD_D, qkv, ACT_NONE, nullptr, s);
            TdAttn cp{};
            cp.q = qkv; cp.ldq = TD_D;
            cp.kc = ck + (size_t)l * B * S * TD_D; cp.vc = cv + (size_t)l * B * S * TD_D; cp.ldkv = TD_D; cp.seq_stride = (long long)S * TD_D;
            cp.st = st; cp.fixed_T = S; cp.out = a; cp.ldo = TD_D;
            launch_td_attention(cp, B, nullptr, s);
            gemv(a, B, TD_D, K + "co", TD_D, nxt, ACT_NONE, cur, s);
            std::swap(cur, nxt);
            ln(cur, K + "ln3", h, B, s);
            gemv(h, B, TD_D, K + "fc1", TD_FFN, ff, ACT_GELU, nullptr, s);
            gemv(ff, B, TD_FFN, K + "fc2", TD_D, nxt, ACT_NONE, cur, s);
            std::swap(cur, nxt);
            if (trace_hidden)
                hipLaunchKernelGGL(td_trace_kernel, dim3(8), dim3(256), 0, s, cur, trace_hidden + (size_t)l * B * TD_D, (long long)B * TD_D,
                                   (long long)TD_LAYERS * B * TD_D, st);
        }
        gemv(cur, B, TD_D, "gen", TD_VOCAB, lg, ACT_NONE, nullptr, s);
        if (trace_logits) hipLaunchKernelGGL(td_trace_kernel, dim3(8), dim3(256), 0, s, lg, trace_logits, (long long)B * TD_VOCAB, (long long)B * TD_VOCAB, st);
        RD_CHECK(cur == x, "table decode: the layer stack must end in the buffer the next embedding is written to");
        TdSelect sel{lg, ids_out, ids_ld, fin, box, tok, st, cfg, max_new, forced, forced_ld, trace_chosen, trace_emitted, B, params_.ptr("emb"),
                     params_.ptr("pos"), x};
        launch_td_select(sel, s);
        hipLaunchKernelGGL(td_advance_kernel, dim3(1), dim3(1), 0, s, st);
    };
    struct StepGraph {          // the captured step; freed on every way out of this function, a throwing RD_HIP included
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        hipStream_t stream = nullptr;
        ~StepGraph() {
            if (exec) {
                (void)hipStreamSynchronize(stream);
                (void)hipGraphExecDestroy(exec);
            }
            if (graph) (void)hipGraphDestroy(graph);
        }
    } sg;
    sg.stream = s;
    if (max_new > 2 && s != nullptr) {          // (the null stream cannot be captured: direct launches there)
        if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            enqueue_step();
            if (hipStreamEndCapture(s, &sg.graph) != hipSuccess || hipGraphInstantiate(&sg.exec, sg.graph, nullptr, nullptr, 0) != hipSuccess) {
                if (sg.graph) (void)hipGraphDestroy(sg.graph);
                sg.graph = nullptr;
                sg.exec = nullptr;
                (void)hipGetLastError();
            }
        } else {
            (void)hipGetLastError();
        }
    }
    int hfin[TD_MAXB] = {0};
    for (int t = 0; t < max_new; ++t) {
        if (sg.exec) RD_HIP(hipGraphLaunch(sg.exec, s));
        else enqueue_step();
        if (!forced && ((t & 7) == 7 || t + 1 == max_new)) {      // all tables ended? (every 8 steps: one small D2H + sync)
            RD_HIP(hipMemcpyAsync(hfin, fin, sizeof(hfin), hipMemcpyDeviceToHost, s));
            RD_HIP(hipStreamSynchronize(s));
            bool all = true;
            for (int b = 0; b < B; ++b) all = all && hfin[b] != 0;
            if (all) break;
        }
    }
    RD_HIP(hipStreamSynchronize(s));
    RD_HIP(hipGetLastError());
    if (n_tokens) {       // tokens of every table, the prefix and its EOS included (max_new + 1 where it never stopped)
        std::vector<long long> ids((size_t)B * ids_ld);
        RD_HIP(hipMemcpy(ids.data(), ids_out, ids.size() * sizeof(long long), hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b) {
            int n = ids_ld;
            for (int c = 1; c < ids_ld; ++c)
                if (ids[(size_t)b * ids_ld + c] == cfg.eos) { n = c + 1; break; }
            n_tokens[b] = n;
        }
    }
    return 0;
}

// rd_table_decode_stream.  decode() above is batch-synchronous: the tables of a batch share one step counter and the loop runs until the
// longest table has ended, so on a page batch of mixed lengths most slot-steps write `pad`.  Here the step is the same launch sequence at
// M = slots, but every row carries its own (table, position, bbox counter) in device memory (TdStream) and a one-workgroup admission launch
// at the end of the captured step hands a finished row the next waiting table.  The host only replays the graph and looks at the state
// every 8 steps.
void TableDecoder::decode_stream(const float* memory, int N, int S, int max_new, int slots, const TdCfg& cfg, long long* ids_out, int* lens_out,
                                 rd_table_stream_stats* stats, hipStream_t s, float* trace_logits, float* trace_hidden, int* trace_sched,
                                 int sched_steps) {
    // refusals first: nothing is launched and the outputs stay as they are
    RD_CHECK(slots >= 1 && slots <= RD_TABLE_STREAM_MAX_SLOTS,
             "table decode stream: slots must be 1 .. " + std::to_string(RD_TABLE_STREAM_MAX_SLOTS) + " (RD_TABLE_STREAM_MAX_SLOTS), got " + std::to_string(slots));
    RD_CHECK(N >= 1, "table decode stream: N must be at least 1, got " + std::to_string(N));
    RD_CHECK(S >= 1 && S <= TD_MAXPOS, "table decode stream: 1 <= S <= 1024 memory rows per table, got " + std::to_string(S));
    RD_CHECK(max_new >= 1 && max_new <= TD_MAXPOS, "table decode stream: 1 <= max_new_tokens <= 1024, got " + std::to_string(max_new));
    RD_CHECK((long long)N * S <= RD_TABLE_STREAM_MAX_TOKENS, "table decode stream: N * S = " + std::to_string((long long)N * S) +
                                                                 " memory rows exceed RD_TABLE_STREAM_MAX_TOKENS (" +
                                                                 std::to_string(RD_TABLE_STREAM_MAX_TOKENS) + "): decode in windows");
    auto in_vocab = [](int v) { return v >= 0 && v < TD_VOCAB; };
    RD_CHECK(in_vocab(cfg.prefix) && in_vocab(cfg.eos) && in_vocab(cfg.close_id), "table decode stream: prefix, eos and close ids must lie in 0 .. 959");
    RD_CHECK(cfg.bbox_lo <= cfg.bbox_hi, "table decode stream: empty bbox id range");
    RD_CHECK(memory && ids_out && lens_out, "table decode stream: null input/output");
    RD_CHECK(!trace_sched || sched_steps > 0, "table decode stream: trace_sched needs sched_steps > 0");
    static_assert(RD_TABLE_STREAM_MAX_SLOTS == TD_MAXB, "a slot is a row of td_gemv_kernel");
    RD_HIP(hipSetDevice(device_));
    const int ids_ld = max_new + 1, M = slots, Tc = max_new;      // Tc: rows of a slot's self cache (positions 0 .. max_new - 1)
    auto al = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t f = sizeof(float);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al(bytes); return o; };
    const size_t o_state = take(sizeof(TdStream));
    const size_t o_ck = take((size_t)TD_LAYERS * N * S * TD_D * f), o_cv = take((size_t)TD_LAYERS * N * S * TD_D * f);          // [layer][N][S][768]
    const size_t o_kc = take((size_t)TD_LAYERS * M * Tc * TD_D * f), o_vc = take((size_t)TD_LAYERS * M * Tc * TD_D * f);        // [layer][slots][Tc][768]
    const size_t o_x0 = take((size_t)TD_D * f);
    const size_t o_act = off;                                       // the step's activations: cleared once, so that an idle row reads nothing uninitialised
    const size_t o_x = take((size_t)M * TD_D * f), o_x2 = take((size_t)M * TD_D * f), o_h = take((size_t)M * TD_D * f);
    const size_t o_qkv = take((size_t)M * 3 * TD_D * f), o_a = take((size_t)M * TD_D * f), o_f = take((size_t)M * TD_FFN * f);
    const size_t o_lg = take((size_t)M * TD_VOCAB * f);
    if (off > buf_bytes_) {
        RD_HIP(hipStreamSynchronize(s));
        if (buf_) RD_HIP(hipFree(buf_));
        buf_ = nullptr;
        buf_bytes_ = 0;
        RD_HIP(hipMalloc((void**)&buf_, off));
        buf_bytes_ = off;
    }
    TdStream* ss = reinterpret_cast<TdStream*>(buf_ + o_state);
    float* ck = reinterpret_cast<float*>(buf_ + o_ck);
    float* cv = reinterpret_cast<float*>(buf_ + o_cv);
    float* kc = reinterpret_cast<float*>(buf_ + o_kc);
    float* vc = reinterpret_cast<float*>(buf_ + o_vc);
    float* x0 = reinterpret_cast<float*>(buf_ + o_x0);
    float* x = reinterpret_cast<float*>(buf_ + o_x);
    float* x2 = reinterpret_cast<float*>(buf_ + o_x2);
    float* h = reinterpret_cast<float*>(buf_ + o_h);
    float* qkv = reinterpret_cast<float*>(buf_ + o_qkv);
    float* a = reinterpret_cast<float*>(buf_ + o_a);
    float* ff = reinterpret_cast<float*>(buf_ + o_f);
    float* lg = reinterpret_cast<float*>(buf_ + o_lg);

    RD_HIP(hipMemsetAsync(buf_ + o_act, 0, off - o_act, s));
    hipLaunchKernelGGL(td_stream_init_kernel, dim3(64), dim3(256), 0, s, ss, ids_out, ids_ld, N, slots, cfg, params_.ptr("emb"), params_.ptr("pos"), x, x0);
    // once per call: every layer's cross-attention K and V of all N tables, in consecutive groups of `slots` tables at the M decode() uses
    // for such a batch: a table's K | V have the bits rd_table_decode gives them in a batch of `slots` and do not depend on N
    for (int g0 = 0; g0 < N; g0 += slots) {
        const int rows = std::min(slots, N - g0) * S;
        const float* mem_g = memory + (size_t)g0 * S * TD_D;
        for (int l = 0; l < TD_LAYERS; ++l) {
            const std::string K = "l" + std::to_string(l) + ".";
            gemm(mem_g, rows, TD_D, K + "ck", TD_D, ck + ((size_t)l * N + g0) * S * TD_D, s);
            gemm(mem_g, rows, TD_D, K + "cv", TD_D, cv + ((size_t)l * N + g0) * S * TD_D, s);
        }
    }
    const TdStreamSelect sel{lg, ids_out, ids_ld, lens_out, ss, cfg, max_new, params_.ptr("emb"), params_.ptr("pos"), x};
    auto enqueue_step = [&]() {          // decode()'s chain at B = slots
        if (trace_sched) hipLaunchKernelGGL(td_stream_sched_kernel, dim3(1), dim3(64), 0, s, ss, trace_sched, sched_steps, slots);
        float* cur = x;
        float* nxt = x2;
        for (int l = 0; l < TD_LAYERS; ++l) {
            const std::string K = "l" + std::to_string(l) + ".";
            ln(cur, K + "ln1", h, M, s);
            gemv(h, M, TD_D, K + "qkv", 3 * TD_D, qkv, ACT_NONE, nullptr, s);
            TdAttn sp{};
            sp.q = qkv; sp.ldq = 3 * TD_D;
            sp.kc = kc + (size_t)l * M * Tc * TD_D; sp.vc = vc + (size_t)l * M * Tc * TD_D; sp.ldkv = TD_D; sp.seq_stride = (long long)Tc * TD_D;
            sp.kcur = qkv + TD_D; sp.vcur = qkv + 2 * TD_D; sp.ldcur = 3 * TD_D;
            sp.st = nullptr; sp.fixed_T = 0; sp.out = a; sp.ldo = TD_D;
            launch_td_attention(sp, M, ss, s);
            gemv(a, M, TD_D, K + "wo", TD_D, nxt, ACT_NONE, cur, s);
            std::swap(cur, nxt);
            ln(cur, K + "ln2", h, M, s);
            gemv(h, M, TD_D, K + "cq", TD_D, qkv, ACT_NONE, nullptr, s);
            TdAttn cp{};
            cp.q = qkv; cp.ldq = TD_D;
            cp.kc = ck + (size_t)l * N * S * TD_D; cp.vc = cv + (size_t)l * N * S * TD_D; cp.ldkv = TD_D; cp.seq_stride = (long long)S * TD_D;
            cp.st = nullptr; cp.fixed_T = S; cp.out = a; cp.ldo = TD_D;
            launch_td_attention(cp, M, ss, s);
            gemv(a, M, TD_D, K + "co", TD_D, nxt, ACT_NONE, cur, s);
            std::swap(cur, nxt);
            ln(cur, K + "ln3", h, M, s);
            gemv(h, M, TD_D, K + "fc1", TD_FFN, ff, ACT_GELU, nullptr, s);
            gemv(ff, M, TD_FFN, K + "fc2", TD_D, nxt, ACT_NONE, cur, s);
            std::swap(cur, nxt);
            if (trace_hidden)
                hipLaunchKernelGGL(td_stream_trace_kernel, dim3(M), dim3(256), 0, s, cur, trace_hidden + (size_t)l * TD_D, TD_D,
                                   (long long)TD_LAYERS * TD_D, max_new, ss);
        }
        gemv(cur, M, TD_D, "gen", TD_VOCAB, lg, ACT_NONE, nullptr, s);
        if (trace_logits) hipLaunchKernelGGL(td_stream_trace_kernel, dim3(M), dim3(256), 0, s, lg, trace_logits, TD_VOCAB, (long long)TD_VOCAB, max_new, ss);
        RD_CHECK(cur == x, "table decode stream: the layer stack must end in the buffer the next embedding is written to");
        launch_td_stream_select(sel, M, s);
        hipLaunchKernelGGL(td_stream_admit_kernel, dim3(1), dim3(256), 0, s, ss, N, slots, x0, x);
    };
    struct StepGraph {          // the captured step; freed on every way out of this function, a throwing RD_HIP included
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        hipStream_t stream = nullptr;
        ~StepGraph() {
            if (exec) {
                (void)hipStreamSynchronize(stream);
                (void)hipGraphExecDestroy(exec);
            }
            if (graph) (void)hipGraphDestroy(graph);
        }
    } sg;
    sg.stream = s;
    if (s != nullptr) {          // one stream, no branches (the null stream cannot be captured: direct launches there)
        if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            enqueue_step();
            if (hipStreamEndCapture(s, &sg.graph) != hipSuccess || hipGraphInstantiate(&sg.exec, sg.graph, nullptr, nullptr, 0) != hipSuccess) {
                if (sg.graph) (void)hipGraphDestroy(sg.graph);
                sg.graph = nullptr;
                sg.exec = nullptr;
                (void)hipGetLastError();
            }
        } else {
            (void)hipGetLastError();
        }
    }
    // every live slot advances by one token per step and a table ends after max_new at the latest: N * max_new steps would decode the tables
    // one after the other in a single slot.  The cap keeps a fault in the admission from spinning this loop
    const long long cap = (long long)N * max_new + 8;
    TdStream hs{};
    bool ended = false;
    for (long long t = 0; t < cap && !ended; ++t) {
        if (sg.exec) RD_HIP(hipGraphLaunch(sg.exec, s));
        else enqueue_step();
        if ((t & 7) == 7) {        // one small D2H + sync every 8 steps
            RD_HIP(hipMemcpyAsync(&hs, ss, sizeof(TdStream), hipMemcpyDeviceToHost, s));
            RD_HIP(hipStreamSynchronize(s));
            ended = hs.next >= N && hs.n_live == 0;
        }
    }
    RD_HIP(hipStreamSynchronize(s));
    RD_HIP(hipGetLastError());
    RD_CHECK(ended, "table decode stream: the device state never reported the end of the queue");
    if (stats) *stats = rd_table_stream_stats{hs.steps, hs.live_slot_steps, slots, hs.next};
}

TableDecoder* table_decoder_create(int device, const void* blob, size_t nbytes) {
    RD_HIP(hipSetDevice(device));
    WeightStore ws;
    ws.load_safetensors(blob, nbytes);
    auto* d = new TableDecoder(device);
    try {
        d->load(ws);
    } catch (...) {
        delete d;
        throw;
    }
    return d;
}
void table_decoder_destroy(TableDecoder* d) { delete d; }
int table_decoder_decode(TableDecoder* d, const float* memory, int B, int S, int max_new, const int* cfg6, long long* ids, int* n_tokens, hipStream_t s,
                         const int* forced, float* trace_hidden, float* trace_logits, int* trace_chosen, int* trace_emitted) {
    TdCfg c{cfg6[0], cfg6[1], cfg6[2], cfg6[3], cfg6[4], cfg6[5]};
    return d->decode(memory, B, S, max_new, c, ids, n_tokens, s, forced, trace_hidden, trace_logits, trace_chosen, trace_emitted);
}
void table_decoder_decode_stream(TableDecoder* d, const float* memory, int N, int S, int max_new, int slots, const int* cfg6, long long* ids, int* lens,
                                 rd_table_stream_stats* stats, hipStream_t s, float* trace_logits, float* trace_hidden, int* trace_sched,
                                 int sched_steps) {
    TdCfg c{cfg6[0], cfg6[1], cfg6[2], cfg6[3], cfg6[4], cfg6[5]};
    d->decode_stream(memory, N, S, max_new, slots, c, ids, lens, stats, s, trace_logits, trace_hidden, trace_sched, sched_steps);
}

// ---- developer entries (api_debug.cpp rd_debug_td_*): ONE synchronised launch of a step's kernel through the launch functions above, on
// caller-provided device buffers; no weight file.  0 = launched and synchronised; -1 = arguments the launch cannot take (nothing launched,
// the outputs untouched) or a HIP error.  The state words (step, per-slot src / pos / box / done, finished, boxcount, tok) are HOST arrays:
// the entry puts them into device state of its own and copies them back out behind the launch.
namespace {
bool td_debug_sync() { return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess; }
struct TdDebugBuf {      // `bytes` of device memory of the entry's own: a copy of `host`, or zeros
    void* d = nullptr;
    size_t bytes;
    TdDebugBuf(size_t n, const void* host) : bytes(n) {
        if (hipMalloc(&d, bytes) != hipSuccess) { d = nullptr; return; }
        if ((host ? hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) : hipMemset(d, 0, bytes)) != hipSuccess) { (void)hipFree(d); d = nullptr; }
    }
    ~TdDebugBuf() { if (d) (void)hipFree(d); }
    bool read(void* host) const { return hipMemcpy(host, d, bytes, hipMemcpyDeviceToHost) == hipSuccess; }
    template <class T> T* as() const { return static_cast<T*>(d); }
};
}  // namespace

// y [B][N] = act(x [B][K] w [N][K]^T + bias) + res [B][N] by td_gemv_kernel; bias and res may be null
int debug_td_gemv(int B, int K, int N, int act, const float* x, const float* w, const float* bias, const float* res, float* y) {
    if (B < 1 || B > TD_MAXB || K <= 0 || K % 256 != 0 || N <= 0 || !x || !w || !y || act < ACT_NONE || act > ACT_HSIG_PADDLE) return -1;
    launch_td_gemv(x, w, bias, res, y, B, K, N, act, nullptr);
    return td_debug_sync() ? 0 : -1;
}

// td_attn_kernel (stream_form 0) or td_stream_attn_kernel (1) over B rows.  Batch form: self != 0: the step is T, rows 0 .. T - 1 of
// the cache are read and this step's kcur / vcur appended as row T (T in 0 .. 1023); self == 0: T keys (1 .. 1024).  Stream form: src [B] and
// pos [B] (host int32) are the slots' tables (-1 = idle) and positions; self: row b's cache block is b and its step pos[b]; cross: T keys of
// block src[b] - kc / vc must hold max(src) + 1 blocks.  seq_stride must cover the rows a sequence reads and appends.
int debug_td_attention(int stream_form, int self, int B, int T, float* kc, float* vc, int ldkv, long long seq_stride, const float* q, int ldq,
                       const float* kcur, const float* vcur, int ldcur, float* out, int ldo, const int* src, const int* pos) {
    if (B < 1 || B > TD_MAXB || !kc || !vc || !q || !out || ldkv < TD_D || (ldkv & 3) || (seq_stride & 3) || ldq < TD_D || ldo < TD_D) return -1;
    if (self && (!kcur || !vcur || ldcur < TD_D || (ldcur & 3))) return -1;
    if (stream_form && (!src || !pos)) return -1;
    int rows = 0;          // cache rows of a sequence that the launch reads or appends
    if (!self) {
        if (T < 1 || T > TD_MAXPOS) return -1;
        rows = T;
    } else if (!stream_form) {
        if (T < 0 || T >= TD_MAXPOS) return -1;
        rows = T + 1;
    }
    TdStream hs{};
    for (int b = 0; b < TD_MAXB; ++b) hs.src[b] = -1;
    if (stream_form)
        for (int b = 0; b < B; ++b) {
            if (src[b] < -1 || pos[b] < 0 || pos[b] >= TD_MAXPOS) return -1;
            hs.src[b] = src[b];
            hs.pos[b] = pos[b];
            if (self && src[b] >= 0) rows = std::max(rows, pos[b] + 1);
        }
    if (seq_stride < (long long)rows * ldkv) return -1;
    const TdState hst{self ? T : 0};
    TdDebugBuf st(sizeof(TdState), &hst), ss(sizeof(TdStream), &hs);
    if (!st.d || !ss.d) return -1;
    TdAttn p{};
    p.q = q; p.ldq = ldq; p.kc = kc; p.vc = vc; p.ldkv = ldkv; p.seq_stride = seq_stride;
    if (self) { p.kcur = kcur; p.vcur = vcur; p.ldcur = ldcur; }
    p.st = stream_form ? nullptr : st.as<TdState>(); p.fixed_T = self ? 0 : T; p.out = out; p.ldo = ldo;
    launch_td_attention(p, B, stream_form ? ss.as<TdStream>() : nullptr, nullptr);
    return td_debug_sync() ? 0 : -1;
}

// td_select_kernel (stream_form 0) or td_stream_select_kernel (1) over B rows of logits [B][960] (device).  Device: ids [.][ids_ld], emb
// [960][768], pos [1024][768], x [B][768], lens (stream form: one word per table).  Host, int32, in and out: batch form finished / boxcount /
// tok [B], forced [B][forced_ld] or null (in only), chosen [B] or null (out only: the whitelist argmax in front of the bbox rule); stream form
// slot_src (in only) / slot_pos / slot_box / slot_done [B].
int debug_td_select(int stream_form, const float* logits, int B, const int* cfg6, int max_new, long long* ids, int ids_ld, const float* emb,
                    const float* pos, float* x, int step, int* finished, int* boxcount, int* tok, const int* forced, int forced_ld, int* chosen,
                    const int* slot_src, int* slot_pos, int* slot_box, int* slot_done, int* lens) {
    if (B < 1 || B > TD_MAXB || !logits || !cfg6 || max_new < 1 || max_new > TD_MAXPOS || !ids || ids_ld < 1 || !emb || !pos || !x) return -1;
    const TdCfg cfg{cfg6[0], cfg6[1], cfg6[2], cfg6[3], cfg6[4], cfg6[5]};
    const size_t words = (size_t)B * sizeof(int);
    if (!stream_form) {
        if (step < 0 || step >= TD_MAXPOS || !finished || !boxcount || !tok || (forced && forced_ld < 1)) return -1;
        const TdState hst{step};
        TdDebugBuf st(sizeof(TdState), &hst), fin(words, finished), box(words, boxcount), tk(words, tok);
        TdDebugBuf fo(forced ? words * forced_ld : sizeof(int), forced), ch(words * (step + 1), nullptr);
        if (!st.d || !fin.d || !box.d || !tk.d || !fo.d || !ch.d) return -1;
        const TdSelect sel{logits, ids, ids_ld, fin.as<int>(), box.as<int>(), tk.as<int>(), st.as<TdState>(), cfg, max_new,
                           forced ? fo.as<int>() : nullptr, forced_ld, ch.as<int>(), nullptr, B, emb, pos, x};
        launch_td_select(sel, nullptr);
        if (!td_debug_sync() || !fin.read(finished) || !box.read(boxcount) || !tk.read(tok)) return -1;
        if (chosen && hipMemcpy(chosen, ch.as<int>() + (size_t)step * B, words, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        return 0;
    }
    if (!slot_src || !slot_pos || !slot_box || !slot_done || !lens) return -1;
    TdStream hs{};
    for (int b = 0; b < TD_MAXB; ++b) hs.src[b] = -1;
    for (int b = 0; b < B; ++b) {          // a live slot writes ids[src][pos + 1]
        if (slot_src[b] < -1 || slot_pos[b] < 0 || (slot_src[b] >= 0 && slot_pos[b] + 1 >= ids_ld)) return -1;
        hs.src[b] = slot_src[b]; hs.pos[b] = slot_pos[b]; hs.box[b] = slot_box[b]; hs.done[b] = slot_done[b];
    }
    TdDebugBuf ss(sizeof(TdStream), &hs);
    if (!ss.d) return -1;
    const TdStreamSelect sel{logits, ids, ids_ld, lens, ss.as<TdStream>(), cfg, max_new, emb, pos, x};
    launch_td_stream_select(sel, B, nullptr);
    if (!td_debug_sync() || !ss.read(&hs)) return -1;
    for (int b = 0; b < B; ++b) { slot_pos[b] = hs.pos[b]; slot_box[b] = hs.box[b]; slot_done[b] = hs.done[b]; }
    return 0;
}

}  // namespace rd
