// Checkbox detection on the device: rapid_doc/utils/checkbox_det_cls.py detect_checkboxes + the image work of classify_checkboxes
// (called at batch_analyze.py:207-219), page batch [P][H][W][3] u8 in HBM -> a few hundred bytes per candidate.  No weights.
//   cb_bin_kernel         grey <= 150 as ONE BIT per pixel: a wavefront's __ballot is one 64-pixel word.  The only pass over the
//                         3 B / pixel page; everything below works on H x ceil(W / 64) words.
//   cb_lines_kernel       MORPH_OPEN by 1 x 15 and by 15 x 1 as shift / AND / OR ladders on words, OR-ed.  The reference also ANDs each
//                         opening with the CLOSING by the same element; opening is anti-extensive and closing extensive, so
//                         open & close == open and the closings are not computed (tests/test_checkbox_host.py proves it on the literal
//                         restatement).  Erosion sees set pixels outside the image and in the unused bits of a row's last word,
//                         dilation clear ones.
//   cb_dilate3_kernel     the 3 x 3 dilation of the line mask (clear border)
//   cb_row_runs_kernel    per row the runs of the COMPLEMENT, counted, then written in raster order (cb_row_scan_kernel between)
//   cb_components_kernel  per page, one workgroup: union-find over row-adjacent runs (8-connectivity, the scheme of db_regions_kernel),
//                         per component the bounding box and the label-order key (checkbox_geom.h block_key); the component that is
//                         FIRST in label order is dropped as the reference's stats[2:] drops it; those that pass the size filter are
//                         the candidates
//   cb_offsets_kernel     where each page's candidates start in the batch's record list
//   cb_cand_kernel        per candidate, one workgroup: the ROI of the dilated mask (bit rows) and the whole tick chain in LDS (grey,
//                         5 x 5 fixed-point blur, 11 x 11 float32 mean, threshold, 3 x 3 open, count)
// A page with more runs than max_runs raises ITS overflow flag and yields nothing; the caller repeats it with the worst-case bound.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "checkbox_geom.h"
#include "rd_kernels.h"

namespace {

using u64 = unsigned long long;

struct CbRun { int16_t y, x0, x1, pad; };
struct CbStage { int32_t key; int16_t x, y, w, h; };

static_assert(sizeof(rd_checkbox_cand) == 24 + 8 * RD_CHECKBOX_ROI_ROWS && sizeof(rd_checkbox_page) == 32, "record layouts");
static_assert(RD_CHECKBOX_ROI_ROWS == rd_cb::kRoiMaxH && rd_cb::kRoiMaxW <= 64, "an ROI row is one word");

template <int NT>
__device__ int cb_block_exclusive_scan(int v, int* smem, int* total) {
    const int tid = threadIdx.x;
    smem[tid] = v;
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {
        const int t = tid >= off ? smem[tid - off] : 0;
        __syncthreads();
        smem[tid] += t;
        __syncthreads();
    }
    const int incl = smem[tid];
    *total = smem[NT - 1];
    __syncthreads();
    return incl - v;
}

// bits of the row's last word that are pixels
__device__ __forceinline__ u64 tail_mask(int W) { return (W & 63) ? ((1ull << (W & 63)) - 1) : ~0ull; }

// ---- page -> threshold bits
__global__ void __launch_bounds__(256) cb_bin_kernel(const uint8_t* __restrict__ pages, int H, int W, int WW, int bgr, u64* __restrict__ bin) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int y = blockIdx.y, p = blockIdx.z;
    if (j >= WW) return;                                     // uniform over the wavefront
    const int x = j * 64 + lane;
    bool on = false;
    if (x < W) {
        const uint8_t* px = pages + (((size_t)p * H + y) * W + x) * 3;
        const int c0 = px[0], c1 = px[1], c2 = px[2];
        on = rd_cb::grey_bgr(bgr ? c0 : c2, c1, bgr ? c2 : c0) <= rd_cb::kGreyThresh;
    }
    const u64 m = __ballot(on);
    if (lane == 0) bin[((size_t)p * H + y) * WW + j] = m;
}

// ---- the two openings
__global__ void __launch_bounds__(256) cb_lines_kernel(const u64* __restrict__ bin, int H, int W, int WW, u64* __restrict__ lines) {
    const int idx = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (idx >= H * WW) return;
    const int y = idx / WW, j = idx - y * WW;
    const u64* page = bin + (size_t)p * H * WW;
    const u64* row = page + (size_t)y * WW;
    const u64 tail = tail_mask(W);
    // horizontal: erosion (set outside), then dilation (clear outside) of the eroded words j - 1 .. j + 1
    auto ext = [&](int jj) -> u64 {
        if (jj < 0 || jj >= WW) return ~0ull;
        const u64 v = row[jj];
        return jj == WW - 1 ? v | ~tail : v;
    };
    auto eroded = [&](int jj) -> u64 {
        if (jj < 0 || jj >= WW) return 0ull;
        const u64 a = ext(jj - 1), b = ext(jj), c = ext(jj + 1);
        u64 e = b;
#pragma unroll
        for (int s = 1; s <= rd_cb::kLineHalf; ++s) e &= ((b >> s) | (c << (64 - s))) & ((b << s) | (a >> (64 - s)));
        return jj == WW - 1 ? e & tail : e;
    };
    const u64 ea = eroded(j - 1), eb = eroded(j), ec = eroded(j + 1);
    u64 oh = eb;
#pragma unroll
    for (int s = 1; s <= rd_cb::kLineHalf; ++s) oh |= ((eb >> s) | (ec << (64 - s))) | ((eb << s) | (ea >> (64 - s)));
    // vertical: rows y - 14 .. y + 14 of this word column; AND over windows of 15 by doubling (2, 4, 8, 15), then OR of the 15 windows
    // whose centre row lies inside the image
    u64 v[29];
#pragma unroll
    for (int k = 0; k < 29; ++k) {
        const int yy = y - 14 + k;
        v[k] = (yy >= 0 && yy < H) ? page[(size_t)yy * WW + j] : ~0ull;
    }
#pragma unroll
    for (int k = 0; k < 28; ++k) v[k] &= v[k + 1];           // windows of 2
#pragma unroll
    for (int k = 0; k < 26; ++k) v[k] &= v[k + 2];           // of 4
#pragma unroll
    for (int k = 0; k < 22; ++k) v[k] &= v[k + 4];           // of 8
    u64 ov = 0;
#pragma unroll
    for (int k = 0; k < 15; ++k) {                           // window [k, k + 14] = rows y - 14 + k .. y + k, centre y - 7 + k
        const int yc = y - 7 + k;
        if (yc >= 0 && yc < H) ov |= v[k] & v[k + 7];
    }
    u64 r = oh | ov;
    if (j == WW - 1) r &= tail;
    lines[(size_t)p * H * WW + idx] = r;
}

// ---- 3 x 3 dilation, clear border
__global__ void __launch_bounds__(256) cb_dilate3_kernel(const u64* __restrict__ lines, int H, int W, int WW, u64* __restrict__ fin) {
    const int idx = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (idx >= H * WW) return;
    const int y = idx / WW, j = idx - y * WW;
    const u64* page = lines + (size_t)p * H * WW;
    u64 r = 0;
    for (int yy = y - 1; yy <= y + 1; ++yy) {
        if (yy < 0 || yy >= H) continue;
        const u64* row = page + (size_t)yy * WW;
        const u64 a = j > 0 ? row[j - 1] : 0ull, b = row[j], c = j + 1 < WW ? row[j + 1] : 0ull;
        r |= b | (b << 1) | (a >> 63) | (b >> 1) | (c << 63);
    }
    if (j == WW - 1) r &= tail_mask(W);
    fin[(size_t)p * H * WW + idx] = r;
}

// ---- rows of the complement -> runs.  One workgroup per row, thread t owns word t (W <= 16384: at most 256 words).
template <bool WRITE>
__global__ void __launch_bounds__(256) cb_row_runs_kernel(const u64* __restrict__ fin, int H, int W, int WW, int32_t* __restrict__ row_cnt,
                                                          const int32_t* __restrict__ row_off, CbRun* __restrict__ runs, int max_runs) {
    __shared__ int scan[256];
    const int y = blockIdx.x, p = blockIdx.y, j = threadIdx.x;
    const u64* row = fin + ((size_t)p * H + y) * WW;
    const u64 tail = tail_mask(W);
    auto comp = [&](int jj) -> u64 {
        if (jj < 0 || jj >= WW) return 0ull;
        const u64 c = ~row[jj];
        return jj == WW - 1 ? c & tail : c;
    };
    const u64 cw = comp(j), prev63 = comp(j - 1) >> 63, next0 = comp(j + 1) & 1ull;
    u64 starts = cw & ~((cw << 1) | prev63);
    u64 ends = cw & ~((cw >> 1) | (next0 << 63));
    int total;
    const int before = cb_block_exclusive_scan<256>(__popcll(starts), scan, &total);
    if (!WRITE) {
        if (j == 0) row_cnt[(size_t)p * H + y] = total;
        return;
    }
    // the k-th start and the k-th end of a row belong to one run: ends before this word = starts before it, less the run that
    // crosses into it
    int slot_s = row_off[(size_t)p * (H + 1) + y] + before;
    int slot_e = slot_s - (int)(prev63 & cw & 1ull);
    CbRun* out = runs + (size_t)p * max_runs;
    while (starts) {
        const int b = __ffsll((long long)starts) - 1;
        starts &= starts - 1;
        if (slot_s < max_runs) { out[slot_s].y = (int16_t)y; out[slot_s].x0 = (int16_t)(j * 64 + b); out[slot_s].pad = 0; }
        ++slot_s;
    }
    while (ends) {
        const int b = __ffsll((long long)ends) - 1;
        ends &= ends - 1;
        if (slot_e < max_runs) out[slot_e].x1 = (int16_t)(j * 64 + b);
        ++slot_e;
    }
}

__global__ void __launch_bounds__(1024) cb_row_scan_kernel(const int32_t* __restrict__ row_cnt, int H, int32_t* __restrict__ row_off, int max_runs,
                                                           rd_checkbox_page* __restrict__ hdr) {
    __shared__ int smem[1024];
    const int p = blockIdx.x;
    int carry = 0;
    for (int y0 = 0; y0 < H; y0 += 1024) {
        const int y = y0 + threadIdx.x;
        const int v = y < H ? row_cnt[(size_t)p * H + y] : 0;
        int total;
        const int ex = cb_block_exclusive_scan<1024>(v, smem, &total);
        if (y < H) row_off[(size_t)p * (H + 1) + y] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        row_off[(size_t)p * (H + 1) + H] = carry;
        rd_checkbox_page h{};
        h.n_runs = carry;
        h.flags = carry > max_runs ? RD_CHECKBOX_RUNS_OVERFLOW : 0;
        h.first_key = -1;
        hdr[p] = h;
    }
}

// ---- runs -> components -> candidates
struct CompWs {
    const CbRun* runs; const int32_t* row_off;
    int32_t *parent, *key, *minx, *maxx, *miny, *maxy;      // [P][max_runs]; the last five hold a component's values at its ROOT run
    CbStage* stage;                                          // [P][max_cand]
    rd_checkbox_page* hdr;
    int max_runs, max_cand, H;
};

// Values that other wavefronts change with atomics (which execute in L2) are read with agent-scope atomic loads: a plain load may be
// served from a line the CU's vector L1 cached before the atomic.
__device__ __forceinline__ int cb_lda(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int cb_find(int32_t* parent, int i) {
    int p = cb_lda(&parent[i]);
    while (p != i) {
        i = p;
        p = cb_lda(&parent[i]);
    }
    return i;
}
__device__ __forceinline__ void cb_union(int32_t* parent, int a, int b) {
    // lock-free: link the larger root under the smaller one; a root only ever changes to a smaller index
    for (;;) {
        a = cb_find(parent, a);
        b = cb_find(parent, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&parent[b], a);
        if (old == b) return;
        b = old;
    }
}
// first run of [lo, hi) (one row: sorted, disjoint) whose x1 >= x
__device__ __forceinline__ int cb_first_run_reaching(const CbRun* runs, int lo, int hi, int x) {
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (runs[m].x1 < x) lo = m + 1;
        else hi = m;
    }
    return lo;
}

__global__ void __launch_bounds__(1024) cb_components_kernel(CompWs w) {
    __shared__ int smem[1024];
    __shared__ int s_first;
    const int p = blockIdx.x, tid = threadIdx.x;
    rd_checkbox_page* hdr = w.hdr + p;
    if (hdr->flags & RD_CHECKBOX_RUNS_OVERFLOW) return;      // n_comp = n_cand = 0 from the scan kernel; uniform over the workgroup
    const int n = hdr->n_runs;
    const CbRun* runs = w.runs + (size_t)p * w.max_runs;
    const int32_t* row_off = w.row_off + (size_t)p * (w.H + 1);
    const size_t base = (size_t)p * w.max_runs;
    int32_t *parent = w.parent + base, *key = w.key + base, *minx = w.minx + base, *maxx = w.maxx + base, *miny = w.miny + base, *maxy = w.maxy + base;
    for (int i = tid; i < n; i += 1024) {
        parent[i] = i; key[i] = 0x7fffffff; minx[i] = 32767; maxx[i] = -1; miny[i] = 32767; maxy[i] = -1;
    }
    if (tid == 0) s_first = 0x7fffffff;
    __syncthreads();
    // 1. union every run with the runs of the previous row it touches (columns may differ by one: 8-connectivity)
    for (int i = tid; i < n; i += 1024) {
        const CbRun r = runs[i];
        if (r.y == 0) continue;
        const int lo = row_off[r.y - 1], hi = row_off[r.y];
        for (int t = cb_first_run_reaching(runs, lo, hi, r.x0 - 1); t < hi && runs[t].x0 <= r.x1 + 1; ++t) cb_union(parent, t, i);
    }
    __syncthreads();
    // 2. flatten; 3. per component the box and the smallest block key (integer atomics: the result does not depend on the order)
    for (int i = tid; i < n; i += 1024) parent[i] = cb_find(parent, i);
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const CbRun r = runs[i];
        const int root = cb_lda(&parent[i]);
        const int k = rd_cb::block_key(r.x0, r.y);
        atomicMin(&minx[root], (int)r.x0);
        atomicMax(&maxx[root], (int)r.x1);
        atomicMin(&miny[root], (int)r.y);
        atomicMax(&maxy[root], (int)r.y);
        atomicMin(&key[root], k);
        atomicMin(&s_first, k);
    }
    __syncthreads();
    const int first = s_first;
    // 4. candidates in the order of their root runs (the host orders them by key)
    CbStage* stage = w.stage + (size_t)p * w.max_cand;
    int n_comp = 0, n_cand = 0;
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + tid;
        const int is_root = i < n && cb_lda(&parent[i]) == i;
        int is_cand = 0;
        CbStage st{};
        if (is_root) {
            const int x0 = cb_lda(&minx[i]), x1 = cb_lda(&maxx[i]), y0 = cb_lda(&miny[i]), y1 = cb_lda(&maxy[i]);
            st.key = cb_lda(&key[i]);
            st.x = (int16_t)x0; st.y = (int16_t)y0; st.w = (int16_t)(x1 - x0 + 1); st.h = (int16_t)(y1 - y0 + 1);
            is_cand = st.key != first && rd_cb::size_ok(st.w, st.h);
        }
        int total_r, total_c;
        (void)cb_block_exclusive_scan<1024>(is_root, smem, &total_r);
        const int ex = cb_block_exclusive_scan<1024>(is_cand, smem, &total_c);
        if (is_cand && n_cand + ex < w.max_cand) stage[n_cand + ex] = st;
        n_comp += total_r;
        n_cand += total_c;
    }
    if (tid == 0) {
        hdr->n_comp = n_comp;
        hdr->n_cand = n_cand;
        hdr->first_key = n ? first : -1;
        if (n_cand > w.max_cand) hdr->flags |= RD_CHECKBOX_CANDS_OVERFLOW;
    }
}

__global__ void __launch_bounds__(1024) cb_offsets_kernel(rd_checkbox_page* __restrict__ hdr, int P, int max_cand) {
    __shared__ int smem[1024];
    const int p = threadIdx.x;
    const int v = p < P ? min(hdr[p].n_cand, max_cand) : 0;
    int total;
    const int ex = cb_block_exclusive_scan<1024>(v, smem, &total);
    if (p < P) hdr[p].cand_off = ex;
}

// ---- one workgroup per candidate
constexpr int kSide = rd_cb::kMaxSide, kArea = kSide * kSide;

__global__ void __launch_bounds__(256) cb_cand_kernel(const uint8_t* __restrict__ pages, int H, int W, int WW, int bgr, const u64* __restrict__ fin,
                                                      const CbStage* __restrict__ stage, const rd_checkbox_page* __restrict__ hdr, int max_cand,
                                                      rd_checkbox_cand* __restrict__ out) {
    __shared__ uint8_t s_a[kArea], s_b[kArea], s_c[kArea];
    __shared__ float s_f[kArea];
    __shared__ int s_red[256];
    const int i = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const rd_checkbox_page h = hdr[p];
    if ((h.flags & RD_CHECKBOX_RUNS_OVERFLOW) || i >= min(h.n_cand, max_cand)) return;      // uniform over the workgroup
    const CbStage st = stage[(size_t)p * max_cand + i];
    rd_checkbox_cand* rec = out + h.cand_off + i;
    const int x = st.x, y = st.y, w = st.w, hh = st.h, n = w * hh;      // 12 <= w, hh <= 50 (size_ok)
    const rd_cb::Roi roi = rd_cb::roi_rect(x, y, w, hh, W, H);
    // the ROI of the dilated line mask, one word per row (at most 60 columns)
    if (tid < RD_CHECKBOX_ROI_ROWS) {
        u64 v = 0;
        if (tid < roi.h && roi.w > 0) {
            const u64* row = fin + ((size_t)p * H + roi.y + tid) * WW;
            const int j = roi.x >> 6, sh = roi.x & 63;
            v = row[j] >> sh;
            if (sh && j + 1 < WW) v |= row[j + 1] << (64 - sh);
            v &= (1ull << roi.w) - 1;
        }
        rec->roi[tid] = v;
    }
    if (tid == 0) {
        rec->key = st.key;
        rec->x = st.x; rec->y = st.y; rec->w = st.w; rec->h = st.h;
        rec->rx = (int16_t)roi.x; rec->ry = (int16_t)roi.y; rec->rw = (int16_t)roi.w; rec->rh = (int16_t)roi.h;
    }
    // the tick chain on image[y : y + h, x : x + w]
    const uint8_t* page = pages + (size_t)p * H * W * 3;
    for (int k = tid; k < n; k += 256) {                                   // grey -> s_a
        const int yy = k / w, xx = k - yy * w;
        const uint8_t* px = page + ((size_t)(y + yy) * W + (x + xx)) * 3;
        const int c0 = px[0], c1 = px[1], c2 = px[2];
        s_a[k] = (uint8_t)rd_cb::grey_bgr(bgr ? c0 : c2, c1, bgr ? c2 : c0);
    }
    __syncthreads();
    for (int k = tid; k < n; k += 256) {                                   // GaussianBlur 5 x 5, fixed point, reflect-101 -> s_b
        const int yy = k / w, xx = k - yy * w;
        const int kw[5] = {1, 4, 6, 4, 1};
        int S = 0;
#pragma unroll
        for (int dy = 0; dy < 5; ++dy) {
            const uint8_t* row = s_a + rd_cb::reflect101(yy + dy - 2, hh) * w;
            int r = 0;
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) r += kw[dx] * (int)row[rd_cb::reflect101(xx + dx - 2, w)];
            S += kw[dy] * r;
        }
        s_b[k] = (uint8_t)((S + 128) >> 8);
    }
    __syncthreads();
    for (int k = tid; k < n; k += 256) {                                   // the mean: rows -> s_f
        const int yy = k / w, xx = k - yy * w;
        float v[11];
#pragma unroll
        for (int t = 0; t < 11; ++t) v[t] = (float)s_b[yy * w + rd_cb::replicate(xx + t - 5, w)];
        s_f[k] = rd_cb::mean_taps(v);
    }
    __syncthreads();
    for (int k = tid; k < n; k += 256) {                                   // columns, round half-even, threshold -> s_a
        const int yy = k / w, xx = k - yy * w;
        float v[11];
#pragma unroll
        for (int t = 0; t < 11; ++t) v[t] = s_f[rd_cb::replicate(yy + t - 5, hh) * w + xx];
        int m = __float2int_rn(rd_cb::mean_taps(v));
        m = m < 0 ? 0 : (m > 255 ? 255 : m);
        s_a[k] = ((int)s_b[k] - m <= -2) ? 1 : 0;
    }
    __syncthreads();
    for (int k = tid; k < n; k += 256) {                                   // 3 x 3 erosion (set outside) -> s_c
        const int yy = k / w, xx = k - yy * w;
        int e = 1;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int y2 = yy + dy, x2 = xx + dx;
                if (y2 >= 0 && y2 < hh && x2 >= 0 && x2 < w) e &= s_a[y2 * w + x2];
            }
        s_c[k] = (uint8_t)e;
    }
    __syncthreads();
    int cnt = 0;
    for (int k = tid; k < n; k += 256) {                                   // 3 x 3 dilation (clear outside), counted
        const int yy = k / w, xx = k - yy * w;
        int d = 0;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int y2 = yy + dy, x2 = xx + dx;
                if (y2 >= 0 && y2 < hh && x2 >= 0 && x2 < w) d |= s_c[y2 * w + x2];
            }
        cnt += d;
    }
    s_red[tid] = cnt;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) s_red[tid] += s_red[tid + s];
        __syncthreads();
    }
    if (tid == 0) rec->tick = s_red[0];
}

struct CbWsLayout { size_t part[RD_CHECKBOX_WS_PARTS]; size_t total; };
CbWsLayout cb_ws_layout(int P, int H, int W, int max_runs, int max_cand) {
    CbWsLayout L{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~size_t(255); return o; };
    const size_t words = (size_t)P * H * ((W + 63) / 64) * 8;
    L.part[0] = take(words);                                 // bin
    L.part[1] = take(words);                                 // lines
    L.part[2] = take(words);                                 // the dilated line mask
    L.part[3] = take((size_t)P * H * 4);                     // row_cnt
    L.part[4] = take((size_t)P * (H + 1) * 4);               // row_off
    L.part[5] = take((size_t)P * max_runs * sizeof(CbRun));  // runs
    for (int k = 6; k < 12; ++k) L.part[k] = take((size_t)P * max_runs * 4);   // parent, key, minx, maxx, miny, maxy
    L.part[12] = take((size_t)P * max_cand * sizeof(CbStage));
    L.total = off;
    return L;
}

}  // namespace

namespace rd {

size_t checkbox_workspace_bytes(int P, int H, int W, int max_runs, int max_cand, size_t* offsets) {
    if (P < 1 || P > RD_CHECKBOX_MAX_PAGES || H < 1 || W < 1 || H > RD_CHECKBOX_MAX_SIDE || W > RD_CHECKBOX_MAX_SIDE || max_runs < 1 || max_cand < 1) return 0;
    const CbWsLayout L = cb_ws_layout(P, H, W, max_runs, max_cand);
    if (offsets)
        for (int k = 0; k < RD_CHECKBOX_WS_PARTS; ++k) offsets[k] = L.part[k];
    return L.total;
}

void launch_checkbox_bin(const uint8_t* pages, int P, int H, int W, int bgr, uint64_t* bin, hipStream_t s) {
    const int WW = (W + 63) / 64;
    hipLaunchKernelGGL(cb_bin_kernel, dim3((WW + 3) / 4, H, P), dim3(256), 0, s, pages, H, W, WW, bgr ? 1 : 0, reinterpret_cast<u64*>(bin));
}

int launch_checkbox_detect(int device, const uint8_t* pages, int P, int H, int W, int bgr, int max_runs, int max_cand, void* ws, size_t ws_bytes,
                           rd_checkbox_page* hdr, rd_checkbox_cand* cands, hipStream_t s, std::string& err) {
    const char* who = "rd_checkbox_detect_device: ";
    if (!pages || !ws || !hdr || !cands) { err = std::string(who) + "pages, workspace, page headers or candidate records are NULL"; return 1; }
    if (P < 1 || P > RD_CHECKBOX_MAX_PAGES) { err = std::string(who) + "P outside 1 .. " + std::to_string(RD_CHECKBOX_MAX_PAGES); return 1; }
    if (H < 1 || W < 1 || H > RD_CHECKBOX_MAX_SIDE || W > RD_CHECKBOX_MAX_SIDE) {
        err = std::string(who) + "H, W outside 1 .. " + std::to_string(RD_CHECKBOX_MAX_SIDE);
        return 1;
    }
    if (max_runs < 1 || max_cand < 1 || (long long)P * max_cand > 0x7fffffffLL) { err = std::string(who) + "max_runs / max_cand must be positive"; return 1; }
    const CbWsLayout L = cb_ws_layout(P, H, W, max_runs, max_cand);
    if (ws_bytes < L.total) { err = std::string(who) + "workspace holds " + std::to_string(ws_bytes) + " bytes, " + std::to_string(L.total) + " needed"; return 1; }
    hipError_t rc = hipSetDevice(device);
    if (rc != hipSuccess) { err = std::string(who) + "hipSetDevice: " + hipGetErrorString(rc); return 1; }
    uint8_t* base = static_cast<uint8_t*>(ws);
    const int WW = (W + 63) / 64;
    u64* bin = reinterpret_cast<u64*>(base + L.part[0]);
    u64* lines = reinterpret_cast<u64*>(base + L.part[1]);
    u64* fin = reinterpret_cast<u64*>(base + L.part[2]);
    int32_t* row_cnt = reinterpret_cast<int32_t*>(base + L.part[3]);
    int32_t* row_off = reinterpret_cast<int32_t*>(base + L.part[4]);
    CbRun* runs = reinterpret_cast<CbRun*>(base + L.part[5]);
    const unsigned word_blocks = (unsigned)(((size_t)H * WW + 255) / 256);
    launch_checkbox_bin(pages, P, H, W, bgr, reinterpret_cast<uint64_t*>(bin), s);
    hipLaunchKernelGGL(cb_lines_kernel, dim3(word_blocks, P), dim3(256), 0, s, bin, H, W, WW, lines);
    hipLaunchKernelGGL(cb_dilate3_kernel, dim3(word_blocks, P), dim3(256), 0, s, lines, H, W, WW, fin);
    hipLaunchKernelGGL(cb_row_runs_kernel<false>, dim3(H, P), dim3(256), 0, s, fin, H, W, WW, row_cnt, row_off, runs, max_runs);
    hipLaunchKernelGGL(cb_row_scan_kernel, dim3(P), dim3(1024), 0, s, row_cnt, H, row_off, max_runs, hdr);
    hipLaunchKernelGGL(cb_row_runs_kernel<true>, dim3(H, P), dim3(256), 0, s, fin, H, W, WW, row_cnt, row_off, runs, max_runs);
    CompWs w{};
    w.runs = runs; w.row_off = row_off;
    w.parent = reinterpret_cast<int32_t*>(base + L.part[6]);
    w.key = reinterpret_cast<int32_t*>(base + L.part[7]);
    w.minx = reinterpret_cast<int32_t*>(base + L.part[8]);
    w.maxx = reinterpret_cast<int32_t*>(base + L.part[9]);
    w.miny = reinterpret_cast<int32_t*>(base + L.part[10]);
    w.maxy = reinterpret_cast<int32_t*>(base + L.part[11]);
    w.stage = reinterpret_cast<CbStage*>(base + L.part[12]);
    w.hdr = hdr;
    w.max_runs = max_runs; w.max_cand = max_cand; w.H = H;
    hipLaunchKernelGGL(cb_components_kernel, dim3(P), dim3(1024), 0, s, w);
    hipLaunchKernelGGL(cb_offsets_kernel, dim3(1), dim3(1024), 0, s, hdr, P, max_cand);
    hipLaunchKernelGGL(cb_cand_kernel, dim3(max_cand, P), dim3(256), 0, s, pages, H, W, WW, bgr ? 1 : 0, fin, w.stage, hdr, max_cand, cands);
    rc = hipGetLastError();
    if (rc != hipSuccess) { err = std::string(who) + "kernel launch: " + hipGetErrorString(rc); return 1; }
    return 0;
}

}  // namespace rd
