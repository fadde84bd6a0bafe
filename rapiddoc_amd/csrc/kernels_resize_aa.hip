// Pillow's antialiased bilinear resample (Image.resize(size, BILINEAR) on an 8-bit image: what torchvision's transforms.Resize runs on
// a PIL image) followed by torchvision's ToTensor + Normalize: rd_preproc_resize_aa_norm (include/rapiddoc_mi355.h).
//
// The arithmetic is Pillow's (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc /
// Vertical_8bpc): per axis a table of 22-bit fixed-point triangle weights whose support grows with the shrink factor, computed on the
// HOST in double in Pillow's operation order; a horizontal pass into a uint8 intermediate [H][OW][3], then a vertical pass over it.  The
// device does integer arithmetic only: acc = 2^21 + sum(pixel * coeff) in int32, clamp(acc >> 22, 0, 255).  A pass whose input and output
// sizes are equal does not run.  The vertical kernel also normalises, ((float(u8) / 255) - mean[c]) / std[c] in fp32 with IEEE division
// in that order, and writes CHW.
//
// Launch shape: every thread owns four neighbouring output pixels of one row (12 bytes).  With the row pitch a multiple of 4 bytes and
// aligned bases the vertical kernel reads 3 dwords per tap and writes one float4 per colour plane, the horizontal kernel stores 3
// dwords; otherwise the same kernels move bytes (template VEC).  The horizontal pass only computes the rows the vertical pass reads.  No
// atomics, no LDS.  Tables: cached per (in, out) per device, uploaded once with hipMemcpyAsync on the caller's stream (a later call on
// another stream waits for the upload's event); the intermediate is kept per (device, stream) and grows on demand.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/rapiddoc_mi355.h"
#include "rd_kernels.h"

namespace rd {

// ---------------------------------------------------------------------------------------------------------------- host: the tables
// bounds [out][2] = (first source index, taps); kk [out][ksize] = int(w * 2^22 +- 0.5).  Returns ksize.  Pillow's precompute_coeffs +
// normalize_coeffs_8bpc for one axis: `filter` RD_RESAMPLE_BILINEAR (triangle, support 1) or RD_RESAMPLE_BICUBIC (a = -0.5, support 2), sampled
// over the box [box0, box1) of the `in` source pixels (Pillow hands the box over as float32: the caller rounds it).
static inline double resample_filter(int filter, double x) {
#pragma clang fp contract(off)
    if (x < 0.0) x = -x;
    if (filter == RD_RESAMPLE_BICUBIC) {
        const double a = -0.5;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
        if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
        return 0.0;
    }
    return x < 1.0 ? 1.0 - x : 0.0;
}

int resample_coeffs(int filter, int in, double box0, double box1, int out, std::vector<int32_t>& bounds, std::vector<int32_t>& kk) {
#pragma clang fp contract(off)
    const double scale = (box1 - box0) / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = (filter == RD_RESAMPLE_BICUBIC ? 2.0 : 1.0) * fs;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    const double ss = 1.0 / fs;
    bounds.assign((size_t)out * 2, 0);
    kk.assign((size_t)out * ksize, 0);
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < out; ++xx) {
        const double center = box0 + (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        if (xmax < 0) xmax = 0;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            const double v = resample_filter(filter, (x + xmin - center + 0.5) * ss);
            w[x] = v;
            ww += v;
        }
        for (int x = 0; x < xmax; ++x) {
            double v = w[x];
            if (ww != 0.0) v /= ww;
            kk[(size_t)xx * ksize + x] = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << 22)) : (int32_t)(0.5 + v * (double)(1 << 22));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return ksize;
}

// the bilinear tables of a full box: what rd_preproc_resize_aa_norm uploads
int resize_aa_coeffs(int in, int out, std::vector<int32_t>& bounds, std::vector<int32_t>& kk) {
    return resample_coeffs(RD_RESAMPLE_BILINEAR, in, 0.0, (double)in, out, bounds, kk);
}

// ---------------------------------------------------------------------------------------------------------------- device
struct AaTable {
    const int32_t* bounds;   // [out][2]
    const int32_t* kk;       // [out][ksize]
    int ksize;
};

__device__ __forceinline__ int aa_clip8(int acc) {
    const int v = acc >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// src [rows][W][3] -> tmp [rows][OW][3], rows y0 .. y1 - 1 only.  Thread = (row, four output pixels).
template <bool VEC>
__global__ void __launch_bounds__(256) resize_aa_h_kernel(const uint8_t* __restrict__ src, int W, int OW, int y0, int y1, AaTable t,
                                                          uint8_t* __restrict__ tmp) {
    const int groups = (OW + 3) >> 2;
    const long total = (long)(y1 - y0) * groups;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int y = y0 + (int)(i / groups), ox0 = (int)(i % groups) * 4;
        const uint8_t* row = src + (size_t)y * W * 3;
        uint32_t pk[3] = {0u, 0u, 0u};
        const int n = OW - ox0 < 4 ? OW - ox0 : 4;
        for (int p = 0; p < n; ++p) {
            const int ox = ox0 + p;
            const int xmin = t.bounds[2 * ox], cnt = t.bounds[2 * ox + 1];
            const int32_t* k = t.kk + (size_t)ox * t.ksize;
            const uint8_t* q = row + (size_t)xmin * 3;
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
            for (int x = 0; x < cnt; ++x) {
                const int c = k[x];
                a0 += (int)q[3 * x] * c;
                a1 += (int)q[3 * x + 1] * c;
                a2 += (int)q[3 * x + 2] * c;
            }
            const int v[3] = {aa_clip8(a0), aa_clip8(a1), aa_clip8(a2)};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int b = p * 3 + c;
                pk[b >> 2] |= (uint32_t)v[c] << (8 * (b & 3));
            }
        }
        uint8_t* o = tmp + ((size_t)y * OW + ox0) * 3;
        if (VEC) {                                           // OW % 4 == 0 and tmp 4-byte aligned: n == 4, o 4-byte aligned
            uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
            o4[0] = pk[0]; o4[1] = pk[1]; o4[2] = pk[2];
        } else {
            for (int b = 0; b < n * 3; ++b) o[b] = (uint8_t)(pk[b >> 2] >> (8 * (b & 3)));
        }
    }
}

struct AaNorm {
    float mean[3], std[3];
};

// in [IH][OW][3] (the intermediate, or the source where the horizontal pass did not run) -> out_f [3][OH][OW] normalised, out_u8
// [OH][OW][3] (may be null).  has_v == 0: IH == OH and the rows pass through.  swap: channel c of the output is channel 2 - c of `in`.
template <bool VEC>
__global__ void __launch_bounds__(256) resize_aa_v_norm_kernel(const uint8_t* __restrict__ in, int OH, int OW, AaTable t, int has_v, int swap,
                                                               AaNorm nm, float* __restrict__ out_f, uint8_t* __restrict__ out_u8) {
    const int groups = (OW + 3) >> 2;
    const long total = (long)OH * groups;
    const size_t pitch = (size_t)OW * 3;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int oy = (int)(i / groups), ox0 = (int)(i % groups) * 4;
        const int n = OW - ox0 < 4 ? OW - ox0 : 4;
        const int ymin = has_v ? t.bounds[2 * oy] : oy, cnt = has_v ? t.bounds[2 * oy + 1] : 1;
        const int32_t* k = t.kk + (size_t)oy * t.ksize;
        int acc[12];
#pragma unroll
        for (int b = 0; b < 12; ++b) acc[b] = has_v ? (1 << 21) : 0;
        const uint8_t* q = in + (size_t)ymin * pitch + (size_t)ox0 * 3;
        for (int y = 0; y < cnt; ++y, q += pitch) {
            const int c = has_v ? k[y] : 1;
            if (VEC) {
                const uint32_t* q4 = reinterpret_cast<const uint32_t*>(q);
                const uint32_t w0 = q4[0], w1 = q4[1], w2 = q4[2];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    acc[b] += (int)((w0 >> (8 * b)) & 255u) * c;
                    acc[4 + b] += (int)((w1 >> (8 * b)) & 255u) * c;
                    acc[8 + b] += (int)((w2 >> (8 * b)) & 255u) * c;
                }
            } else {
#pragma unroll
                for (int b = 0; b < 12; ++b)
                    if (b < n * 3) acc[b] += (int)q[b] * c;
            }
        }
        int v[12];
#pragma unroll
        for (int b = 0; b < 12; ++b) v[b] = has_v ? aa_clip8(acc[b]) : acc[b];
        if (swap) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int s = v[3 * p];
                v[3 * p] = v[3 * p + 2];
                v[3 * p + 2] = s;
            }
        }
        float f[12];
#pragma unroll
        for (int b = 0; b < 12; ++b) f[b] = (((float)v[b] / 255.0f) - nm.mean[b % 3]) / nm.std[b % 3];
        const size_t plane = (size_t)OH * OW, at = (size_t)oy * OW + ox0;
        if (VEC) {
#pragma unroll
            for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(out_f + c * plane + at) = make_float4(f[c], f[3 + c], f[6 + c], f[9 + c]);
            if (out_u8) {
                uint32_t* o4 = reinterpret_cast<uint32_t*>(out_u8 + at * 3);
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    o4[j] = (uint32_t)v[4 * j] | ((uint32_t)v[4 * j + 1] << 8) | ((uint32_t)v[4 * j + 2] << 16) | ((uint32_t)v[4 * j + 3] << 24);
            }
        } else {
#pragma unroll
            for (int b = 0; b < 12; ++b)
                if (b < n * 3) {
                    out_f[(b % 3) * plane + at + b / 3] = f[b];
                    if (out_u8) out_u8[at * 3 + b] = (uint8_t)v[b];
                }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host: caches, launch
namespace {
struct TableEntry {
    std::vector<int32_t> host;          // bounds | kk: outlives the asynchronous upload
    int32_t* dev = nullptr;
    int ksize = 0, out = 0;
    hipEvent_t uploaded = nullptr;
    hipStream_t stream = nullptr;
    AaTable view() const { return AaTable{dev, dev + (size_t)out * 2, ksize}; }
};
struct Scratch {
    uint8_t* p = nullptr;
    size_t bytes = 0;
};
std::mutex g_mu;
std::map<std::tuple<int, int, int>, std::unique_ptr<TableEntry>> g_tables;       // (device, in, out)
std::map<std::pair<int, hipStream_t>, Scratch> g_scratch;                        // (device, stream)
constexpr size_t kMaxTables = 512;

const char* hip_err(hipError_t e, const char* what, std::string& err, const char* who = "rd_preproc_resize_aa_norm") {
    err = std::string(who) + ": " + what + ": " + hipGetErrorString(e);
    return err.c_str();
}

// Called once per launch BEFORE its lookups (a launch holds at most two tables): a full cache is emptied.  hipFree waits for the device,
// so nothing in flight reads a freed table.
void evict_if_full() {
    if (g_tables.size() + 2 <= kMaxTables) return;
    for (auto& kv : g_tables) {
        (void)hipFree(kv.second->dev);
        (void)hipEventDestroy(kv.second->uploaded);
    }
    g_tables.clear();
}

// the table of one axis on the device, uploaded in stream order on first use
TableEntry* table_for(int device, int in, int out, hipStream_t s, std::string& err) {
    auto key = std::make_tuple(device, in, out);
    auto it = g_tables.find(key);
    if (it == g_tables.end()) {
        auto e = std::make_unique<TableEntry>();
        std::vector<int32_t> bounds, kk;
        e->ksize = resize_aa_coeffs(in, out, bounds, kk);
        e->out = out;
        e->host = std::move(bounds);
        e->host.insert(e->host.end(), kk.begin(), kk.end());
        const size_t bytes = e->host.size() * sizeof(int32_t);
        hipError_t rc = hipMalloc((void**)&e->dev, bytes);
        if (rc != hipSuccess) { hip_err(rc, "hipMalloc of a coefficient table", err); return nullptr; }
        rc = hipMemcpyAsync(e->dev, e->host.data(), bytes, hipMemcpyHostToDevice, s);
        if (rc == hipSuccess) rc = hipEventCreateWithFlags(&e->uploaded, hipEventDisableTiming);
        if (rc == hipSuccess) rc = hipEventRecord(e->uploaded, s);
        if (rc != hipSuccess) {
            (void)hipFree(e->dev);
            hip_err(rc, "upload of a coefficient table", err);
            return nullptr;
        }
        e->stream = s;
        it = g_tables.emplace(key, std::move(e)).first;
    } else if (it->second->stream != s) {
        hipError_t rc = hipStreamWaitEvent(s, it->second->uploaded, 0);
        if (rc != hipSuccess) { hip_err(rc, "hipStreamWaitEvent", err); return nullptr; }
    }
    return it->second.get();
}

inline unsigned aa_grid(long threads) {
    long b = (threads + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}
inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }
}  // namespace

// 0 on success; otherwise `err` holds the message and NOTHING was launched by the failing step.
int launch_resize_aa_norm(int device, const uint8_t* src, int H, int W, int OH, int OW, const float mean[3], const float std[3], int swap_rb,
                          float* out, uint8_t* out_u8, hipStream_t s, std::string& err) {
    if (H < 1 || W < 1 || OH < 1 || OW < 1 || H > RD_RESIZE_AA_MAX_SIDE || W > RD_RESIZE_AA_MAX_SIDE || OH > RD_RESIZE_AA_MAX_SIDE ||
        OW > RD_RESIZE_AA_MAX_SIDE) {
        err = "rd_preproc_resize_aa_norm: H, W, OH, OW must lie in 1 .. " + std::to_string(RD_RESIZE_AA_MAX_SIDE) + ", got " + std::to_string(H) +
              " x " + std::to_string(W) + " -> " + std::to_string(OH) + " x " + std::to_string(OW);
        return 1;
    }
    if (!src || !out) { err = "rd_preproc_resize_aa_norm: null input / output pointer"; return 1; }
    hipError_t rc = hipSetDevice(device);
    if (rc != hipSuccess) { hip_err(rc, "hipSetDevice", err); return 1; }
    std::lock_guard<std::mutex> lock(g_mu);
    const bool has_h = W != OW, has_v = H != OH;
    evict_if_full();
    TableEntry *th = nullptr, *tv = nullptr;
    if (has_h && !(th = table_for(device, W, OW, s, err))) return 1;
    if (has_v && !(tv = table_for(device, H, OH, s, err))) return 1;
    int y0 = 0, y1 = H;                                      // the rows the vertical pass reads
    if (has_v) {
        const int32_t* b = tv->host.data();
        y0 = b[0];
        y1 = b[2 * (OH - 1)] + b[2 * (OH - 1) + 1];
    }
    const uint8_t* vin = src;
    if (has_h) {
        Scratch& sc = g_scratch[{device, s}];
        const size_t need = (size_t)H * OW * 3;
        if (sc.bytes < need) {
            if (sc.p) (void)hipFree(sc.p);                   // waits for the device: no earlier launch still writes it
            sc.p = nullptr;
            sc.bytes = 0;
            rc = hipMalloc((void**)&sc.p, need);
            if (rc != hipSuccess) { hip_err(rc, "hipMalloc of the intermediate", err); return 1; }
            sc.bytes = need;
        }
        const long threads = (long)(y1 - y0) * ((OW + 3) / 4);
        if (OW % 4 == 0 && aligned(sc.p, 4))
            hipLaunchKernelGGL(resize_aa_h_kernel<true>, dim3(aa_grid(threads)), dim3(256), 0, s, src, W, OW, y0, y1, th->view(), sc.p);
        else
            hipLaunchKernelGGL(resize_aa_h_kernel<false>, dim3(aa_grid(threads)), dim3(256), 0, s, src, W, OW, y0, y1, th->view(), sc.p);
        vin = sc.p;
    }
    AaNorm nm;
    for (int c = 0; c < 3; ++c) { nm.mean[c] = mean ? mean[c] : 0.f; nm.std[c] = std ? std[c] : 1.f; }
    const AaTable vt = has_v ? tv->view() : AaTable{nullptr, nullptr, 0};
    const long threads = (long)OH * ((OW + 3) / 4);
    const bool vec = OW % 4 == 0 && aligned(vin, 4) && aligned(out, 16) && (!out_u8 || aligned(out_u8, 4));
    if (vec)
        hipLaunchKernelGGL(resize_aa_v_norm_kernel<true>, dim3(aa_grid(threads)), dim3(256), 0, s, vin, OH, OW, vt, has_v ? 1 : 0, swap_rb ? 1 : 0, nm,
                           out, out_u8);
    else
        hipLaunchKernelGGL(resize_aa_v_norm_kernel<false>, dim3(aa_grid(threads)), dim3(256), 0, s, vin, OH, OW, vt, has_v ? 1 : 0, swap_rb ? 1 : 0, nm,
                           out, out_u8);
    rc = hipGetLastError();
    if (rc != hipSuccess) { hip_err(rc, "kernel launch", err); return 1; }
    return 0;
}

// ================================================================================================ the formula pre-process
// rd_formula_margin_boxes / rd_formula_preproc_plan / rd_formula_preproc_batch (include/rapiddoc_mi355.h): UniMERNetImgDecode +
// UniMERNetTestTransform + LatexImageFormat of PP-FormulaNet_plus with Pillow's integer arithmetic.  Per crop: the margin box (one
// workgroup, LDS reductions), then on the box Image.resize(BILINEAR) = the two passes above with a row pitch (the source is a window of
// a page), Image.thumbnail = reduce + the bicubic passes over a float32 box, and one final kernel that runs the last vertical pass (or a
// copy), pastes into the 384 x 384 canvas and writes the grey network input.  One thread per output pixel and byte accesses throughout:
// bases and pitches of page windows are not 4-byte aligned.  Intermediates and the batch's coefficient tables: the (device, stream)
// scratch of rd_preproc_resize_aa_norm, library-owned and grown on demand.
constexpr int kFS = RD_FORMULA_SIDE;

__device__ __forceinline__ int pil_grey(const uint8_t* p) {           // Pillow's convert("L")
    return (19595 * (int)p[0] + 38470 * (int)p[1] + 7471 * (int)p[2] + 0x8000) >> 16;
}

// One workgroup per crop, two scans: min / max of the grey level, then the bounding box of the pixels under the threshold.  A wavefront
// covers one row per step (a crop narrower than 64 pixels: 64 / w rows).  boxes [n][4] = (x0, y0, x1, y1), x1 / y1 exclusive.
__global__ void __launch_bounds__(256) formula_margin_kernel(const rd_formula_crop* __restrict__ descs, int32_t* __restrict__ boxes) {
    __shared__ int red[4][256];
    const rd_formula_crop d = descs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t* box = boxes + 4 * (size_t)blockIdx.x;
    if (d.w < 1 || d.h < 1) {                                 // uniform over the workgroup
        if (tid < 4) box[tid] = 0;
        return;
    }
    const int rpw = d.w >= 64 ? 1 : 64 / d.w;
    const int sub = d.w >= 64 ? 0 : lane / d.w, col0 = lane - sub * d.w;
    const int ystart = sub < rpw ? wave * rpw + sub : d.h, ystep = 4 * rpw;
    int mn = 255, mx = 0;
    for (int y = ystart; y < d.h; y += ystep) {
        const uint8_t* row = d.base + (int64_t)y * d.pitch;
        for (int x = col0; x < d.w; x += 64) {
            const int L = pil_grey(row + 3 * (size_t)x);
            mn = L < mn ? L : mn;
            mx = L > mx ? L : mx;
        }
    }
    red[0][tid] = mn;
    red[1][tid] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] = min(red[0][tid], red[0][tid + s]);
            red[1][tid] = max(red[1][tid], red[1][tid + s]);
        }
        __syncthreads();
    }
    mn = red[0][0];
    mx = red[1][0];
    __syncthreads();
    if (mx == mn) {                                           // a uniform crop is kept whole
        if (tid == 0) { box[0] = 0; box[1] = 0; box[2] = d.w; box[3] = d.h; }
        return;
    }
    const int thr = 200 * (mx - mn);                          // (L - mn) / (mx - mn) * 255 < 200, in integers
    int x0 = d.w, y0 = d.h, x1 = 0, y1 = 0;
    for (int y = ystart; y < d.h; y += ystep) {
        const uint8_t* row = d.base + (int64_t)y * d.pitch;
        for (int x = col0; x < d.w; x += 64) {
            if ((pil_grey(row + 3 * (size_t)x) - mn) * 255 < thr) {
                x0 = x < x0 ? x : x0;
                x1 = x + 1 > x1 ? x + 1 : x1;
                y0 = y < y0 ? y : y0;
                y1 = y + 1 > y1 ? y + 1 : y1;
            }
        }
    }
    red[0][tid] = x0; red[1][tid] = y0; red[2][tid] = x1; red[3][tid] = y1;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] = min(red[0][tid], red[0][tid + s]);
            red[1][tid] = min(red[1][tid], red[1][tid + s]);
            red[2][tid] = max(red[2][tid], red[2][tid + s]);
            red[3][tid] = max(red[3][tid], red[3][tid + s]);
        }
        __syncthreads();
    }
    if (tid < 4) box[tid] = red[tid][0];
}

// src [rows] rows of `pitch` bytes, 3 channels -> dst [rows][OW][3].  Thread = one output pixel.  rows * OW <= 2^28.
__global__ void __launch_bounds__(256) resample_h_kernel(const uint8_t* __restrict__ src, int64_t pitch, int rows, int OW, AaTable t,
                                                         uint8_t* __restrict__ dst) {
    const int total = rows * OW;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int y = i / OW, ox = i - y * OW;
        const int xmin = t.bounds[2 * ox], cnt = t.bounds[2 * ox + 1];
        const int32_t* k = t.kk + (size_t)ox * t.ksize;
        const uint8_t* q = src + (int64_t)y * pitch + (size_t)xmin * 3;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int x = 0; x < cnt; ++x) {
            const int c = k[x];
            a0 += (int)q[3 * x] * c;
            a1 += (int)q[3 * x + 1] * c;
            a2 += (int)q[3 * x + 2] * c;
        }
        uint8_t* o = dst + (size_t)i * 3;
        o[0] = (uint8_t)aa_clip8(a0); o[1] = (uint8_t)aa_clip8(a1); o[2] = (uint8_t)aa_clip8(a2);
    }
}

// the vertical taps of output pixel (oy, ox) over src (rows of `pitch` bytes)
__device__ __forceinline__ void resample_v_taps(const uint8_t* __restrict__ src, int64_t pitch, int oy, int ox, const AaTable& t, int v[3]) {
    const int ymin = t.bounds[2 * oy], cnt = t.bounds[2 * oy + 1];
    const int32_t* k = t.kk + (size_t)oy * t.ksize;
    const uint8_t* q = src + (int64_t)ymin * pitch + (size_t)ox * 3;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    for (int y = 0; y < cnt; ++y, q += pitch) {
        const int c = k[y];
        a0 += (int)q[0] * c;
        a1 += (int)q[1] * c;
        a2 += (int)q[2] * c;
    }
    v[0] = aa_clip8(a0); v[1] = aa_clip8(a1); v[2] = aa_clip8(a2);
}

// src [t's input rows] rows of `pitch` bytes, OW pixels each -> dst [OH][OW][3].  OH * OW <= 2^28.
__global__ void __launch_bounds__(256) resample_v_kernel(const uint8_t* __restrict__ src, int64_t pitch, int OH, int OW, AaTable t,
                                                         uint8_t* __restrict__ dst) {
    const int total = OH * OW;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int oy = i / OW, ox = i - oy * OW;
        int v[3];
        resample_v_taps(src, pitch, oy, ox, t, v);
        uint8_t* o = dst + (size_t)i * 3;
        o[0] = (uint8_t)v[0]; o[1] = (uint8_t)v[1]; o[2] = (uint8_t)v[2];
    }
}

// Pillow's Image.reduce((fx, fy)) over the full image: src [H] rows of `pitch` bytes, W pixels each -> dst [RH][RW][3], RW = ceil(W / fx).  A cell of n pixels (the last
// row and column hold fewer) is ((sum + n / 2) * (2^24 / n)) >> 24 in 32-bit unsigned arithmetic.
__global__ void __launch_bounds__(256) formula_reduce_kernel(const uint8_t* __restrict__ src, int64_t pitch, int W, int H, int fx, int fy, int RW,
                                                             int RH, uint8_t* __restrict__ dst) {
    const int total = RW * RH;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int ry = i / RW, rx = i - ry * RW;
        const int xa = rx * fx, ya = ry * fy;
        const int nx = W - xa < fx ? W - xa : fx, ny = H - ya < fy ? H - ya : fy;
        const uint32_t n = (uint32_t)(nx * ny), m = (1u << 24) / n;
        uint32_t s0 = n / 2, s1 = n / 2, s2 = n / 2;
        for (int y = 0; y < ny; ++y) {
            const uint8_t* q = src + (int64_t)(ya + y) * pitch + (size_t)xa * 3;
            for (int x = 0; x < nx; ++x) {
                s0 += q[3 * x];
                s1 += q[3 * x + 1];
                s2 += q[3 * x + 2];
            }
        }
        uint8_t* o = dst + (size_t)i * 3;
        o[0] = (uint8_t)((s0 * m) >> 24); o[1] = (uint8_t)((s1 * m) >> 24); o[2] = (uint8_t)((s2 * m) >> 24);
    }
}

// The last stage of one crop: src (rows of `pitch` bytes, w pixels each) -> the vertical pass to h rows (has_v) or the rows as they are ->
// pasted at (pad_x, pad_y) into the 384 x 384 canvas of zeros -> out_u8 [384][384][3] (may be null) and the network input out_f
// [384][384]: x_c = (u8 * f32(1 / 255) - mean) / std, grey = .114 x_0 + .587 x_1 + .299 x_2, every operation rounded (no fma).
__global__ void __launch_bounds__(256) formula_final_kernel(const uint8_t* __restrict__ src, int64_t pitch, int w, int h, int pad_x, int pad_y,
                                                            int has_v, AaTable t, float* __restrict__ out_f, uint8_t* __restrict__ out_u8) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kFS * kFS) return;
    const int Y = i / kFS, X = i - Y * kFS;
    const int x = X - pad_x, y = Y - pad_y;
    int v[3] = {0, 0, 0};
    if (x >= 0 && x < w && y >= 0 && y < h) {
        if (has_v) {
            resample_v_taps(src, pitch, y, x, t, v);
        } else {
            const uint8_t* q = src + (int64_t)y * pitch + (size_t)x * 3;
            v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
        }
    }
    if (out_u8) {
        uint8_t* o = out_u8 + (size_t)i * 3;
        o[0] = (uint8_t)v[0]; o[1] = (uint8_t)v[1]; o[2] = (uint8_t)v[2];
    }
    const float inv255 = (float)(1.0 / 255.0), mean = 0.7931f, sd = 0.1738f;
    const float f0 = ((float)v[0] * inv255 - mean) / sd, f1 = ((float)v[1] * inv255 - mean) / sd, f2 = ((float)v[2] * inv255 - mean) / sd;
    float g = 0.114f * f0;
    g = g + 0.587f * f1;
    g = g + 0.299f * f2;
    out_f[i] = g;
}

// ---------------------------------------------------------------------------------------------------------------- host: the plan
namespace {
// Pillow's round_aspect (Image.thumbnail): of floor(v) and ceil(v) the one whose aspect is nearer, floor on a tie, at least 1
int round_aspect(double v, double aspect, bool is_x) {
#pragma clang fp contract(off)
    const double lo = std::floor(v), hi = std::ceil(v);
    auto key = [&](double n) { return is_x ? std::fabs(aspect - n / (double)kFS) : (n == 0.0 ? 0.0 : std::fabs(aspect - (double)kFS / n)); };
    const double pick = key(lo) <= key(hi) ? lo : hi;
    return pick < 1.0 ? 1 : (int)pick;
}
inline bool side_ok(long long v) { return v >= 1 && v <= RD_RESIZE_AA_MAX_SIDE; }
}  // namespace

void formula_preproc_plan(int w, int h, rd_formula_plan* p) {
#pragma clang fp contract(off)
    *p = rd_formula_plan{};
    if (!side_ok(w) || !side_ok(h)) return;                  // served = 0, nothing else is stated
    const int short_ = w <= h ? w : h, long_ = w <= h ? h : w;
    const int new_long = (int)((double)(384LL * long_) / (double)short_);      // int(384 * long / short)
    const int W = w <= h ? kFS : new_long, H = w <= h ? new_long : kFS;
    p->resize_w = W; p->resize_h = H;
    p->final_w = W; p->final_h = H;
    p->fx = p->fy = 1;
    p->reduced_w = W; p->reduced_h = H;
    p->box_w = (float)W; p->box_h = (float)H;
    p->thumb = (W > kFS || H > kFS) ? 1 : 0;
    if (p->thumb) {
        const double aspect = (double)W / (double)H;
        int x = kFS, y = kFS;
        if (1.0 >= aspect) x = round_aspect((double)kFS * aspect, aspect, true);
        else y = round_aspect((double)kFS / aspect, aspect, false);
        p->final_w = x; p->final_h = y;
        int fx = (int)((double)W / (double)x / 2.0), fy = (int)((double)H / (double)y / 2.0);
        fx = fx ? fx : 1; fy = fy ? fy : 1;
        p->fx = fx; p->fy = fy;
        if (fx > 1 || fy > 1) {
            p->reduced_w = (W + fx - 1) / fx; p->reduced_h = (H + fy - 1) / fy;
            p->box_w = (float)((double)W / (double)fx); p->box_h = (float)((double)H / (double)fy);
        }
    }
    p->pad_x = (kFS - p->final_w) / 2; p->pad_y = (kFS - p->final_h) / 2;
    p->served = (side_ok(W) && side_ok(H)) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: the launchers
int launch_formula_margin_boxes(int device, const rd_formula_crop* descs_dev, int n, int32_t* boxes_dev, hipStream_t s, std::string& err) {
    if (!descs_dev || !boxes_dev || n < 1 || n > 65535) { err = "rd_formula_margin_boxes: null descriptors / boxes, or n outside 1 .. 65535"; return 1; }
    hipError_t rc = hipSetDevice(device);
    if (rc != hipSuccess) { hip_err(rc, "hipSetDevice", err, "rd_formula_margin_boxes"); return 1; }
    hipLaunchKernelGGL(formula_margin_kernel, dim3((unsigned)n), dim3(256), 0, s, descs_dev, boxes_dev);
    rc = hipGetLastError();
    if (rc != hipSuccess) { hip_err(rc, "kernel launch", err, "rd_formula_margin_boxes"); return 1; }
    return 0;
}

// The coefficient tables of one batch: computed on the host for every crop (no cache: formula boxes rarely repeat a size), gathered in one
// pinned staging buffer per (device, stream) and uploaded with ONE hipMemcpyAsync behind the intermediates in the scratch.  The event
// marks the end of that upload: the next call on the stream waits for it (it has long happened) before it rewrites the staging buffer.
namespace {
struct FormulaStage {
    int32_t* host = nullptr;
    size_t words = 0;
    hipEvent_t uploaded = nullptr;
};
std::map<std::pair<int, hipStream_t>, FormulaStage> g_formula_stage;            // (device, stream), under g_mu

struct TabRef {                                              // one table inside the batch's block: bounds at `off`, kk behind them
    size_t off = 0;
    int out = 0, ksize = 0;
    bool on = false;
    AaTable view(const int32_t* base) const { return on ? AaTable{base + off, base + off + (size_t)out * 2, ksize} : AaTable{nullptr, nullptr, 0}; }
};
struct CropProgram {
    rd_formula_plan plan;
    TabRef h1, v1, h2, v2;                                   // bilinear horizontal / vertical, bicubic horizontal / vertical
};
TabRef add_table(std::vector<int32_t>& all, int filter, int in, float box1, int out) {
    std::vector<int32_t> bounds, kk;
    TabRef r;
    r.ksize = resample_coeffs(filter, in, 0.0, (double)box1, out, bounds, kk);
    r.off = all.size();
    r.out = out;
    r.on = true;
    all.insert(all.end(), bounds.begin(), bounds.end());
    all.insert(all.end(), kk.begin(), kk.end());
    return r;
}
}  // namespace

int launch_formula_preproc_batch(int device, const rd_formula_crop* descs, const int32_t* boxes, int n, float* out, uint8_t* out_u8, hipStream_t s,
                                 std::string& err) {
    const char* who = "rd_formula_preproc_batch";
    if (!descs || !boxes || !out || n < 1) { err = std::string(who) + ": null descriptors / boxes / output, or n < 1"; return 1; }
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    std::vector<CropProgram> progs((size_t)n);
    std::vector<int32_t> tabs;
    size_t inter = 0;                                         // bytes of the largest crop's intermediates
    for (int i = 0; i < n; ++i) {
        const rd_formula_crop& d = descs[i];
        const int32_t* b = boxes + 4 * (size_t)i;
        if (!d.base || !side_ok(d.w) || !side_ok(d.h) || d.pitch < (int64_t)d.w * 3 || b[0] < 0 || b[1] < 0 || b[2] <= b[0] || b[3] <= b[1] || b[2] > d.w ||
            b[3] > d.h) {
            err = std::string(who) + ": crop " + std::to_string(i) + ": null base, a side outside 1 .. " + std::to_string(RD_RESIZE_AA_MAX_SIDE) +
                  ", a pitch below 3 w, or a box outside the crop";
            return 1;
        }
        const int bw = b[2] - b[0], bh = b[3] - b[1];
        CropProgram& g = progs[(size_t)i];
        rd_formula_plan& p = g.plan;
        formula_preproc_plan(bw, bh, &p);
        if (!p.served) {
            err = std::string(who) + ": crop " + std::to_string(i) + ": a box of " + std::to_string(bw) + " x " + std::to_string(bh) +
                  " needs an intermediate beyond " + std::to_string(RD_RESIZE_AA_MAX_SIDE) + " pixels (rd_formula_preproc_plan: served = 0)";
            return 1;
        }
        // a pass whose in == out over the full box does not run (Pillow's need_horizontal / need_vertical)
        if (bw != p.resize_w) g.h1 = add_table(tabs, RD_RESAMPLE_BILINEAR, bw, (float)bw, p.resize_w);
        if (bh != p.resize_h) g.v1 = add_table(tabs, RD_RESAMPLE_BILINEAR, bh, (float)bh, p.resize_h);
        if (p.thumb && (p.final_w != p.reduced_w || p.box_w != (float)p.reduced_w))
            g.h2 = add_table(tabs, RD_RESAMPLE_BICUBIC, p.reduced_w, p.box_w, p.final_w);
        if (p.thumb && (p.final_h != p.reduced_h || p.box_h != (float)p.reduced_h))
            g.v2 = add_table(tabs, RD_RESAMPLE_BICUBIC, p.reduced_h, p.box_h, p.final_h);
        const size_t one = up((size_t)bh * p.resize_w * 3) + up((size_t)p.resize_h * p.resize_w * 3) + up((size_t)p.reduced_h * p.reduced_w * 3) +
                           up((size_t)p.reduced_h * p.final_w * 3);
        inter = one > inter ? one : inter;
    }
    const size_t tab_bytes = tabs.size() * sizeof(int32_t), need = inter + up(tab_bytes);
    hipError_t rc = hipSetDevice(device);
    if (rc != hipSuccess) { hip_err(rc, "hipSetDevice", err, who); return 1; }
    std::lock_guard<std::mutex> lock(g_mu);
    Scratch& sc = g_scratch[{device, s}];
    if (sc.bytes < need) {
        if (sc.p) (void)hipFree(sc.p);                       // waits for the device: no earlier launch still writes it
        sc.p = nullptr;
        sc.bytes = 0;
        rc = hipMalloc((void**)&sc.p, need);
        if (rc != hipSuccess) { hip_err(rc, "hipMalloc of the intermediates", err, who); return 1; }
        sc.bytes = need;
    }
    const int32_t* dtab = reinterpret_cast<const int32_t*>(sc.p + inter);       // inter is a multiple of 256
    if (tab_bytes) {
        FormulaStage& st = g_formula_stage[{device, s}];
        if (!st.uploaded) {
            rc = hipEventCreateWithFlags(&st.uploaded, hipEventDisableTiming);
            if (rc != hipSuccess) { st.uploaded = nullptr; hip_err(rc, "hipEventCreate", err, who); return 1; }
        } else {
            rc = hipEventSynchronize(st.uploaded);           // the previous batch's upload has left the staging buffer
            if (rc != hipSuccess) { hip_err(rc, "hipEventSynchronize", err, who); return 1; }
        }
        if (st.words < tabs.size()) {
            if (st.host) (void)hipHostFree(st.host);
            st.host = nullptr;
            st.words = 0;
            rc = hipHostMalloc((void**)&st.host, tab_bytes * 2, hipHostMallocDefault);
            if (rc != hipSuccess) { st.host = nullptr; hip_err(rc, "hipHostMalloc of the table staging buffer", err, who); return 1; }
            st.words = tabs.size() * 2;
        }
        std::copy(tabs.begin(), tabs.end(), st.host);
        rc = hipMemcpyAsync(sc.p + inter, st.host, tab_bytes, hipMemcpyHostToDevice, s);
        if (rc == hipSuccess) rc = hipEventRecord(st.uploaded, s);
        if (rc != hipSuccess) { hip_err(rc, "upload of the coefficient tables", err, who); return 1; }
    }
    for (int i = 0; i < n; ++i) {
        const rd_formula_crop& d = descs[i];
        const int32_t* b = boxes + 4 * (size_t)i;
        const CropProgram& g = progs[(size_t)i];
        const rd_formula_plan& p = g.plan;
        const int bh = b[3] - b[1], W = p.resize_w, H = p.resize_h;
        uint8_t* bufA = sc.p;                                                   // [bh][W][3]: the bilinear horizontal pass
        uint8_t* bufB = bufA + up((size_t)bh * W * 3);                          // [H][W][3]: the bilinear result
        uint8_t* bufC = bufB + up((size_t)H * W * 3);                           // [reduced_h][reduced_w][3]
        uint8_t* bufD = bufC + up((size_t)p.reduced_h * p.reduced_w * 3);       // [reduced_h][final_w][3]: the bicubic horizontal pass
        const uint8_t* cur = d.base + (int64_t)b[1] * d.pitch + (size_t)b[0] * 3;
        int64_t pitch = d.pitch;
        if (g.h1.on) {
            hipLaunchKernelGGL(resample_h_kernel, dim3(aa_grid((long)bh * W)), dim3(256), 0, s, cur, pitch, bh, W, g.h1.view(dtab), bufA);
            cur = bufA; pitch = (int64_t)W * 3;
        }
        TabRef tv;                                                              // the vertical pass the final kernel runs
        int vw = W, vh = H;                                                     // the size in front of the pad
        if (g.v1.on) {
            if (p.thumb) {
                hipLaunchKernelGGL(resample_v_kernel, dim3(aa_grid((long)H * W)), dim3(256), 0, s, cur, pitch, H, W, g.v1.view(dtab), bufB);
                cur = bufB; pitch = (int64_t)W * 3;
            } else {
                tv = g.v1;
            }
        }
        if (p.thumb) {
            if (p.fx > 1 || p.fy > 1) {
                hipLaunchKernelGGL(formula_reduce_kernel, dim3(aa_grid((long)p.reduced_h * p.reduced_w)), dim3(256), 0, s, cur, pitch, W, H, p.fx,
                                   p.fy, p.reduced_w, p.reduced_h, bufC);
                cur = bufC; pitch = (int64_t)p.reduced_w * 3;
            }
            vw = p.final_w; vh = p.final_h;
            if (g.h2.on) {
                hipLaunchKernelGGL(resample_h_kernel, dim3(aa_grid((long)p.reduced_h * p.final_w)), dim3(256), 0, s, cur, pitch, p.reduced_h, p.final_w,
                                   g.h2.view(dtab), bufD);
                cur = bufD; pitch = (int64_t)p.final_w * 3;
            }
            if (g.v2.on) tv = g.v2;
        }
        hipLaunchKernelGGL(formula_final_kernel, dim3((kFS * kFS + 255) / 256), dim3(256), 0, s, cur, pitch, vw, vh, p.pad_x, p.pad_y, tv.on ? 1 : 0,
                           tv.view(dtab), out + (size_t)i * kFS * kFS, out_u8 ? out_u8 + (size_t)i * kFS * kFS * 3 : nullptr);
    }
    rc = hipGetLastError();
    if (rc != hipSuccess) { hip_err(rc, "kernel launch", err, who); return 1; }
    return 0;
}

}  // namespace rd
