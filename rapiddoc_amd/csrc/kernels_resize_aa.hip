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
// bounds [out][2] = (first source index, taps); kk [out][ksize] = int(w * 2^22 + 0.5).  Returns ksize.
int resize_aa_coeffs(int in, int out, std::vector<int32_t>& bounds, std::vector<int32_t>& kk) {
#pragma clang fp contract(off)
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;                     // the bilinear filter's own support is 1
    const int ksize = (int)std::ceil(support) * 2 + 1;
    const double ss = 1.0 / fs;
    bounds.assign((size_t)out * 2, 0);
    kk.assign((size_t)out * ksize, 0);
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double t = (x + xmin - center + 0.5) * ss;
            if (t < 0.0) t = -t;
            const double v = t < 1.0 ? 1.0 - t : 0.0;
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

const char* hip_err(hipError_t e, const char* what, std::string& err) {
    err = std::string("rd_preproc_resize_aa_norm: ") + what + ": " + hipGetErrorString(e);
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

}  // namespace rd
