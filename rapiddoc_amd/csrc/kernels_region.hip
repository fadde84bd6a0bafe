// Region composition on the device (include/rapiddoc_mi355.h rd_region_canvases): the detector / recogniser canvases of the OCR and table
// stages - crop_img (rapid_doc/utils/model_utils.py:90-124) with its polygon mask, and _apply_mask_boxes_to_image (analyze_utils.py:82-103)
// - written from the pages where they lie in HBM.  Every region names its own page (address, pitch, size), so the pages of a launch
// need not be of one size.  No weights; a byte copy.
//   region_mask_kernel      the keep mask of every region that has a polygon, one thread per canvas pixel of the region's window: the
//                           polygon's edges are set up once per workgroup in LDS (region_geom.h make_edge), then every pixel asks
//                           rd_region::keep - rows, pixels and regions all in parallel, no pass ordering between fill and outline.  The
//                           mask is one byte per canvas pixel in the workspace, written only inside the window.
//   region_compose_kernel   canvas k <- 255, the page pixel inside the region's clipped window (255 where the mask says so), and the same
//                           with every mask box at 255 for the detector's copy.  VEC: 16 bytes per lane (canvas rows that are multiples
//                           of 16 bytes on 16-byte aligned canvases - every RegionOcr canvas, gw % 64 == 0); otherwise one pixel per lane.
// Nothing is written outside the two canvas arrays; page bytes are read only inside the window clipped to the page.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "rd_kernels.h"
#include "region_geom.h"

namespace {

static_assert(sizeof(rd_region_desc) == 64, "rd_region_desc layout");
static_assert(RD_REGION_MAX_POLY == rd_region::kMaxPoly, "one vertex cap");

constexpr int kMaskPixelsPerBlock = 1024;

// the region rectangle clipped to the page: size, page origin, canvas origin
struct Window { int w, h, px, py, cx, cy; };

__host__ __device__ inline Window window_of(const rd_region_desc& d) {
    const int x0c = d.x0 > 0 ? d.x0 : 0, y0c = d.y0 > 0 ? d.y0 : 0;
    const int x1c = d.x1 < d.page_w ? d.x1 : d.page_w, y1c = d.y1 < d.page_h ? d.y1 : d.page_h;
    Window wn;
    wn.w = x1c > x0c && y1c > y0c ? x1c - x0c : 0;
    wn.h = x1c > x0c && y1c > y0c ? y1c - y0c : 0;
    wn.px = x0c; wn.py = y0c;
    wn.cx = d.paste_x + (x0c - d.x0); wn.cy = d.paste_y + (y0c - d.y0);
    return wn;
}

__global__ __launch_bounds__(256) void region_mask_kernel(const rd_region_desc* __restrict__ descs, const int32_t* __restrict__ pts, int gh, int gw,
                                                          uint8_t* __restrict__ mask) {
    const rd_region_desc d = descs[blockIdx.y];
    if (d.poly_n <= 0) return;
    const Window wn = window_of(d);
    const long long first = (long long)blockIdx.x * kMaskPixelsPerBlock, total = (long long)gh * gw;
    const long long last = first + kMaskPixelsPerBlock < total ? first + kMaskPixelsPerBlock : total;       // pixels [first, last)
    if (wn.w == 0 || first >= total || (int)((last - 1) / gw) < wn.cy || (int)(first / gw) >= wn.cy + wn.h) return;   // (uniform: whole block)
    __shared__ rd_region::Edge edges[rd_region::kMaxPoly];
    const int n = d.poly_n;
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
        const int32_t* p = pts + 2 * ((size_t)d.poly_off + (t == 0 ? n - 1 : t - 1));
        const int32_t* q = pts + 2 * ((size_t)d.poly_off + t);
        // the polygon translated by the UNclipped corner, on a window that starts at the clipped one: polygon_keep_mask's raster
        edges[t] = rd_region::make_edge(p[0] - d.x0, p[1] - d.y0, q[0] - d.x0, q[1] - d.y0);
    }
    __syncthreads();
    uint8_t* m = mask + (size_t)blockIdx.y * (size_t)total;
    for (long long i = first + threadIdx.x; i < last; i += blockDim.x) {
        const int y = (int)(i / gw), x = (int)(i - (long long)y * gw);
        const int wx = x - wn.cx, wy = y - wn.cy;
        if (wx < 0 || wy < 0 || wx >= wn.w || wy >= wn.h) continue;
        m[i] = rd_region::keep(edges, n, wx, wy) ? 1 : 0;
    }
}

struct Pixel { const uint8_t* src; bool boxed; };     // src: the page pixel, or null for white

__device__ inline Pixel pixel_of(const rd_region_desc& d, const Window& wn, const uint8_t* __restrict__ m, const int32_t* __restrict__ boxes,
                                 int gw, int x, int y) {
    Pixel p{nullptr, false};
    const int wx = x - wn.cx, wy = y - wn.cy;
    if (wx >= 0 && wy >= 0 && wx < wn.w && wy < wn.h && (d.poly_n <= 0 || m[(size_t)y * gw + x]))
        p.src = d.page + (size_t)(wn.py + wy) * (size_t)d.pitch + (size_t)(wn.px + wx) * 3;
    for (int b = 0; b < d.box_n; ++b) {
        const int32_t* q = boxes + 4 * ((size_t)d.box_off + b);
        p.boxed = p.boxed || (x >= q[0] && x < q[2] && y >= q[1] && y < q[3]);
    }
    return p;
}

template <bool VEC>
__global__ __launch_bounds__(256) void region_compose_kernel(const rd_region_desc* __restrict__ descs, const int32_t* __restrict__ boxes, int gh, int gw,
                                                             const uint8_t* __restrict__ mask, uint8_t* __restrict__ canv, uint8_t* __restrict__ det) {
    const rd_region_desc d = descs[blockIdx.y];
    const Window wn = window_of(d);
    const size_t pixels = (size_t)gh * gw;
    const uint8_t* m = mask ? mask + (size_t)blockIdx.y * pixels : nullptr;
    uint8_t* c = canv + (size_t)blockIdx.y * pixels * 3;
    uint8_t* dc = det ? det + (size_t)blockIdx.y * pixels * 3 : nullptr;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (VEC) {                                       // 16 bytes of ONE canvas row (the row length is a multiple of 16)
        const size_t row_bytes = (size_t)gw * 3, off = i * 16;
        if (off >= pixels * 3) return;
        const int y = (int)(off / row_bytes), bx = (int)(off - (size_t)y * row_bytes);
        int x = bx / 3, ch = bx - 3 * x;
        alignas(16) uint8_t out[16];
        alignas(16) uint8_t dout[16];
        Pixel p = pixel_of(d, wn, m, boxes, gw, x, y);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const uint8_t v = p.src ? p.src[ch] : (uint8_t)255;
            out[t] = v;
            dout[t] = p.boxed ? (uint8_t)255 : v;
            if (++ch == 3 && t < 15) { ch = 0; ++x; p = pixel_of(d, wn, m, boxes, gw, x, y); }
        }
        *reinterpret_cast<uint4*>(c + off) = *reinterpret_cast<const uint4*>(out);
        if (dc) *reinterpret_cast<uint4*>(dc + off) = *reinterpret_cast<const uint4*>(dout);
    } else {                                         // any width: one pixel per lane
        if (i >= pixels) return;
        const int y = (int)(i / gw), x = (int)(i - (size_t)y * gw);
        const Pixel p = pixel_of(d, wn, m, boxes, gw, x, y);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const uint8_t v = p.src ? p.src[ch] : (uint8_t)255;
            c[i * 3 + ch] = v;
            if (dc) dc[i * 3 + ch] = p.boxed ? (uint8_t)255 : v;
        }
    }
}

constexpr int kMaxSide = 16384, kMaxRegions = 65535, kMaxCoord = 1 << 28;

}  // namespace

namespace rd {

size_t region_canvases_workspace_bytes(int n, int gh, int gw) {
    if (n < 1 || n > kMaxRegions || gh < 1 || gw < 1 || gh > kMaxSide || gw > kMaxSide) return 0;
    return ((size_t)n * gh * gw + 15) / 16 * 16;
}

// What a descriptor list must satisfy before anything is launched; boxes_host = the mask boxes the descriptors index (null: not looked at).
// Sets *any_poly / *n_boxes (the length of the box list the descriptors span).
int region_check_descs(const rd_region_desc* d, int n, int gh, int gw, const int32_t* boxes_host, bool* any_poly, size_t* n_boxes, std::string& err) {
    auto small = [](int v) { return v >= -kMaxCoord && v <= kMaxCoord; };
    *any_poly = false;
    *n_boxes = 0;
    for (int k = 0; k < n; ++k) {
        const std::string who = "region " + std::to_string(k) + ": ";
        if (d[k].poly_n < 0 || d[k].poly_off < 0 || d[k].box_n < 0 || d[k].box_off < 0) { err = who + "negative polygon / box offset or count"; return 1; }
        if (d[k].poly_n > RD_REGION_MAX_POLY) {
            err = who + "polygon of " + std::to_string(d[k].poly_n) + " vertices, the cap is " + std::to_string(RD_REGION_MAX_POLY);
            return 1;
        }
        if (!small(d[k].x0) || !small(d[k].y0) || !small(d[k].x1) || !small(d[k].y1) || !small(d[k].paste_x) || !small(d[k].paste_y) ||
            d[k].page_w < 0 || d[k].page_h < 0 || d[k].page_w > kMaxCoord || d[k].page_h > kMaxCoord) {
            err = who + "coordinates beyond +-2^28";
            return 1;
        }
        const Window wn = window_of(d[k]);
        if (wn.w > 0 && (!d[k].page || d[k].pitch < 3 * (int64_t)d[k].page_w)) { err = who + "page is NULL or its pitch is below 3 * page_w"; return 1; }
        *any_poly = *any_poly || d[k].poly_n > 0;
        if (d[k].box_n > 0 && (size_t)d[k].box_off + d[k].box_n > *n_boxes) *n_boxes = (size_t)d[k].box_off + d[k].box_n;
        if (!boxes_host) continue;
        for (int b = 0; b < d[k].box_n; ++b) {
            const int32_t* q = boxes_host + 4 * ((size_t)d[k].box_off + b);
            if (q[0] < 0 || q[1] < 0 || q[2] > gw || q[3] > gh || q[0] >= q[2] || q[1] >= q[3]) {
                err = who + "mask box " + std::to_string(b) + " is empty or leaves the " + std::to_string(gh) + " x " + std::to_string(gw) + " canvas";
                return 1;
            }
        }
    }
    return 0;
}

int launch_region_canvases(int device, const rd_region_desc* descs, int n, const int32_t* pts, const int32_t* boxes, int gh, int gw, uint8_t* canv,
                           uint8_t* det, void* ws, size_t ws_bytes, hipStream_t s, std::string& err) {
    const std::string who = "rd_region_canvases: ";
    if (!descs || !canv) { err = who + "descriptors or canvases are NULL"; return 1; }
    if (n < 1 || n > kMaxRegions) { err = who + "n outside 1 .. " + std::to_string(kMaxRegions); return 1; }
    if (gh < 1 || gw < 1 || gh > kMaxSide || gw > kMaxSide) { err = who + "gh, gw outside 1 .. " + std::to_string(kMaxSide); return 1; }
    hipError_t rc = hipSetDevice(device);
    if (rc != hipSuccess) { err = who + "hipSetDevice: " + hipGetErrorString(rc); return 1; }
    // The descriptors live on the device; the checks need them here.  64 bytes a region (and 16 a mask box) come back on the caller's
    // stream - behind the upload that wrote them - before anything is launched.
    std::vector<rd_region_desc> host(n);
    rc = hipMemcpyAsync(host.data(), descs, sizeof(rd_region_desc) * (size_t)n, hipMemcpyDeviceToHost, s);
    if (rc == hipSuccess) rc = hipStreamSynchronize(s);
    if (rc != hipSuccess) { err = who + "reading the descriptors back: " + hipGetErrorString(rc); return 1; }
    bool any_poly = false;
    size_t n_boxes = 0;
    if (region_check_descs(host.data(), n, gh, gw, nullptr, &any_poly, &n_boxes, err) != 0) { err = who + err; return 1; }
    if (n_boxes > 0) {
        if (!boxes) { err = who + "a region has mask boxes but boxes_dev is NULL"; return 1; }
        std::vector<int32_t> hb(4 * n_boxes);
        rc = hipMemcpyAsync(hb.data(), boxes, sizeof(int32_t) * hb.size(), hipMemcpyDeviceToHost, s);
        if (rc == hipSuccess) rc = hipStreamSynchronize(s);
        if (rc != hipSuccess) { err = who + "reading the mask boxes back: " + hipGetErrorString(rc); return 1; }
        if (region_check_descs(host.data(), n, gh, gw, hb.data(), &any_poly, &n_boxes, err) != 0) { err = who + err; return 1; }
    }
    if (any_poly) {
        if (!pts) { err = who + "a region has a polygon but pts_dev is NULL"; return 1; }
        const size_t need = region_canvases_workspace_bytes(n, gh, gw);
        if (!ws || ws_bytes < need) {
            err = who + "workspace holds " + std::to_string(ws ? ws_bytes : 0) + " bytes, " + std::to_string(need) + " needed";
            return 1;
        }
    }
    const size_t pixels = (size_t)gh * gw;
    uint8_t* mask = any_poly ? static_cast<uint8_t*>(ws) : nullptr;
    if (any_poly)
        hipLaunchKernelGGL(region_mask_kernel, dim3((unsigned)((pixels + kMaskPixelsPerBlock - 1) / kMaskPixelsPerBlock), n), dim3(256), 0, s, descs, pts,
                           gh, gw, mask);
    const bool vec = (gw * 3) % 16 == 0 && reinterpret_cast<uintptr_t>(canv) % 16 == 0 && reinterpret_cast<uintptr_t>(det) % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(region_compose_kernel<true>, dim3((unsigned)((pixels * 3 / 16 + 255) / 256), n), dim3(256), 0, s, descs, boxes, gh, gw, mask, canv, det);
    else
        hipLaunchKernelGGL(region_compose_kernel<false>, dim3((unsigned)((pixels + 255) / 256), n), dim3(256), 0, s, descs, boxes, gh, gw, mask, canv, det);
    rc = hipGetLastError();
    if (rc != hipSuccess) { err = who + "kernel launch: " + hipGetErrorString(rc); return 1; }
    return 0;
}

}  // namespace rd
