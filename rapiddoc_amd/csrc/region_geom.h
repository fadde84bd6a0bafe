// "Is pixel (x, y) of an h x w window set by cv2.fillPoly(mask, [pts], 1)?" - the raster of rd_fill_poly (polygon_ops.cpp) as a function of
// ONE pixel, for the device (kernels_region.hip) and the host (rd_debug_region_keep_mask) alike: ONE source for both, as checkbox_geom.h
// and db_geom.h are for their stages.  Integer arithmetic only, 64-bit where a product can leave 32 bits.
//
//   interior   rd_fill_poly keeps, per non-horizontal edge, a 16.16 x that starts at the upper end point and grows by the truncated
//              dx = ((x1 - x0) << 16) / (y1 - y0) per row.  Integer addition is exact, so on row y the edge stands at
//              x_start + (y - y0) * dx: rows are independent.  The active edges (y0 <= y < y1) sorted by x are paired (0,1), (2,3), ...
//              and a pair fills ceil(left) .. floor(right), i.e. pixel x is set iff left <= (x << 16) <= right for some pair.  With
//              lt / le = the number of active edges left of / not right of X = x << 16, the sorted positions lt .. le - 1 hold X itself, and
//              such a pair exists iff an EVEN index e with lt - 1 <= e <= le - 1 and e + 1 < (active edges) exists: no sort is needed,
//              and ties in the sort cannot matter.
//   boundary   draw_line8 walks an edge from its left end point: `major` steps along the longer axis, a step along the other axis
//              whenever err < 0, err starting at major - 2 minor.  err stays inside [-2 minor, 2 major - 2 minor), which fixes the
//              number of minor steps taken before step i: c(i) = floor((2 minor i + major - 1) / (2 major)).  Pixel (x, y) is on the
//              walk iff its major-axis offset i lies in 0 .. major and its minor-axis offset equals c(i) - tested without a division.
//   degenerate n == 0 sets nothing; n == 1 and n == 2 have no interior (a pair of coinciding edges fills only where the line itself passes
//              through a pixel centre) - the same code serves them.
// tests/test_region_geom_host.py holds this header to rd_fill_poly pixel for pixel.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RD_RG_HD __host__ __device__ inline
#else
#define RD_RG_HD inline
#endif

namespace rd_region {

constexpr int kMaxPoly = 64;            // RD_REGION_MAX_POLY: the most vertices a polygon of a region may have on the device route
constexpr int kShift = 16;              // cv2's XY_SHIFT

struct Edge {
    int32_t ax, ay, bx, by;             // the line, left end point first (draw_line8 swaps the same way)
    int32_t y0, y1;                     // interior: active on rows y0 <= y < y1; y0 == y1 for a horizontal edge (never active)
    int64_t xs, dx;                     // 16.16 x on row y0, increment per row
};

// the edge p -> q (window coordinates)
RD_RG_HD Edge make_edge(int32_t px, int32_t py, int32_t qx, int32_t qy) {
    Edge e;
    const bool swap = qx < px;
    e.ax = swap ? qx : px; e.ay = swap ? qy : py;
    e.bx = swap ? px : qx; e.by = swap ? py : qy;
    e.y0 = e.y1 = 0; e.xs = e.dx = 0;
    if (py != qy) {
        const int64_t x0 = (int64_t)px << kShift, x1 = (int64_t)qx << kShift;
        e.dx = (x1 - x0) / ((int64_t)qy - (int64_t)py);          // truncated towards zero, as the host's
        if (py < qy) { e.y0 = py; e.y1 = qy; e.xs = x0; }
        else         { e.y0 = qy; e.y1 = py; e.xs = x1; }
    }
    return e;
}

// does draw_line8's walk of the edge visit (x, y)?
RD_RG_HD bool on_line(const Edge& e, int x, int y) {
    const int64_t dxl = (int64_t)e.bx - e.ax, dyl = (int64_t)e.by - e.ay;
    const int64_t ystep = dyl < 0 ? -1 : 1, ady = dyl < 0 ? -dyl : dyl;
    const bool steep = ady > dxl;
    const int64_t major = steep ? ady : dxl, minor = steep ? dxl : ady;
    const int64_t offx = (int64_t)x - e.ax, offy = ((int64_t)y - e.ay) * ystep;
    const int64_t i = steep ? offy : offx, t = steep ? offx : offy;
    if (i < 0 || i > major || t < 0) return false;
    if (major == 0) return t == 0;
    const int64_t v = 2 * minor * i + major - 1;                  // t == floor(v / (2 major))
    return 2 * major * t <= v && v < 2 * major * (t + 1);
}

// is (x, y) set by the raster of the polygon whose n edges are e[0 .. n) (make_edge(p[i - 1], p[i]), the closing edge included)?
RD_RG_HD bool keep(const Edge* e, int n, int x, int y) {
    const int64_t X = (int64_t)x << kShift;
    int lt = 0, le = 0, active = 0;
    bool hit = false;
    for (int k = 0; k < n; ++k) {
        hit = hit || on_line(e[k], x, y);
        if (e[k].y0 <= y && y < e[k].y1) {
            const int64_t xe = e[k].xs + ((int64_t)y - e[k].y0) * e[k].dx;
            ++active;
            lt += xe < X ? 1 : 0;
            le += xe <= X ? 1 : 0;
        }
    }
    if (hit) return true;
    int lo = lt - 1 < 0 ? 0 : lt - 1;
    lo += lo & 1;                                                  // the first even index >= lt - 1
    const int hi = le - 1 < active - 2 ? le - 1 : active - 2;
    return lo <= hi;
}

}  // namespace rd_region
