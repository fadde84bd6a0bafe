// Host stages between the GPU stages of a page batch, for a whole batch in one call (no GPU needed):
//
//   rd_text_boxes_order_merge   det boxes -> reading order -> same-line merge: rapiddoc_amd.ocr_host.sorted_boxes + merge_det_boxes
//                               (rapid_doc/utils/ocr_utils.py:105-127 and :16-67,130-317), which stay the definition of the result;
//   rd_ctc_rows_text            rows of rd_ctc_collapse / rd_ctc_collapse_lines -> one UTF-8 buffer + confidences: ocr_host.parse_ctc_rows
//                               + format_score (rapid_doc/backend/pipeline/analyze_utils.py:280).
//
// Both restate pure-Python loops over numpy scalars; the arithmetic below is float32 where numpy's is (float32 boxes with weak Python
// scalars, NEP 50) and must give the same bits: tests/test_host_native_boxes.py and tests/test_host_native_rows.py compare them.
#include <algorithm>
#include <charconv>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/rapiddoc_mi355.h"

#pragma clang fp contract(off)

namespace {

struct Quad {
    float p[8];                 // x0 y0 x1 y1 x2 y2 x3 y3 (tl, tr, br, bl)
};
struct BBox {
    float x0, y0, x1, y1;
};

// calculate_is_angle: the diagonal's vertical extent differs from the mean side height by more than 20 %
bool quad_is_tilted(const Quad& q) {
    const float height = ((q.p[7] - q.p[1]) + (q.p[5] - q.p[3])) / 2.0f;
    const float diag = q.p[5] - q.p[1];
    return !(0.8f * height <= diag && diag <= 1.2f * height);
}

bool y_overlap_exceeds(const BBox& a, const BBox& b, float thr) {
    const float d = std::min(a.y1, b.y1) - std::max(a.y0, b.y0);
    const float ov = d > 0.0f ? d : 0.0f;
    const float mh = std::min(a.y1 - a.y0, b.y1 - b.y0);
    return mh > 0.0f ? (ov / mh) > thr : false;
}

void put_bbox(const BBox& b, float* o) {
    o[0] = b.x0; o[1] = b.y0; o[2] = b.x1; o[3] = b.y0; o[4] = b.x1; o[5] = b.y1; o[6] = b.x0; o[7] = b.y1;
}

// one page: k records -> at most k quads at `out`; returns their number
int order_merge_page(const rd_text_box* in, int k, float* out) {
    std::vector<Quad> q((size_t)k);
    for (int i = 0; i < k; ++i)
        for (int c = 0; c < 8; ++c) q[i].p[c] = (float)(int32_t)in[i].pts[c];        // astype(int32) toward zero, then astype(float32)
    // sorted_boxes: stable by (y, x) of the first corner, then the adjacent swaps inside a row (top-left y closer than 10)
    std::stable_sort(q.begin(), q.end(), [](const Quad& a, const Quad& b) { return a.p[1] < b.p[1] || (a.p[1] == b.p[1] && a.p[0] < b.p[0]); });
    for (int i = 0; i + 1 < k; ++i)
        for (int j = i; j >= 0; --j) {
            const float dy = q[j + 1].p[1] - q[j].p[1];
            if ((dy < 0.0f ? -dy : dy) < 10.0f && q[j + 1].p[0] < q[j].p[0]) std::swap(q[j], q[j + 1]);
            else break;
        }
    // merge_det_boxes
    std::vector<BBox> flat;
    std::vector<int> tilted;
    flat.reserve((size_t)k);
    for (int i = 0; i < k; ++i) {
        if (quad_is_tilted(q[i])) tilted.push_back(i);
        else flat.push_back({q[i].p[0], q[i].p[1], q[i].p[2], q[i].p[5]});
    }
    std::stable_sort(flat.begin(), flat.end(), [](const BBox& a, const BBox& b) { return a.y0 < b.y0; });
    int n = 0;
    std::vector<BBox> line, merged;
    const size_t nf = flat.size();
    for (size_t lo = 0; lo < nf;) {
        size_t hi = lo + 1;                   // a line: every box overlaps the one before it by more than 0.6 of the smaller height
        while (hi < nf && y_overlap_exceeds(flat[hi], flat[hi - 1], 0.6f)) ++hi;
        float x_min = flat[lo].x0, x_max = flat[lo].x1, y_min = flat[lo].y0, y_max = flat[lo].y1;
        for (size_t i = lo + 1; i < hi; ++i) {
            x_min = std::min(x_min, flat[i].x0); x_max = std::max(x_max, flat[i].x1);
            y_min = std::min(y_min, flat[i].y0); y_max = std::max(y_max, flat[i].y1);
        }
        if (x_max - x_min > (y_max - y_min) * 4.0f) {         // LINE_WIDTH_TO_HEIGHT_RATIO_THRESHOLD
            line.assign(flat.begin() + lo, flat.begin() + hi);
            std::stable_sort(line.begin(), line.end(), [](const BBox& a, const BBox& b) { return a.x0 < b.x0; });
            merged.clear();
            for (BBox b : line) {
                if (!merged.empty() && !(merged.back().x1 < b.x0)) {
                    const BBox m = merged.back();
                    merged.pop_back();
                    b = {std::min(m.x0, b.x0), std::min(m.y0, b.y0), std::max(m.x1, b.x1), std::max(m.y1, b.y1)};
                }
                merged.push_back(b);
            }
            for (const BBox& m : merged) put_bbox(m, out + 8 * (size_t)n++);
        } else {
            for (size_t i = lo; i < hi; ++i) put_bbox(flat[i], out + 8 * (size_t)n++);
        }
        lo = hi;
    }
    for (int i : tilted) std::memcpy(out + 8 * (size_t)n++, q[i].p, sizeof(q[i].p));
    return n;
}

}  // namespace

extern "C" int rd_text_boxes_order_merge(const rd_text_box* boxes, const int32_t* counts, int B, int max_in, float* quads_out, int32_t* n_out) {
    if (B < 0 || max_in < 0 || (B > 0 && (!boxes || !counts || !quads_out || !n_out))) return 1;
    for (int b = 0; b < B; ++b)
        if (counts[b] < 0 || counts[b] > max_in) return 1;
    for (int b = 0; b < B; ++b)
        n_out[b] = order_merge_page(boxes + (size_t)b * max_in, counts[b], quads_out + (size_t)b * max_in * 8);
    return 0;
}

extern "C" int rd_ctc_rows_text(const uint8_t* rows, int n, int row_bytes, uint8_t* text_out, int64_t text_cap, int64_t* byte_off_out,
                                int32_t* n_chars_out, double* conf_out, double* conf3_out) {
    if (n < 0 || row_bytes < 16 || text_cap < 0 || !byte_off_out || (n > 0 && (!rows || !n_chars_out || !conf_out || !conf3_out))) return 1;
    int64_t pos = 0;
    byte_off_out[0] = 0;
    for (int b = 0; b < n; ++b) {
        const uint8_t* row = rows + (size_t)b * row_bytes;
        int32_t nbytes;
        float conf;
        std::memcpy(&nbytes, row, 4);
        std::memcpy(&conf, row + 4, 4);
        if (nbytes < 0 || nbytes > row_bytes - 16) return 1;
        if (pos + nbytes > text_cap || (nbytes > 0 && !text_out)) return 2;
        int32_t chars = 0;
        for (int32_t i = 0; i < nbytes; ++i) {
            const uint8_t c = row[16 + i];
            text_out[pos + i] = c;
            chars += (c & 0xC0) != 0x80;          // every byte that is not a UTF-8 continuation byte starts a character
        }
        pos += nbytes;
        byte_off_out[b + 1] = pos;
        n_chars_out[b] = chars;
        // float(f"{score:.3f}") of the float32's double value: both conversions are correctly rounded and know no locale
        const double s = (double)conf;
        conf_out[b] = s;
        char buf[400];
        const auto w = std::to_chars(buf, buf + sizeof(buf), s, std::chars_format::fixed, 3);
        double r = s;
        if (w.ec == std::errc()) std::from_chars(buf, w.ptr, r);
        conf3_out[b] = r;
    }
    return 0;
}
