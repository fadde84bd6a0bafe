// Host half of the checkbox stage (rd_checkbox_finish): rapid_doc/utils/checkbox_det_cls.py classify_checkboxes :37-91 on the records
// the device left (kernels_checkbox.hip) - the size filter and the ROI rectangle in double (checkbox_geom.h, the source the kernels
// compile too: a record that disagrees is an error, never a silent difference), label order, the contour rule on the ROI of the
// dilated line mask, the tick share.
#pragma clang fp contract(off)
#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "checkbox_geom.h"
#include "rd_kernels.h"

namespace rd {

// :53-72  findContours(roi, RETR_EXTERNAL, CHAIN_APPROX_NONE); the y that most contour points share (ties: the smaller y) and the
// runner-up; the larger of the two is the box's bottom edge.  Kept when no contour point lies below it.  An ROI without a contour
// point makes the reference raise (max of an empty list); here the candidate is rejected.
static bool contour_rule_keeps(const uint8_t* roi, int h, int w) {
    std::vector<std::vector<int32_t>> contours;
    find_external_contours(roi, h, w, true, contours);
    std::map<int, int> count;
    int y_max = -1;
    for (const auto& c : contours)
        for (size_t k = 1; k < c.size(); k += 2) {
            ++count[c[k]];
            y_max = std::max(y_max, c[k]);
        }
    if (count.empty()) return false;
    std::vector<std::pair<int, int>> order(count.begin(), count.end());          // (y, count)
    std::sort(order.begin(), order.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) {
        return a.second != b.second ? a.second > b.second : a.first < b.first;
    });
    int bottom_y = order[0].first;
    if (order.size() > 1) bottom_y = std::max(bottom_y, order[1].first);
    const double diff = (double)(y_max - bottom_y);
    return !(diff >= 0.9);
}

int checkbox_finish(const rd_checkbox_cand* cands, int n, int H, int W, rd_checkbox_box* out, int max_out, int32_t* n_out, std::string& err) {
    const char* who = "rd_checkbox_finish: ";
    if (!n_out || n < 0 || max_out < 0 || (n > 0 && !cands) || (max_out > 0 && !out) || H < 1 || W < 1 || H > RD_CHECKBOX_MAX_SIDE ||
        W > RD_CHECKBOX_MAX_SIDE) {
        err = std::string(who) + "null records / output / count, or H, W outside 1 .. " + std::to_string(RD_CHECKBOX_MAX_SIDE);
        return 1;
    }
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cands[a].key < cands[b].key; });
    std::vector<rd_checkbox_box> kept;
    std::vector<uint8_t> roi;
    for (int i : order) {
        const rd_checkbox_cand& c = cands[i];
        const rd_cb::Roi r = rd_cb::roi_rect(c.x, c.y, c.w, c.h, W, H);
        if (c.x < 0 || c.y < 0 || c.x + c.w > W || c.y + c.h > H || !rd_cb::size_ok(c.w, c.h) || r.x != c.rx || r.y != c.ry || r.w != c.rw ||
            r.h != c.rh || r.w < 1 || r.h < 1 || r.w > rd_cb::kRoiMaxW || r.h > rd_cb::kRoiMaxH) {
            err = std::string(who) + "record " + std::to_string(i) + " disagrees with the host's size filter or ROI rectangle";
            return 3;
        }
        roi.assign((size_t)r.w * r.h, 0);
        for (int y = 0; y < r.h; ++y)
            for (int x = 0; x < r.w; ++x) roi[(size_t)y * r.w + x] = (uint8_t)((c.roi[y] >> x) & 1u ? 255 : 0);
        if (!contour_rule_keeps(roi.data(), r.h, r.w)) continue;
        const double share = (double)c.tick / (double)(c.w * c.h);               // :83-88
        kept.push_back(rd_checkbox_box{c.x, c.y, c.w, c.h, share > 0.2 ? 1 : 0});
    }
    *n_out = (int32_t)kept.size();
    if ((int)kept.size() > max_out) { err = std::string(who) + "max_out too small"; return 2; }
    std::copy(kept.begin(), kept.end(), out);
    return 0;
}

}  // namespace rd
