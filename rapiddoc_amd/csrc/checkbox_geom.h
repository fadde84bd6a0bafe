// Arithmetic of the checkbox stage that the device (kernels_checkbox.hip) and the host (checkbox_host.cpp) must do alike: ONE source
// for both, as db_geom.h is for the DB post-process.  rapid_doc/utils/checkbox_det_cls.py classify_checkboxes :38-49, in Python's
// float64: products rounded one by one, int() truncating towards zero, no fused multiply-add.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RD_CB_HD __host__ __device__ inline
#else
#define RD_CB_HD inline
#endif
#pragma clang fp contract(off)

namespace rd_cb {

constexpr int kMinSide = 12, kMaxSide = 50;              // min_width / max_width
constexpr int kRoiMaxW = 60, kRoiMaxH = 70;              // int(50 * 1.2), int(50 * 1.4)
constexpr int kGreyThresh = 150, kLine = 15, kLineHalf = 7;

// OpenCV 4's 15-bit BGR2GRAY
RD_CB_HD int grey_bgr(int b, int g, int r) { return (3735 * b + 19235 * g + 9798 * r + 16384) >> 15; }

// the label-order key of a pixel: its 2 x 2 block in block-raster order (first provisional label of OpenCV's block-based labelers)
RD_CB_HD int32_t block_key(int x, int y) { return ((int32_t)(y >> 1) << 16) | (int32_t)(x >> 1); }

// :39-40  min_width <= w, h <= max_width and 0.9 <= w / h <= 1.1
RD_CB_HD bool size_ok(int w, int h) {
    if (w < kMinSide || w > kMaxSide || h < kMinSide || h > kMaxSide) return false;
    const double ratio = (double)w / (double)h;
    return 0.9 <= ratio && ratio <= 1.1;
}

struct Roi { int x, y, w, h; };
// :43-49  the rectangle of the dilated line mask that the contour rule looks at
RD_CB_HD Roi roi_rect(int x, int y, int w, int h, int W, int H) {
    const double el = 0.1, er = 0.1, et = 0.1, eb = 0.3;
    const double wl = (double)w * el, ht = (double)h * et;
    int nx = (int)((double)x - wl), ny = (int)((double)y - ht);
    nx = nx > 0 ? nx : 0;
    ny = ny > 0 ? ny : 0;
    const double fw = (1.0 + el) + er, fh = (1.0 + et) + eb;
    int nw = (int)((double)w * fw), nh = (int)((double)h * fh);
    nw = nw < W - nx ? nw : W - nx;
    nh = nh < H - ny ? nh : H - ny;
    return Roi{nx, ny, nw, nh};
}

// the 11-tap Gaussian of adaptiveThreshold(GAUSSIAN_C, 11): exp(-(i - 5)^2 / 8) normalised in double, cast to float32; taps 5 .. 10
// (tests/test_checkbox_host.py holds these constants to that formula)
#define RD_CB_MEAN_TAPS {0x1.9ac20ap-3f, 0x1.6a7e1ep-3f, 0x1.f2464cp-4f, 0x1.0ab50ap-4f, 0x1.bcb86ap-6f, 0x1.20c256p-7f}

// s = k0 x0; s += kj (x-j + xj), j = 1 .. 5, in float32; v[0 .. 10] are the eleven samples
RD_CB_HD float mean_taps(const float* v) {
    const float kMeanTap[6] = RD_CB_MEAN_TAPS;
    float s = kMeanTap[0] * v[5];
    for (int j = 1; j <= 5; ++j) {
        const float pair = v[5 - j] + v[5 + j];
        const float prod = kMeanTap[j] * pair;
        s = s + prod;
    }
    return s;
}

RD_CB_HD int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
RD_CB_HD int replicate(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

}  // namespace rd_cb
