// rd_stage_pack (include/rapiddoc_mi355.h): the host images of a plugin-seam call - numpy crops in pageable memory, each with its own row
// pitch - gathered row by row into one pinned staging buffer, so that ONE host-to-device copy carries them all.  Host code only: no HIP
// call, no global state; rapiddoc_amd.host_stage.HostImageStage owns the buffer and the copy.
//
// Work is shared out by BYTES, at row granularity: the packed rows of all images in order form one byte sequence of `total` bytes, thread
// t of T copies the rows that START inside [total * t / T, total * (t + 1) / T).  Every row belongs to exactly one thread, and a thread
// finds its rows of image i from the image's first byte in that sequence alone - no search, no shared counter.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/rapiddoc_mi355.h"

namespace {

constexpr int kMaxThreads = 16;
constexpr int64_t kBytesPerThread = 64 * 1024;       // below this a thread costs more than it copies

struct Image {
    const uint8_t* src;
    int64_t pitch, row_bytes, first;                  // first: position of the image's first byte in the sequence of all packed rows
    int32_t h;
    uint8_t* dst;
};

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the rows of every image that start inside [lo, hi) of the packed sequence
void copy_range(const std::vector<Image>& images, int64_t lo, int64_t hi) {
    for (const Image& im : images) {
        if (im.row_bytes == 0 || im.h == 0) continue;
        const int64_t r0 = lo > im.first ? std::min<int64_t>(im.h, ceil_div(lo - im.first, im.row_bytes)) : 0;
        const int64_t r1 = hi > im.first ? std::min<int64_t>(im.h, ceil_div(hi - im.first, im.row_bytes)) : 0;
        for (int64_t r = r0; r < r1; ++r) std::memcpy(im.dst + r * im.row_bytes, im.src + r * im.pitch, (size_t)im.row_bytes);
    }
}

}  // namespace

extern "C" int rd_stage_pack(const uint8_t* const* srcs, const int64_t* pitches, const int32_t* hs, const int32_t* ws, const int64_t* offsets, int n,
                             uint8_t* dst, int64_t dst_bytes, int n_threads) {
    if (n < 0 || dst_bytes < 0) return 1;
    if (n == 0) return 0;
    if (!srcs || !pitches || !hs || !ws || !offsets || !dst) return 1;
    std::vector<Image> images;
    images.reserve((size_t)n);
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (hs[i] < 0 || ws[i] < 0 || offsets[i] < 0) return 1;
        const int64_t row_bytes = 3 * (int64_t)ws[i], bytes = row_bytes * hs[i];
        if (offsets[i] > dst_bytes || bytes > dst_bytes - offsets[i]) return 1;
        if (bytes > 0 && (!srcs[i] || (hs[i] > 1 && pitches[i] < row_bytes))) return 1;
        images.push_back({srcs[i], pitches[i], row_bytes, total, hs[i], dst + offsets[i]});
        total += bytes;
    }
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)n_threads, (int64_t)kMaxThreads, total / kBytesPerThread}));
    if (T == 1) {
        copy_range(images, 0, total);
        return 0;
    }
    std::vector<std::thread> pool;
    pool.reserve((size_t)T - 1);
    auto bound = [&](int t) { return (int64_t)((__int128)total * t / T); };
    int started = 1;                                  // threads 1 .. started - 1 run; what could not be started is copied here
    try {
        for (; started < T; ++started) pool.emplace_back(copy_range, std::cref(images), bound(started), bound(started + 1));
    } catch (const std::system_error&) {
    }
    copy_range(images, 0, bound(1));
    if (started < T) copy_range(images, bound(started), total);
    for (std::thread& th : pool) th.join();
    return 0;
}
