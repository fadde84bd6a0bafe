// Stand-alone host program over csrc/resize_sources_check.h (the argument checks of rd_preproc_resize_norm_sources): the accepted and
// the refused cases, meant to be built with a host sanitizer and run on a CPU.  No HIP, no library.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/resize_sources_check_main.cpp -o /tmp/rsc && /tmp/rsc
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../rapiddoc_amd/csrc/resize_sources_check.h"

static int failures = 0;

static rd_resize_source_desc desc(int64_t off, int W = 8, int H = 8, int OW = 4, int OH = 4, int64_t pitch = 24, uintptr_t src = 4096) {
    rd_resize_source_desc d{};
    d.src = reinterpret_cast<const uint8_t*>(src);
    d.pitch = pitch; d.out_off = off; d.W = W; d.H = H; d.OW = OW; d.OH = OH;
    return d;
}

static void expect(const char* what, int want_rc, const std::vector<rd_resize_source_desc>& v, int64_t out_floats, int interp = 1, bool host = true,
                   bool dev = true, bool out = true, int n = -1, int64_t want_max = -1) {
    std::string err;
    int64_t max_px = -7;
    const void* some = reinterpret_cast<const void*>(0x10000);
    const int rc = rd::check_resize_sources(host ? v.data() : nullptr, dev ? some : nullptr, n < 0 ? (int)v.size() : n, interp, out ? some : nullptr,
                                            out_floats, max_px, err);
    const bool ok = rc == want_rc && (want_rc == 0 ? err.empty() : !err.empty()) && (want_max < 0 || max_px == want_max);
    std::printf("%-58s rc %d %s%s\n", what, rc, ok ? "ok" : "UNEXPECTED", err.empty() ? "" : ("  [" + err + "]").c_str());
    failures += ok ? 0 : 1;
}

int main() {
    const int64_t i64max = std::numeric_limits<int64_t>::max();
    // accepted
    expect("two slots, exactly fitting", 0, {desc(0), desc(48)}, 96, 1, true, true, true, -1, 16);
    expect("slots in descending order, a gap between them", 0, {desc(100), desc(3)}, 148, 2);
    expect("one source, the largest sides", 0, {desc(0, 32768, 32768, 32768, 32768, 3 * 32768)}, (int64_t)3 << 30, 2, true, true, true, -1, (int64_t)1 << 30);
    expect("65535 sources", 0, [] { std::vector<rd_resize_source_desc> v; for (int k = 0; k < 65535; ++k) v.push_back(desc(48 * (int64_t)k)); return v; }(),
           48 * (int64_t)65535);
    expect("out_floats = INT64_MAX, the last slot at its end", 0, {desc(i64max - 48)}, i64max);
    // refused
    expect("NULL host array", 1, {desc(0)}, 48, 1, false);
    expect("NULL device array", 1, {desc(0)}, 48, 1, true, false);
    expect("NULL out_dev", 1, {desc(0)}, 48, 1, true, true, false);
    expect("n = 0", 1, {desc(0)}, 48, 1, true, true, true, 0);
    expect("n = 65536", 1, std::vector<rd_resize_source_desc>(65536, desc(0)), 48);
    expect("NULL src", 1, {desc(0, 8, 8, 4, 4, 24, 0)}, 48);
    expect("pitch below 3 * W", 1, {desc(0, 8, 8, 4, 4, 23)}, 48);
    expect("W = 0", 1, {desc(0, 0)}, 48);
    expect("H = 32769", 1, {desc(0, 8, 32769)}, 48);
    expect("OW = -1", 1, {desc(0, 8, 8, -1)}, 48);
    expect("OH = 32769", 1, {desc(0, 8, 8, 4, 32769)}, i64max);
    expect("interp = 0", 1, {desc(0)}, 48, 0);
    expect("interp = 3", 1, {desc(0)}, 48, 3);
    expect("negative out_off", 1, {desc(-1)}, 48);
    expect("out_off = INT64_MIN", 1, {desc(std::numeric_limits<int64_t>::min())}, 48);
    expect("one float too far", 1, {desc(0), desc(49)}, 96);
    expect("out_off = INT64_MAX", 1, {desc(i64max)}, 96);
    expect("out_off = INT64_MAX, out_floats = INT64_MAX", 1, {desc(i64max)}, i64max);
    expect("out_off = INT64_MAX - 47, out_floats = INT64_MAX", 1, {desc(i64max - 47)}, i64max);
    expect("negative out_floats", 1, {desc(0)}, -1);
    expect("slots overlap by one float", 1, {desc(0), desc(47)}, 96);
    expect("slots overlap, descending order", 1, {desc(60), desc(20), desc(100), desc(67)}, 200);
    expect("two slots at one offset", 1, {desc(7), desc(7)}, 96);
    std::printf("%s\n", failures ? "FAILED" : "all cases as expected");
    return failures ? 1 : 0;
}
