// Host rules every launcher and every prepare_*_weights function shares (plain inline host functions; rd_kernels.h includes this file).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace rd {

// RD_* switches: off = the first character is '0', on = it is '1', or an integer with a default.  Each call reads the environment; a site
// that wants the value once per process keeps its own function-local `static`, a site that reads per plan or per engine calls it then.
inline bool rd_env_off(const char* name) { const char* e = std::getenv(name); return e && e[0] == '0'; }
inline bool rd_env_on(const char* name) { const char* e = std::getenv(name); return e && e[0] == '1'; }
inline int rd_env_int(const char* name, int dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) : dflt; }

// Kernels that need more than 64 KB of dynamic LDS opt in once per (kernel, device): the attribute belongs to the device
// the call is made on, and one process may drive several GPUs.  `mask` is a static of the launcher, one bit per device.
inline void rd_allow_dynamic_lds(const void* kernel, size_t bytes, unsigned long long& mask) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(mask & bit)) {
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        mask |= bit;
    }
}

// CUs of the device that is current at the first call (cached for the process); 256 when the runtime does not say.
inline int rd_cu_count() {
    static const int n_cu = [] {
        int dev = 0, n = 0;
        (void)hipGetDevice(&dev);
        return hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
    }();
    return n_cu;
}

// CUs the persistent matrix kernels size their grids for.  Their workgroups book a CU's LDS and registers completely (gemm_h1 2 x 80 KB,
// the mixers 146 - 148 KB), so while one of them covers all 256 CUs nothing of another stream - not even a bandwidth-bound depthwise
// launch that needs no matrix pipe - can start: RD_PERSISTENT_CUS=n leaves 256 - n CUs (spread over the XCDs by the dispatcher's round robin)
// to whatever else is in flight.  Default: all of them.
//   rd_cu_budget(rd_cu_count()):  conv3x3_h1, conv9x9_h1, gemm_h1, mixer_res, mixer_ws
//   rd_cu_count() as it is:       conv_h3 (8-wavefront tiles), conv_direct_h3, gemm_h3_dma, stem34, stem_fused
inline int rd_cu_budget(int n_cu) {
    static const int env = rd_env_int("RD_PERSISTENT_CUS", 0);
    return env > 0 && env < n_cu ? env : n_cu;
}

// The single-accumulator split kernels scale a weight matrix by ONE power of two: the exponent ex with max |w| * 2^ex in [2^13, 2^14);
// 0 for an all-zero matrix or one with a non-finite element.  clamp > 0 bounds |ex| (a scale and its inverse that both stay normal
// floats); RD_EXP_NO_CLAMP leaves ex as it comes, which differs only where max |w| < 2^-86.
constexpr int RD_EXP_CLAMP = 100, RD_EXP_NO_CLAMP = 0;
inline int rd_pow2_exp(const float* w, size_t n, int clamp) {
    float mx = 0.f;
    for (size_t i = 0; i < n; ++i) mx = std::fmax(mx, std::fabs(w[i]));
    if (!(mx > 0.f) || !std::isfinite(mx)) return 0;
    int x = 0;
    (void)std::frexp(mx, &x);           // mx = m * 2^x, m in [0.5, 1)
    const int ex = 14 - x;
    return clamp <= 0 ? ex : ex > clamp ? clamp : ex < -clamp ? -clamp : ex;
}

inline uint16_t rd_half_bits(_Float16 h) {
    uint16_t b;
    __builtin_memcpy(&b, &h, 2);
    return b;
}
// fp16 (hi, lo) halves of the scaled weight vs = v * 2^ex: hi = fp16(vs), lo = fp16(vs - hi)
inline void rd_split_scaled(float v, int ex, uint16_t& hi, uint16_t& lo) {
    const float vs = std::ldexp(v, ex);
    const _Float16 h = (_Float16)vs;
    hi = rd_half_bits(h);
    lo = rd_half_bits((_Float16)(vs - (float)h));
}
// ... and of the three-product ("h3") kernels: hi = fp16(v), lo = fp16((v - hi) * 2048)
inline void rd_split_2048(float v, uint16_t& hi, uint16_t& lo) {
    const _Float16 h = (_Float16)v;
    hi = rd_half_bits(h);
    lo = rd_half_bits((_Float16)((v - (float)h) * 2048.f));
}

}  // namespace rd
