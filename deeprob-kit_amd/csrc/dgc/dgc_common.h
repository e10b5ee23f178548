// What the translation units of libdeeprob_dgc.so share: the thread-local error text behind dpg_last_error(), the
// argument and launch checks, and the library's counter-based uniform.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../../include/deeprob_dgc.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libdeeprob_dgc is written for gfx950 (MI355X)"
#endif

namespace dpg_detail {

// (an inline variable: one copy for the whole library)
inline thread_local char g_error[512] = "";

inline void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

// the generator of csrc/ratspn_topdown.hip, replayed by the tests:
// (splitmix64(seed + ctr * golden) >> 40) / 2^24
__device__ __forceinline__ float td_uniform(unsigned long long seed, unsigned long long ctr) {
    unsigned long long z = seed + ctr * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(unsigned)(z >> 40) * (1.0f / 16777216.0f);
}

}  // namespace dpg_detail

#define DPG_REQUIRE(cond, ...)                  \
    do {                                        \
        if (!(cond)) {                          \
            dpg_detail::set_error(__VA_ARGS__); \
            return DPG_EINVAL;                  \
        }                                       \
    } while (0)

#define DPG_LAUNCH(what, ...)                                                  \
    do {                                                                       \
        (void)hipGetLastError();                                               \
        hipLaunchKernelGGL(__VA_ARGS__);                                       \
        hipError_t e__ = hipGetLastError();                                    \
        if (e__ != hipSuccess) {                                               \
            dpg_detail::set_error("%s: %s", (what), hipGetErrorString(e__));   \
            return DPG_ELAUNCH;                                                \
        }                                                                      \
    } while (0)
