// What the translation units of libdeeprob_rat.so share: the thread-local error text behind dpr_last_error() and the
// argument and launch checks.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../../include/deeprob_rat.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libdeeprob_rat is written for gfx950 (MI355X)"
#endif

namespace dpr_detail {

// (an inline variable: one copy for the whole library)
inline thread_local char g_error[512] = "";

inline void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

}  // namespace dpr_detail

#define DPR_REQUIRE(cond, code, ...)            \
    do {                                        \
        if (!(cond)) {                          \
            dpr_detail::set_error(__VA_ARGS__); \
            return (code);                      \
        }                                       \
    } while (0)

#define DPR_LAUNCH(what, ...)                                                  \
    do {                                                                       \
        (void)hipGetLastError();                                               \
        hipLaunchKernelGGL(__VA_ARGS__);                                       \
        hipError_t e__ = hipGetLastError();                                    \
        if (e__ != hipSuccess) {                                               \
            dpr_detail::set_error("%s: %s", (what), hipGetErrorString(e__));   \
            return DPR_ELAUNCH;                                                \
        }                                                                      \
    } while (0)
