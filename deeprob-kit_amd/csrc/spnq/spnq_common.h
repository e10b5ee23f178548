// What the translation units of libdeeprob_spnq.so share: the thread-local error text behind dpq_last_error() and the
// argument and launch checks.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../../include/deeprob_spnq.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libdeeprob_spnq is written for gfx950 (MI355X)"
#endif

namespace dpq_detail {

// (an inline variable: one copy for the whole library)
inline thread_local char g_error[512] = "";

inline void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

static inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

}  // namespace dpq_detail

#define DPQ_REQUIRE(cond, code, ...)            \
    do {                                        \
        if (!(cond)) {                          \
            dpq_detail::set_error(__VA_ARGS__); \
            return (code);                      \
        }                                       \
    } while (0)

#define DPQ_LAUNCH(what, ...)                                                  \
    do {                                                                       \
        (void)hipGetLastError();                                               \
        hipLaunchKernelGGL(__VA_ARGS__);                                       \
        hipError_t e__ = hipGetLastError();                                    \
        if (e__ != hipSuccess) {                                               \
            dpq_detail::set_error("%s: %s", (what), hipGetErrorString(e__));   \
            return DPQ_ELAUNCH;                                                \
        }                                                                      \
    } while (0)
