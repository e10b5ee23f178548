// What the translation units of libdeeprob_clt.so share: the thread-local error text behind dpc_last_error(), the
// argument and launch checks, lse2 of the header's order of operations, and the shape of the segmented pair-count tile.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../../include/deeprob_clt.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libdeeprob_clt is written for gfx950 (MI355X)"
#endif

namespace dpc_detail {

// The segmented pair counts (cnet.hip, cut.hip): a work-group of kPairThreads owns kPairTile x kPairTile variable pairs
// and stages kPairWords plane words of both operands per step; grid.z is the task or the entry.
constexpr int kPairThreads = 256;
constexpr int kPairTile = 32;
constexpr int kPairWords = 32;
constexpr int kMaxGridZ = 65535;
constexpr int64_t kMaxGridX = 2147483647;

// (an inline variable: one copy for the whole library)
inline thread_local char g_error[512] = "";

inline void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

__device__ __forceinline__ float lse2(float a, float b) {
    const float hi = fmaxf(a, b), lo = fminf(a, b);
    if (hi == -INFINITY) return -INFINITY;
    return hi + log1pf(expf(lo - hi));
}

}  // namespace dpc_detail

#define DPC_REQUIRE(cond, ...)                  \
    do {                                        \
        if (!(cond)) {                          \
            dpc_detail::set_error(__VA_ARGS__); \
            return DPC_EINVAL;                  \
        }                                       \
    } while (0)

#define DPC_LAUNCH(what, ...)                                                  \
    do {                                                                       \
        (void)hipGetLastError();                                               \
        hipLaunchKernelGGL(__VA_ARGS__);                                       \
        hipError_t e__ = hipGetLastError();                                    \
        if (e__ != hipSuccess) {                                               \
            dpc_detail::set_error("%s: %s", (what), hipGetErrorString(e__));   \
            return DPC_ELAUNCH;                                                \
        }                                                                      \
    } while (0)
