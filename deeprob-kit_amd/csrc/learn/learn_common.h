// What the sources of libdeeprob_learn.so share: the thread-local error text behind dpl_last_error() (defined in
// learn.hip) and the argument / launch checks of the entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/deeprob_learn.h"

namespace dpl_detail {
void set_error(const char *fmt, ...);
}

#define DPL_REQUIRE(cond, ...)                \
    do {                                      \
        if (!(cond)) {                        \
            dpl_detail::set_error(__VA_ARGS__); \
            return DPL_EINVAL;                \
        }                                     \
    } while (0)

#define DPL_LAUNCH(what, ...)                                                  \
    do {                                                                       \
        (void)hipGetLastError();                                               \
        hipLaunchKernelGGL(__VA_ARGS__);                                       \
        hipError_t e__ = hipGetLastError();                                    \
        if (e__ != hipSuccess) {                                               \
            dpl_detail::set_error("%s: %s", (what), hipGetErrorString(e__));   \
            return DPL_ELAUNCH;                                                \
        }                                                                      \
    } while (0)

namespace dpl_detail {
constexpr int kThreads = 256;
constexpr int kMaxGrid = 2147483647;
}
