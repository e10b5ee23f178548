// What the entry points of every small library (libdeeprob_learn / _clt / _dgc / _spnq / _rat) are built from: the gfx950
// guard, the thread-local error text behind <prefix>_last_error(), the argument and launch checks and the compute-unit
// count.  Instantiated once per library: its *_common.h names the library's namespace and its launch status first,
//
//     #define DP_ENTRY_NS dpr_detail
//     #define DP_ENTRY_ELAUNCH DPR_ELAUNCH
//     #include "../shared/entry.h"
//
// so the error text is DP_ENTRY_NS::g_error, a symbol of that library alone: two libraries in one process never share it.
// (libdeeprob_hip.so keeps its own dpk::set_error / DPK_REQUIRE / DPK_LAUNCH / device_cus() of common.h: the same shape --
// DPK_LAUNCH(what, ...) is DP_LAUNCH with dpk's error text -- but cached per device, and DPK_LAUNCH_IN carries the
// profiling hook.)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#if !defined(DP_ENTRY_NS) || !defined(DP_ENTRY_ELAUNCH)
#error "define DP_ENTRY_NS and DP_ENTRY_ELAUNCH before including shared/entry.h"
#endif
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "the deeprob libraries are written for gfx950 (MI355X)"
#endif

namespace DP_ENTRY_NS {

// (an inline variable: one copy for the whole library)
inline thread_local char g_error[512] = "";

inline void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

// compute units of the current device, 256 if unknown
inline int device_cus() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    return (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
}

}  // namespace DP_ENTRY_NS

// return `code` with the formatted text as the library's last error unless `cond` holds
#define DP_REQUIRE(cond, code, ...)              \
    do {                                         \
        if (!(cond)) {                           \
            DP_ENTRY_NS::set_error(__VA_ARGS__); \
            return (code);                       \
        }                                        \
    } while (0)

// hipLaunchKernelGGL(...) with the stale error dropped first; a launch that fails returns the library's *_ELAUNCH
#define DP_LAUNCH(what, ...)                                                  \
    do {                                                                      \
        (void)hipGetLastError();                                              \
        hipLaunchKernelGGL(__VA_ARGS__);                                      \
        hipError_t e__ = hipGetLastError();                                   \
        if (e__ != hipSuccess) {                                              \
            DP_ENTRY_NS::set_error("%s: %s", (what), hipGetErrorString(e__)); \
            return DP_ENTRY_ELAUNCH;                                          \
        }                                                                     \
    } while (0)
