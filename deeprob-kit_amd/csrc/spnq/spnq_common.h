// libdeeprob_spnq.so's instance of the shared entry-point scaffolding (error text, checks), and align_up.
#pragma once
#include "../../../include/deeprob_spnq.h"
#define DP_ENTRY_NS dpq_detail
#define DP_ENTRY_ELAUNCH DPQ_ELAUNCH
#include "../shared/entry.h"

#define DPQ_REQUIRE DP_REQUIRE
#define DPQ_LAUNCH DP_LAUNCH

namespace dpq_detail {

static inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

}  // namespace dpq_detail
