// libdeeprob_dgc.so's instance of the shared entry-point scaffolding (error text, checks, compute units).
#pragma once
#include "../../../include/deeprob_dgc.h"
#define DP_ENTRY_NS dpg_detail
#define DP_ENTRY_ELAUNCH DPG_ELAUNCH
#include "../shared/entry.h"

#define DPG_REQUIRE(cond, ...) DP_REQUIRE(cond, DPG_EINVAL, __VA_ARGS__)
#define DPG_LAUNCH DP_LAUNCH
