// libdeeprob_rat.so's instance of the shared entry-point scaffolding (error text, checks, compute units).
#pragma once
#include "../../../include/deeprob_rat.h"
#define DP_ENTRY_NS dpr_detail
#define DP_ENTRY_ELAUNCH DPR_ELAUNCH
#include "../shared/entry.h"

#define DPR_REQUIRE DP_REQUIRE
#define DPR_LAUNCH DP_LAUNCH
