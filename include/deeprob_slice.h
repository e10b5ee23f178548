/*
 * deeprob_slice.h -- the grid choice of the RAT-SPN slice mapping (deeprob-kit_amd/csrc/ratspn_gemm_slice.hip), exported by
 * libdeeprob_hip.so beside the entry points of deeprob_hip.h (prefix dps_: that header's list stays what it is).  Host side
 * only: no entry point here touches the device or a stream.  No reference counterpart (the reference is launch-agnostic).
 *
 * A slice launch that has the chip to itself takes one work-group per compute unit.  Launches that run side by side -- two
 * evaluation streams, the parallel chains of a captured evaluation window -- each take a share instead and walk more blocks
 * per work-group: the cost per launch and work-group is paid less often, and while the other lanes stream.  The LANE COUNT of
 * a launch is this launch plus the launches beside it:
 *   - dps_slice_lanes(n >= 1) fixes it for the process;
 *   - else the value the caller states in the flags of dpk_ratspn_forward (DPK_FLAG_SLICE_LANES_SHIFT / _MASK);
 *   - else, for an eager launch, 1 + the other workspaces whose last slice launch went to another stream that is still busy
 *     (hipStreamQuery), at most 4, and only once that was so at 4 consecutive launches of the workspace; back to 1 at the
 *     first launch that finds them idle.  A lane that shares looks only at every 8th launch (the query puts a marker into
 *     the stream it asks about: not free for a busy peer), so it can run up to 7 launches on its share beside idle peers.
 *     A workspace that was sharing when a look found its peers idle (the caller synchronised) returns to the lane count
 *     it had at the first look within DPS_AUTO_REENTRY of its launches that finds them busy again: no second streak;
 *   - else (a launch under stream capture: nothing is queried) 1.
 * Per-sample results do not depend on the lane count, bit for bit.
 */
#ifndef DEEPROB_SLICE_H
#define DEEPROB_SLICE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPS_LANES_MAX 15     /* most lanes a launch can be told of (the flag field's four bits) */
#define DPS_AUTO_LANES_MAX 4 /* most lanes auto mode settles at                                 */
#define DPS_AUTO_STREAK 4    /* consecutive launches with busy peers before auto mode shares    */
#define DPS_AUTO_RECHECK 8   /* a lane that shares looks at its peers at every 8th launch only  */
#define DPS_AUTO_REENTRY 8   /* ... and one that shared when they fell idle: again, if busy in this many */

/* Work-groups of a slice launch over `ntiles` blocks of 32 samples on a device of `cus` compute units, run on `lanes`
 * lanes, whose first `np` work-groups carry the in-launch table check (0: none).  Pure arithmetic.
 *   lanes <= 1: min(ntiles, cus).
 *   else: gmax = max(cus / lanes, min(np, ntiles)), rounds = ceil(ntiles / gmax), grid = max(ceil(ntiles / rounds),
 *   min(np, ntiles)): the fewest work-groups that finish in `rounds` block rounds; never more than gmax.
 * 0 for ntiles <= 0 or cus <= 0. */
int32_t dps_slice_grid(int64_t ntiles, int32_t cus, int32_t lanes, int32_t np);

/* Process-wide lane count: 0 = as stated / auto (the default, also DPK_SLICE_LANES in the environment, read once),
 * 1 = every launch takes the whole chip, n = every launch runs on n lanes (at most DPS_LANES_MAX); negative: back to the
 * initial value.  Returns the previous setting. */
int32_t dps_slice_lanes(int32_t lanes);

/* The grid and the lane count of the most recent slice launch of the process (0 before the first). */
int32_t dps_slice_last_grid(void);
int32_t dps_slice_last_lanes(void);

#ifdef __cplusplus
}
#endif
#endif /* DEEPROB_SLICE_H */
