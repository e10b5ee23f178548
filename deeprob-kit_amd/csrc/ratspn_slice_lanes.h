// The auto-mode lane decision of the RAT-SPN slice mapping (ratspn_gemm_slice.hip: slice_lanes_auto) as a pure function of
// what a workspace remembers and what its look at the peer streams found.  Plain C++, no device and no runtime call: the
// table is unit-tested on the host (tests/test_slice_reentry_host.py compiles this header into a small program).
#pragma once

namespace dpk {

struct SliceLaneState {
    int streak;   // consecutive looks that found a peer busy
    int lanes;    // what the last look decided
    int resume;   // the lane count this workspace shared at when a look found its peers idle (0: none remembered)
    int gap;      // looks that found the peers idle since then
};

// One look of a workspace at its peers: `busy` of them have work in flight.
//   - Peers busy at `streak_min` consecutive looks: 1 + busy lanes, at most `lanes_max`.
//   - A workspace that WAS sharing when a look found its peers idle (a synchronisation of the caller's loop, not the end of
//     it) goes back to the lane count it had at the first look that finds them busy again, if that look is one of the
//     `reentry` looks after the idle one; it does not count to `streak_min` a second time.  A lane on the whole chip
//     looks at every launch, so the gap is counted in launches of the workspace.  reentry = 0: no such memory.
//   - Everything else takes the whole chip: the first launch after idle, a workspace that never shared, one whose peers
//     have been gone for longer than the gap.
inline SliceLaneState slice_lanes_next(SliceLaneState s, int busy, int streak_min, int lanes_max, int reentry) {
    if (busy > 0) {
        s.streak = s.streak + 1 < streak_min ? s.streak + 1 : streak_min;
        if (s.streak >= streak_min) {
            s.lanes = 1 + busy < lanes_max ? 1 + busy : lanes_max;
        } else if (s.resume > 1 && s.gap < reentry) {
            s.lanes = s.resume;
            s.streak = streak_min;
        } else {
            s.lanes = 1;
        }
        s.resume = 0;
        s.gap = 0;
        return s;
    }
    if (s.lanes > 1) {
        s.resume = s.lanes;
        s.gap = 0;
    } else if (s.resume > 1 && ++s.gap >= reentry) {
        s.resume = 0;
        s.gap = 0;
    }
    s.streak = 0;
    s.lanes = 1;
    return s;
}

}  // namespace dpk
