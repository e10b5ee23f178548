"""Auto-mode lanes of the slice mapping across a synchronisation (csrc/ratspn_gemm_slice.hip: slice_lanes_auto, the decision
in csrc/ratspn_slice_lanes.h): two replicas on two streams at B = 7 681, the smallest slice batch.  A fresh workspace counts
the full streak before it shares; a workspace that was sharing when a look found its peers idle (the caller synchronised)
is back on its share at the first look that finds them busy -- within DPS_AUTO_REENTRY of its launches, not after; the first
launch after idle takes the whole chip; dps_slice_lanes(1) overrides all of it; and every launch's per-sample results are
those of the whole-chip launch, bit for bit.

What a look finds is made deterministic: every launch is followed, on its stream, by a few passes over a 1 GiB buffer
(~1.5 ms of device time, against some tens of microseconds of host time per launch), so a stream that was launched on since
the last synchronisation is still busy when the other stream's launch looks at it."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 784
B = 7681


@pytest.fixture
def auto_lanes():
    from deeprob.hip import load_library, slice as sl
    lib = load_library()
    prev = lib.dpk_ratspn_slice_batch_min(-2)          # (the library's own threshold: B is the smallest slice batch)
    prev_lanes = sl.lanes(0)
    gc.collect()                                        # (workspaces of earlier tests leave the registry when they are freed)
    yield sl
    sl.lanes(prev_lanes)
    lib.dpk_ratspn_slice_batch_min(prev)


class TwoStreams:
    def __init__(self, sl):
        from deeprob.spn.models import GaussianRatSpn
        from deeprob.parallel import workspace_replica
        self.sl = sl
        torch.manual_seed(0)
        model = GaussianRatSpn(D, rg_depth=2, rg_repetitions=8, rg_batch=2, rg_sum=2, random_state=42).eval().cuda()
        self.models = [model, workspace_replica(model)]
        self.xs = [torch.randn(B, D, generator=torch.Generator().manual_seed(5 + k)).cuda() for k in range(2)]
        self.streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        self.plug = [torch.zeros(1 << 28, device='cuda') for _ in range(2)]
        sl.lanes(1)
        self.plans = [self.models[k].fused_plan(self.xs[k]) for k in range(2)]
        self.ref = [self.plans[k].run().clone() for k in range(2)]
        sl.lanes(0)
        torch.cuda.synchronize()
        self.outs = []
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.grid_of = {n: sl.grid(-(-B // 32), cus, n, 13) for n in (1, 2)}

    def launch(self, k, busy_after=True):
        """One launch of replica k on its stream -> its lane count (the grid is checked against it)."""
        with torch.cuda.stream(self.streams[k]):
            self.outs.append((k, self.plans[k].run().clone()))
            lanes, grid = self.sl.last_lanes(), self.sl.last_grid()
            if busy_after:
                for _ in range(3):
                    self.plug[k].add_(1.0)
        assert grid == self.grid_of[lanes], (lanes, grid)
        return lanes

    def alternate(self, n):
        return [self.launch(i % 2) for i in range(n)]

    def drain(self, k, more=0):
        """Replica k alone, synchronised after every launch, until a look finds the other stream idle (+ `more` launches)."""
        seen = []
        while not seen or seen[-1] != 1:
            assert len(seen) < self.sl.DPS_AUTO_RECHECK, seen
            seen.append(self.launch(k, busy_after=False))
            torch.cuda.synchronize()
        for _ in range(more):
            seen.append(self.launch(k, busy_after=False))
            torch.cuda.synchronize()
        assert set(seen[:-1 - more]) <= {2} and set(seen[-1 - more:]) == {1}, seen
        return seen

    def check_outputs(self):
        torch.cuda.synchronize()
        for i, (k, o) in enumerate(self.outs):
            assert torch.equal(o, self.ref[k]), i
        self.outs = []


def test_lanes_across_a_synchronisation(auto_lanes):
    sl = auto_lanes
    streak, reentry = sl.DPS_AUTO_STREAK, sl.DPS_AUTO_REENTRY
    with torch.no_grad():
        two = TwoStreams(sl)
        # fresh workspaces: the first launch finds everything idle; from then on each stream sees the other busy
        first = two.alternate(12)
        print('12 alternating launches:', first)
        assert first[0::2] == [1] * streak + [2] * (6 - streak)              # (its first look found nothing: streak + 1 launches)
        assert first[1::2] == [1] * (streak - 1) + [2] * (7 - streak)
        torch.cuda.synchronize()
        after = two.alternate(6)
        print('after a synchronisation:', after)
        assert set(after) <= {1, 2} and after[2] == 2 and after[3] == 2     # (the second launch of each stream shares)
        two.check_outputs()

        # both lanes fall back to the whole chip at a look that finds the other stream idle ...
        print('drained:', two.drain(0), two.drain(1))
        # ... and the loop goes on: the first launch after idle takes the whole chip, everything after it the share
        back = two.alternate(6)
        print('the loop resumes:', back)
        assert back == [1, 2, 2, 2, 2, 2]
        two.check_outputs()

        # peers gone for longer than the gap: the full streak is due again, as for a fresh workspace
        print('drained:', two.drain(0, more=reentry), two.drain(1, more=reentry))
        late = two.alternate(2 * streak + 2)
        print('after {} launches alone:'.format(reentry), late)
        assert late[0::2] == [1] * streak + [2] and late[1::2] == [1] * (streak - 1) + [2, 2]
        two.check_outputs()

        # the override: every launch takes the whole chip, whatever the peers do
        sl.lanes(1)
        assert two.alternate(4) == [1] * 4
        sl.lanes(0)
        two.check_outputs()
