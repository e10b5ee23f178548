"""The auto-mode lane decision of the slice mapping without a device (csrc/ratspn_slice_lanes.h: slice_lanes_next, the pure
function slice_lanes_auto applies to what a look at the peer streams found).  The header is plain C++: the test compiles
it into a small program that replays sequences of looks and prints the lane count after each, and checks the table:
a fresh workspace counts the full streak, a workspace that was sharing when its peers fell idle takes its share again at
the first busy look within DPS_AUTO_REENTRY launches, and not after that."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'

MAIN = r'''
#include "ratspn_slice_lanes.h"
#include "deeprob_slice.h"
#include <stdio.h>
#include <stdlib.h>
// argv[1]: the re-entry bound (negative: the header's); argv[2..]: busy peers found at each look of one workspace
int main(int argc, char **argv) {
    int reentry = atoi(argv[1]);
    if (reentry < 0) reentry = DPS_AUTO_REENTRY;
    dpk::SliceLaneState s{0, 1, 0, 0};
    for (int i = 2; i < argc; ++i) {
        s = dpk::slice_lanes_next(s, atoi(argv[i]), DPS_AUTO_STREAK, DPS_AUTO_LANES_MAX, reentry);
        printf("%d ", s.lanes);
    }
    printf("\n");
    return 0;
}
'''


@pytest.fixture(scope='module')
def looks(tmp_path_factory):
    d = tmp_path_factory.mktemp('reentry')
    src, exe = str(d / 'main.cpp'), str(d / 'looks')
    open(src, 'w').write(MAIN)
    r = subprocess.run([CXX, '-x', 'c++', '-std=c++17', '-O1', '-I' + os.path.join(ROOT, 'deeprob-kit_amd', 'csrc'),
                        '-I' + os.path.join(ROOT, 'include'), src, '-o', exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]

    def run(busy, reentry=-1):
        out = subprocess.run([exe, str(reentry)] + [str(b) for b in busy], stdout=subprocess.PIPE, text=True, check=True,
                             timeout=60).stdout
        return [int(t) for t in out.split()]
    return run


def constants():
    from deeprob.hip import slice as sl
    return sl.DPS_AUTO_STREAK, sl.DPS_AUTO_LANES_MAX, sl.DPS_AUTO_REENTRY


def test_constants():
    streak, lanes_max, reentry = constants()
    assert (streak, lanes_max) == (4, 4) and 1 <= reentry <= 64


def test_fresh_workspace_counts_the_full_streak(looks):
    streak, lanes_max, _ = constants()
    assert looks([1] * 6) == [1] * (streak - 1) + [2] * (7 - streak)
    assert looks([0, 1, 1, 1, 0, 1, 1, 1, 1]) == [1] * 8 + [2]                 # (an idle look starts the count again)
    assert looks([2] * 5) == [1] * (streak - 1) + [3, 3]
    assert looks([7] * 5)[-1] == lanes_max                                    # (1 + busy, capped)
    assert looks([1] * 4 + [2, 1]) == [1, 1, 1, 2, 3, 2]                      # (a settled lane follows its peers)


def test_a_lane_that_was_sharing_comes_back_at_the_first_busy_look(looks):
    streak, _, reentry = constants()
    warm = [1] * streak
    # the loop synchronises: one idle look (the whole chip), then busy again: the share at once, and it stays
    assert looks(warm + [0, 1, 1]) == [1] * (streak - 1) + [2, 1, 2, 2]
    assert looks([2] * streak + [0, 1])[-2:] == [1, 3]                        # (the lane count it had, not 1 + busy)
    # ... at any of the `reentry` launches after the idle look, and not at the next one
    for idle in range(1, reentry + 3):
        got = looks(warm + [0] * idle + [1])
        assert got[streak:streak + idle] == [1] * idle
        assert got[-1] == (2 if idle <= reentry else 1), (idle, got)
    # past the gap the full streak is due again
    late = looks(warm + [0] * (reentry + 1) + [1] * streak)
    assert late[-streak:] == [1] * (streak - 1) + [2]
    # the memory is spent by one re-entry: the next idle look renews it, an idle look of a lane that did not share does not
    assert looks(warm + [0, 1, 0, 1]) == [1] * (streak - 1) + [2, 1, 2, 1, 2]
    assert looks([1, 1, 0, 1]) == [1, 1, 1, 1]


def test_no_reentry_is_the_previous_rule(looks):
    """With a bound of 0 the decision is the one that went before: lanes = 1 + busy once the streak is full, else 1."""
    import random
    streak, lanes_max, _ = constants()
    rng = random.Random(7)
    for _ in range(20):
        busy = [rng.choice([0, 0, 1, 1, 1, 2, 5]) for _ in range(40)]
        want, run = [], 0
        for b in busy:
            run = min(run + 1, streak) if b > 0 else 0
            want.append(min(1 + b, lanes_max) if run >= streak else 1)
        assert looks(busy, reentry=0) == want
