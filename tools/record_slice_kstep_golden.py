"""Writes tests/golden/slice_kstep_bits.npz: the per-sample log-likelihoods (int32 bit patterns) of every case of
tests/test_slice_kstep_bits_gpu.py, from the library DEEPROB_HIP_LIB names -- the build BEFORE the slice kernel's K-step
took its low halves from v_fma_mix_f32 (build that commit in its own tree and point DEEPROB_HIP_LIB at its
libdeeprob_hip.so).  Needs an MI355X.  The second launch of a plan must repeat its first, bit for bit, or nothing is
written: the test holds both to the fixture.

    DEEPROB_HIP_LIB=/path/to/earlier/libdeeprob_hip.so python tools/record_slice_kstep_golden.py [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'deeprob-kit_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from tests import test_slice_kstep_bits_gpu as t
    from deeprob.hip import load_library, slice as sl, LIB_PATH
    lib = load_library()
    prev = lib.dpk_ratspn_slice_batch_min(0)
    sl.lanes(0)
    out = {}
    for kind in t.KINDS:
        for mode in t.MODES:
            for B in t.BATCHES:
                first, again = t.evaluate(kind, B, mode)
                assert sl.last_lanes() == t.LANES.get(B, 1) and sl.last_grid() >= 1
                assert again is None or np.array_equal(first, again), (kind, mode, B)
                out[t.key(kind, B, mode)] = first
    lib.dpk_ratspn_slice_batch_min(prev)
    path = args.out or t.GOLDEN
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print('{} cases from {} -> {} ({} bytes)'.format(len(out), LIB_PATH, path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
