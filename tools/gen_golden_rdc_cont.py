"""Generate tests/golden/rdc_cont.npz: small continuous data sets, the RDC draws and the scores the REFERENCE library
gives on them (deeprob/spn/learning/splitting/rdc.py:rdc_scores, scikit-learn's iterative CCA), next to this project's
restated ridge score (tests/learn_cont_ref.py).  Needs the reference tree, scipy and scikit-learn:

    python tools/gen_golden_rdc_cont.py --reference /path/to/deeprob-kit

Per case it prints both score matrices and their largest difference (the table of DESIGN.md, "rdc on continuous columns")
and records the pairs on which BOTH values lie at least 0.1 from the threshold 0.3: only those enter the test
(tests/test_learn_cont_host.py), which asserts the threshold decision and prints the distances.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
K, S, D_THRESHOLD, MARGIN = 20, 1.0 / 6.0, 0.3, 0.1


def case_data(name):
    """Columns 0, 1 strongly dependent (1 a noisy nonlinear image of 0), 2 a weaker image of 0, 3 and 4 independent."""
    n, seed = {'n2000': (2000, 11), 'n300': (300, 12), 'n64': (64, 13)}[name]
    rs = np.random.RandomState(seed)
    a = rs.randn(n)
    x = np.stack([a, np.tanh(a) + 0.3 * rs.randn(n), a * a + 0.5 * rs.randn(n), rs.randn(n), rs.rand(n)], axis=1)
    x[::7, 4] = 0.5                # ties
    return x.astype(np.float32), seed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='the root of the reference deeprob-kit tree')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'rdc_cont.npz'))
    args = ap.parse_args()
    from tests import learn_cont_ref as ref
    sys.path.insert(0, args.reference)
    from deeprob.spn.learning.splitting.rdc import rdc_scores
    from deeprob.spn.structure.leaf import Gaussian
    out = {'k': K, 's': S, 'd': D_THRESHOLD}
    for name in ('n2000', 'n300', 'n64'):
        x, seed = case_data(name)
        m = x.shape[1]
        domains = [(float(x[:, i].min()), float(x[:, i].max())) for i in range(m)]
        theirs = np.asarray(rdc_scores(x, [Gaussian] * m, domains, np.random.RandomState(seed), k=K, s=S), np.float64)
        w, b = ref.draw_features(np.random.RandomState(seed), m, K, S)
        ours = ref.rdc_scores_with(ref.as_device(x), w, b)
        ia, ib = np.triu_indices(m, 1)
        keep = (np.abs(theirs[ia, ib] - D_THRESHOLD) >= MARGIN) & (np.abs(ours[ia, ib] - D_THRESHOLD) >= MARGIN)
        print(name, 'reference\n', np.round(theirs, 3), '\nrestated ridge score\n', np.round(ours, 3))
        print(name, 'largest |difference|', float(np.abs(theirs - ours)[ia, ib].max()), 'pairs kept', int(keep.sum()), 'of', len(ia))
        out.update({name + '_rows': x, name + '_w': w, name + '_b': b, name + '_reference': theirs,
                    name + '_pairs': np.stack([ia[keep], ib[keep]], axis=1).astype(np.int32)})
    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
