"""Golden vectors for the moments of node-graph SPNs: the reference's ``deeprob.spn.algorithms.moments`` runs on its own
JSON exports under tests/golden/ (tools/gen_golden_spn.py).  The output holds recorded results only:
tests/golden/spn_moments.npz with, per circuit, ``<name>.moment<k>`` (k = 1..4), ``<name>.variance`` and
``<name>.kurtosis``, each ``[n_features]`` float32.  ``skewness`` is left out on purpose: the reference's line 86 adds
where the third central moment subtracts (see deeprob/spn/algorithms/moments.py of this package).

    cd tools && PYTHONPATH=<reference checkout> python3 gen_golden_spn_moments.py
"""
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, '..', 'tests', 'golden')
CIRCUITS = ('binary16', 'mixed4')


def main():
    from deeprob.spn.structure.io import load_spn_json
    from deeprob.spn.algorithms.moments import moment, variance, kurtosis
    out = {}
    for name in CIRCUITS:
        root = load_spn_json(os.path.join(OUT, 'spn_%s.json' % name))
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for k in (1, 2, 3, 4):
                out['%s.moment%d' % (name, k)] = np.asarray(moment(root, k), np.float32)
            out['%s.variance' % name] = np.asarray(variance(root), np.float32)
            out['%s.kurtosis' % name] = np.asarray(kurtosis(root), np.float32)
        print(name, 'expectation', out['%s.moment1' % name], 'variance', out['%s.variance' % name])
    np.savez_compressed(os.path.join(OUT, 'spn_moments.npz'), **out)


if __name__ == '__main__':
    main()
