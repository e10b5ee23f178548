"""Golden LearnSPN runs of the reference with its default column split, ``split_cols='rdc'`` (splitting/rdc.py), on small
discrete data sets.  Outputs hold data only: tests/golden/rdc_<config>.npz with the training data, the reference's
``save_spn_json`` text of ``learn_spn`` and of ``learn_estimator``, the per-row log-likelihoods of the data and of a 30 %
NaN copy, the reference's ``rdc_scores`` of the whole data with ``RandomState(0)``, the seed, the margin and the counts
of calls, pairs and deviant pairs.

The reference's score is an estimate (random features, iterative CCA) of the maximal correlation, which
tests/rdc_ref.py:maxcorr_svd computes exactly.  A run is kept only if, in every ``rdc_scores`` call it made, the two agree
on every threshold decision, (reference > d) == (closed form > d), and every closed-form score is at least 1e-4 away from
d = 0.3; otherwise the next learner seed is tried.  A pair counts as deviant when |reference - closed form| > 1e-4 (the
reference's CCA inverting a noise direction on a small slice: DESIGN.md).  For the one call on the whole data the two
must agree within 1e-4 (1e-6 for binary data); a configuration that fails this gets another data seed, not a wider bound.

    cd tools && PYTHONPATH=<reference checkout> python3 gen_golden_rdc.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, 'tests', 'golden')
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.append(p)

from gen_golden_learnspn import mixture, text_of, MAX_BYTES  # noqa: E402
from tests import rdc_ref  # noqa: E402

D, MIN_MARGIN, DEVIANT, MIN_ROWS = 0.3, 1e-4, 1e-4, 128

CONFIGS = {     # name -> (domain sizes, rows, data seed)
    'binary16': ([2] * 16, 2000, 1),
    'mixed10': ([2, 3, 5, 2, 3, 5, 2, 3, 5, 2], 2000, 3),
    'cat3x12': ([3] * 12, 3000, 2),
    'wide16': ([16, 2, 9, 16, 3, 12, 2, 16], 3000, 4),
}


class Watch:
    """Wraps the reference's rdc_scores: next to every call, the closed form on the same slice."""

    def __init__(self, rdc):
        self.rdc, self.orig = rdc, rdc.rdc_scores
        self.margin, self.calls, self.pairs, self.deviant, self.flips, self.worst = np.inf, 0, 0, 0, 0, 0.0

    def __call__(self, data, distributions, domains, random_state, **kw):
        got = np.asarray(self.orig(data, distributions, domains, random_state, **kw), np.float64)
        ks = [len(dom) for dom in domains]
        want = rdc_ref.rdc_scores(np.asarray(data).astype(np.int64), ks, np.random.RandomState(0))
        off = ~np.eye(len(ks), dtype=bool)
        self.calls += 1
        self.pairs += int(off.sum()) // 2
        self.deviant += int((np.abs(got - want)[off] > DEVIANT).sum()) // 2
        self.flips += int(((got > D) != (want > D))[off].sum()) // 2
        self.worst = max(self.worst, float(np.abs(got - want)[off].max()))
        self.margin = min(self.margin, float(np.abs(want[off] - D).min()))
        return got.astype(np.float32)

    def __enter__(self):
        self.rdc.rdc_scores = self
        return self

    def __exit__(self, *a):
        self.rdc.rdc_scores = self.orig


def generate(name):
    from deeprob.spn.structure.leaf import Bernoulli, Categorical
    from deeprob.spn.learning.learnspn import learn_spn
    from deeprob.spn.learning.wrappers import learn_estimator
    from deeprob.spn.learning.splitting import rdc
    from deeprob.spn.algorithms.inference import log_likelihood
    ks, n_rows, data_seed = CONFIGS[name]
    x, _ = mixture(ks, n_rows, data_seed)
    data = x.astype(np.float32)
    dists = [Bernoulli if k == 2 else Categorical for k in ks]
    domains = [list(range(k)) for k in ks]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        scores_ref = np.asarray(rdc.rdc_scores(data, dists, domains, np.random.RandomState(0)), np.float64)
    closed = rdc_ref.rdc_scores(x, ks, np.random.RandomState(0))
    full_err = float(np.abs(scores_ref - closed).max())
    print(name, 'whole data: max |reference - closed form| = %.3g' % full_err)
    assert full_err <= (1e-6 if max(ks) == 2 else 1e-4), 'change the data seed of this configuration'
    kw = dict(learn_leaf='mle', split_rows='random', split_cols='rdc', min_rows_slice=MIN_ROWS, verbose=False)
    for seed in range(42, 142):
        with Watch(rdc) as w, warnings.catch_warnings():
            warnings.simplefilter('ignore')
            root = learn_spn(data, dists, domains, random_state=seed, **kw)
            spn_text = text_of(root)
            calls, pairs, deviant, worst = w.calls, w.pairs, w.deviant, w.worst
            est = learn_estimator(data, dists, domains, random_state=seed, **kw)
            est_text = text_of(est)
        if w.flips or w.margin < MIN_MARGIN:
            print(name, 'seed', seed, 'margin %.3g' % w.margin, 'flips', w.flips, 'rejected')
            continue
        rs = np.random.RandomState(1000 + seed)
        mask = rs.rand(*data.shape) < 0.3
        x_nan = data.copy()
        x_nan[mask] = np.nan
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ll = np.asarray(log_likelihood(est, data), np.float64).reshape(-1)
            ll_nan = np.asarray(log_likelihood(est, x_nan), np.float64).reshape(-1)
            ll_spn = np.asarray(log_likelihood(root, data), np.float64).reshape(-1)
        path = os.path.join(OUT, 'rdc_%s.npz' % name)
        np.savez_compressed(path, data=x, ks=np.asarray(ks, np.int32), spn_json=np.asarray(spn_text),
                            est_json=np.asarray(est_text), ll=ll, ll_nan=ll_nan, ll_spn=ll_spn, nan_mask=np.packbits(mask),
                            seed=seed, data_seed=data_seed, margin=w.margin, rdc_calls=calls, rdc_pairs=pairs,
                            rdc_deviant=deviant, rdc_worst=worst, scores_ref=scores_ref, min_rows_slice=MIN_ROWS)
        size = os.path.getsize(path)
        print(name, 'seed', seed, 'margin %.3g over %d pairs of %d calls, %d deviant (worst %.3g)'
              % (w.margin, pairs, calls, deviant, worst), 'bytes', size)
        assert size <= MAX_BYTES, 'raise min_rows_slice or shrink the data'
        return
    raise SystemExit('no seed gave a margin of %g for %s' % (MIN_MARGIN, name))


if __name__ == '__main__':
    for config in (sys.argv[1:] or CONFIGS):
        generate(config)
