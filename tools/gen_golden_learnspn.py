"""Golden LearnSPN runs of the reference (deeprob/spn/learning/learnspn.py, wrappers.py) on small discrete data sets.
Outputs hold data only: tests/golden/learnspn_<config>_<split_cols>.npz with the training data, the reference's
``save_spn_json`` text of ``learn_spn`` and of ``learn_estimator`` (the pruned circuit), the per-row log-likelihoods of
the data and of a 30 % NaN copy, ``compute_data_domains`` of the data, the seeds and the G-test margin.

A run is kept only if every G-test it made is clear of its threshold: min |g - threshold| / threshold >= 1e-3 over all
calls (the reference sums 4-25 float32 terms of magnitude up to n log(..) into a g of order 10: its own rounding is of
order 1e-5 of the threshold, and a float64 evaluation must not flip a decision).  Otherwise the next learner seed is tried.

    cd tools && PYTHONPATH=<reference checkout> python3 gen_golden_learnspn.py
"""
import io
import json
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, '..', 'tests', 'golden')
MIN_MARGIN = 1e-3
MAX_BYTES = 150 * 1000

CONFIGS = {     # name -> (domain sizes, rows, data seed)
    'binary16': ([2] * 16, 2000, 1),
    'cat3x12': ([3] * 12, 3000, 2),
    'mixed10': ([2, 3, 5, 2, 3, 5, 2, 3, 5, 2], 2000, 3),
}


def mixture(ks, n_rows, seed, n_clusters=4, noise=0.2):
    """Rows of a mixture of ``n_clusters`` prototypes: a row copies its cluster's prototype, and each entry is replaced
    by a uniform value of its domain with probability ``noise``."""
    rs = np.random.RandomState(seed)
    ks = np.asarray(ks)
    protos = np.stack([rs.randint(0, ks) for _ in range(n_clusters)])
    z = rs.randint(0, n_clusters, size=n_rows)
    x = protos[z]
    flip = rs.rand(n_rows, len(ks)) < noise
    x = np.where(flip, rs.randint(0, ks, size=(n_rows, len(ks))), x)
    return x.astype(np.uint8), z


class Margin:
    """Wraps the reference's gtest: records min |g - threshold| / threshold over the calls."""

    def __init__(self, gvs):
        self.gvs, self.orig, self.value, self.calls = gvs, gvs.gtest, np.inf, 0

    def __call__(self, data, i, j, distributions, domains, p=5.0, test=True):
        if not test:
            return self.orig(data, i, j, distributions, domains, p, test=False)
        g = self.orig(data, i, j, distributions, domains, p, test=False)
        thresh = 2.0 * (len(domains[i]) - 1) * (len(domains[j]) - 1) * p
        self.calls += 1
        if thresh > 0:
            self.value = min(self.value, abs(float(g) - thresh) / thresh)
        return g < thresh

    def __enter__(self):
        self.gvs.gtest = self
        return self

    def __exit__(self, *a):
        self.gvs.gtest = self.orig


def text_of(root):
    from deeprob.spn.structure.io import save_spn_json
    buf = io.StringIO()
    save_spn_json(root, buf)
    return buf.getvalue()


def generate(name, split_cols):
    from deeprob.spn.structure.leaf import Bernoulli, Categorical
    from deeprob.spn.learning.learnspn import learn_spn
    from deeprob.spn.learning.wrappers import learn_estimator, compute_data_domains
    from deeprob.spn.learning.splitting import gvs
    from deeprob.spn.algorithms.inference import log_likelihood
    ks, n_rows, data_seed = CONFIGS[name]
    x, _ = mixture(ks, n_rows, data_seed)
    data = x.astype(np.float32)
    dists = [Bernoulli if k == 2 else Categorical for k in ks]
    domains = [list(range(k)) for k in ks]
    kw = dict(learn_leaf='mle', split_rows='random', split_cols=split_cols, min_rows_slice=64, verbose=False)
    for seed in range(42, 142):
        with Margin(gvs) as m, warnings.catch_warnings():
            warnings.simplefilter('ignore')
            root = learn_spn(data, dists, domains, random_state=seed, **kw)
            spn_text = text_of(root)
            est = learn_estimator(data, dists, domains, random_state=seed, **kw)
            est_text = text_of(est)
        if m.value < MIN_MARGIN:
            print(name, split_cols, 'seed', seed, 'margin', m.value, 'rejected')
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
        path = os.path.join(OUT, 'learnspn_%s_%s.npz' % (name, split_cols))
        np.savez_compressed(path, data=x, ks=np.asarray(ks, np.int32), spn_json=np.asarray(spn_text),
                            est_json=np.asarray(est_text), ll=ll, ll_nan=ll_nan, ll_spn=ll_spn, nan_mask=np.packbits(mask),
                            domains_json=np.asarray(json.dumps(compute_data_domains(data, dists))),
                            seed=seed, data_seed=data_seed, margin=m.value, gtest_calls=m.calls, min_rows_slice=64)
        size = os.path.getsize(path)
        print(name, split_cols, 'seed', seed, 'margin %.3g over %d g-tests' % (m.value, m.calls), 'nodes',
              len(json.loads(spn_text)['nodes']), '->', len(json.loads(est_text)['nodes']), 'bytes', size)
        assert size <= MAX_BYTES, 'raise min_rows_slice or shrink the data'
        return
    raise SystemExit('no seed gave a margin of %g for %s %s' % (MIN_MARGIN, name, split_cols))


if __name__ == '__main__':
    for config in CONFIGS:
        for cols in ('gvs', 'rgvs'):
            generate(config, cols)
