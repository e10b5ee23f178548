"""Golden runs of the reference's histogram column splits (deeprob/spn/learning/splitting/entropy.py, gini.py, gvs.py)
on one small continuous and one small discrete data set.  Outputs hold data only: tests/golden/learnspn_hist_cont.npz and
learnspn_hist_disc.npz with the training data, three row sets (all rows and two subsets), and per function -- entropy_cols,
entropy_adaptive_cols, gini_cols, gini_adaptive_cols, gvs_cols, rgvs_cols -- the clusters it returns on each row set and the
``save_spn_json`` text of ``learn_spn(split_cols=<the function>, split_rows='random', min_rows_slice=64)``; for the
continuous set also the G value of every column pair and numpy's 'fd' and 'scott' bin counts of every column, per row set.

Every call of the three statistics is watched (the functions are patched as gen_golden_learnspn.py patches ``gtest``), and
a learner seed is kept only if every call of its run is clear of its decision:
  * every ``(hi - lo) / width`` behind a bin count is at least 1e-3 from an integer (a float64 width differs from numpy's
    float32 one by about 1e-6 relative; at up to 100 bins that moves the quotient by 1e-4);
  * every entropy / Gini index is at least 1e-6 relative from its threshold;
  * every G is at least 1e-3 relative from its threshold, and no G-test has zero degrees of freedom (its threshold is 0 and
    its G pure rounding).
The tool asserts that the fixture decides something: the continuous G-tests come out both ways, every entropy / Gini
result on the whole matrix holds both clusters, and every learned circuit has a Product node above non-leaf children.

    cd tools && PYTHONPATH=<reference checkout> python3 gen_golden_learnspn_hist.py
"""
import io
import json
import os
import warnings

import numpy as np

from gen_golden_learnspn import CONFIGS, mixture

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, '..', 'tests', 'golden')
BIN_MARGIN, STAT_MARGIN, G_MARGIN = 1e-3, 1e-6, 1e-3
MAX_BYTES = 150 * 1000
N_ROWS, DATA_SEED = 600, 11
FUNCTIONS = ('entropy_cols', 'entropy_adaptive_cols', 'gini_cols', 'gini_adaptive_cols', 'gvs_cols', 'rgvs_cols')
#: the keyword arguments of each function per data set: thresholds between the statistics of the two kinds of column
KWARGS = {
    'cont': {'entropy_cols': {'e': 0.9}, 'entropy_adaptive_cols': {'e': 0.9, 'size': N_ROWS}, 'gini_cols': {'e': 0.75},
             'gini_adaptive_cols': {'e': 0.75, 'size': N_ROWS}, 'gvs_cols': {'p': 2.0}, 'rgvs_cols': {'p': 2.0}},
    'disc': {'entropy_cols': {'e': 1.2}, 'entropy_adaptive_cols': {'e': 1.2, 'size': 2000}, 'gini_cols': {'e': 0.55},
             'gini_adaptive_cols': {'e': 0.55, 'size': 2000}, 'gvs_cols': {'p': 5.0}, 'rgvs_cols': {'p': 5.0}},
}
#: what ``learn_spn`` gets instead: its first column splits see about half of the rows, so the adaptive thresholds are
#: referred to half the data (with the true size they would fall under every statistic and every split would be trivial)
LEARN_KWARGS = {kind: dict(kw, entropy_adaptive_cols=dict(kw['entropy_adaptive_cols'], size=kw['entropy_adaptive_cols']['size'] // 2),
                           gini_adaptive_cols=dict(kw['gini_adaptive_cols'], size=kw['gini_adaptive_cols']['size'] // 2))
                for kind, kw in KWARGS.items()}


def continuous(n_rows=N_ROWS, seed=DATA_SEED):
    """``[n_rows, 6]`` float32: two clusters; column 1 a copy of column 0 with little noise and column 2 a noisier one
    (the dependent block); column 3 independent; column 4 rounded to one decimal (values on edges, ties); column 5 heavy
    tailed (the cube of a Gaussian: most of its mass in a few of its bins)."""
    rs = np.random.RandomState(seed)
    z = rs.rand(n_rows) < 0.4
    x = np.empty((n_rows, 6))
    x[:, 0] = np.where(z, -2.0, 1.5) + rs.randn(n_rows)
    x[:, 1] = x[:, 0] + 0.05 * rs.randn(n_rows)
    x[:, 2] = 0.8 * x[:, 0] + 0.3 * rs.randn(n_rows)
    x[:, 3] = rs.randn(n_rows)
    x[:, 4] = np.round(2.0 * rs.randn(n_rows), 1)
    x[:, 5] = rs.randn(n_rows) ** 3
    return x.astype(np.float32)


def row_sets(n_rows, seed):
    """All rows, a sorted scattered subset of 257 rows and an unsorted one of 150 rows."""
    rs = np.random.RandomState(seed)
    return {'all': np.arange(n_rows), 'a': np.sort(rs.permutation(n_rows)[:257]), 'b': rs.permutation(n_rows)[:150]}


class Watch:
    """Patches ``entropy_cols``, ``gini_cols`` and ``gtest`` of the reference: the original runs, and beside it the
    margins of the call are recorded."""

    def __init__(self):
        from deeprob.spn.learning.splitting import entropy, gini, gvs
        self.mods = {'entropy': entropy, 'gini': gini, 'gvs': gvs}
        self.orig = {'entropy': entropy.entropy_cols, 'gini': gini.gini_cols, 'gvs': gvs.gtest}
        self.bins = self.stat = self.g = np.inf
        self.zero_dof = 0
        self.g_outcomes = set()

    def quotient(self, col, rule):
        from numpy.lib import _histograms_impl as impl
        width = {'scott': impl._hist_bin_scott, 'fd': impl._hist_bin_fd}[rule](col, None)
        if width and col.min() != col.max():
            q = float((col.max() - col.min()) / width)
            self.bins = min(self.bins, abs(q - round(q)))

    def stat_cols(self, which):
        from deeprob.spn.structure.leaf import LeafType

        def run(data, distributions, domains, random_state, e=0.3, alpha=0.1):
            for i in range(data.shape[1]):
                if distributions[i].LEAF_TYPE == LeafType.DISCRETE:
                    hist, _ = np.histogram(data[:, i], bins=domains[i] + [len(domains[i])])
                    norm = 1.0
                else:
                    self.quotient(data[:, i], 'scott')
                    hist, _ = np.histogram(data[:, i], bins='scott')
                    norm = np.log2(len(hist)) if len(hist) > 1 else np.nan
                probs = (hist + alpha) / (len(data) + len(hist) * alpha)
                value = -np.sum(probs * np.log2(probs)) / norm if which == 'entropy' else 1.0 - np.sum(probs ** 2.0)
                if np.isfinite(value):
                    self.stat = min(self.stat, abs(float(value) - e) / e)
            return self.orig[which](data, distributions, domains, random_state, e=e, alpha=alpha)
        return run

    def gtest(self, data, i, j, distributions, domains, p=5.0, test=True):
        from deeprob.spn.structure.leaf import LeafType
        g = self.orig['gvs'](data, i, j, distributions, domains, p, test=False)
        if not test:
            return g
        if distributions[i].LEAF_TYPE == LeafType.DISCRETE:
            b1, b2 = len(domains[i]), len(domains[j])
        else:
            for c in (i, j):
                self.quotient(data[:, c], 'fd')
            b1, b2 = (len(np.histogram_bin_edges(data[:, c], bins='fd')) - 1 for c in (i, j))
        thresh = 2.0 * (b1 - 1) * (b2 - 1) * p
        if thresh > 0:
            self.g = min(self.g, abs(float(g) - thresh) / thresh)
        else:
            self.zero_dof += 1
        self.g_outcomes.add(bool(g < thresh))
        return g < thresh

    def clear(self):
        return self.bins >= BIN_MARGIN and self.stat >= STAT_MARGIN and self.g >= G_MARGIN and self.zero_dof == 0

    def __enter__(self):
        self.mods['entropy'].entropy_cols = self.stat_cols('entropy')
        self.mods['gini'].gini_cols = self.stat_cols('gini')
        self.mods['gvs'].gtest = self.gtest
        return self

    def __exit__(self, *a):
        self.mods['entropy'].entropy_cols = self.orig['entropy']
        self.mods['gini'].gini_cols = self.orig['gini']
        self.mods['gvs'].gtest = self.orig['gvs']


def functions():
    from deeprob.spn.learning.splitting import entropy, gini, gvs
    return {name: (lambda mod, name: lambda *a, **kw: getattr(mod, name)(*a, **kw))(mod, name)
            for mod, names in ((entropy, FUNCTIONS[:2]), (gini, FUNCTIONS[2:4]), (gvs, FUNCTIONS[4:])) for name in names}


def text_of(root):
    from deeprob.spn.structure.io import save_spn_json
    buf = io.StringIO()
    save_spn_json(root, buf)
    return buf.getvalue()


def decides(spn_text):
    """Whether a circuit has a Product node with a child that is not a leaf: a column split that was not trivial."""
    g = json.loads(spn_text)
    cls = {int(n['id']): n['class'] for n in g['nodes']}
    return any(cls[int(e['target'])] == 'Product' and cls[int(e['source'])] in ('Sum', 'Product')
               for e in (g['links'] if 'links' in g else g['edges']))


def generate(kind):
    from deeprob.spn.structure.leaf import Bernoulli, Categorical, Gaussian
    from deeprob.spn.learning.learnspn import learn_spn
    from deeprob.spn.learning.splitting import gvs
    if kind == 'cont':
        data = continuous()
        dists = [Gaussian] * data.shape[1]
        domains = [(float(data[:, i].min()), float(data[:, i].max())) for i in range(data.shape[1])]
        stored, extra = data, {}
    else:
        ks, n_rows, data_seed = CONFIGS['mixed10']
        x, _ = mixture(ks, n_rows, data_seed)
        data = x.astype(np.float32)
        dists = [Bernoulli if k == 2 else Categorical for k in ks]
        domains = [list(range(k)) for k in ks]
        stored, extra = x, {'ks': np.asarray(ks, np.int32)}
    sets = row_sets(len(data), 5)
    fns = functions()
    for seed in range(42, 142):
        out = dict(extra)
        with Watch() as w, warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for name in FUNCTIONS:
                for k, (key, rows) in enumerate(sets.items()):      # (row set k is split with the seed `seed + k`)
                    out['clusters_%s_%s' % (name, key)] = np.asarray(
                        fns[name](data[rows], dists, domains, np.random.RandomState(seed + k), **KWARGS[kind][name]), np.int64)
                out['spn_json_' + name] = np.asarray(text_of(learn_spn(
                    data, dists, domains, learn_leaf='mle', split_rows='random', split_cols=fns[name],
                    split_cols_kwargs=dict(LEARN_KWARGS[kind][name]), min_rows_slice=64, random_state=seed, verbose=False)))
            both_ways = set(w.g_outcomes)
            if kind == 'cont':
                nf = data.shape[1]
                for key, rows in sets.items():
                    g = np.zeros((nf, nf))
                    for i in range(nf):
                        for j in range(i + 1, nf):
                            w.gtest(data[rows], i, j, dists, domains, p=KWARGS[kind]['gvs_cols']['p'])
                            g[i, j] = g[j, i] = gvs.gtest(data[rows], i, j, dists, domains, test=False)
                    out['g_' + key] = g
                    for rule in ('fd', 'scott'):
                        out['bins_%s_%s' % (rule, key)] = np.asarray(
                            [len(np.histogram_bin_edges(data[rows, i], bins=rule)) - 1 for i in range(nf)], np.int32)
        if not w.clear():
            print(kind, 'seed', seed, 'margins: bins %.3g stat %.3g g %.3g, %d zero-dof tests: rejected'
                  % (w.bins, w.stat, w.g, w.zero_dof))
            continue
        assert kind != 'cont' or both_ways == {True, False}, 'the continuous G-test must come out both ways: %s' % both_ways
        for name in FUNCTIONS[:4]:
            assert set(out['clusters_%s_all' % name]) == {0, 1}, (name, out['clusters_%s_all' % name])
        for name in FUNCTIONS:
            assert decides(str(out['spn_json_' + name])), name + ': every column split of the run was trivial'
        path = os.path.join(OUT, 'learnspn_hist_%s.npz' % kind)
        np.savez_compressed(path, data=stored, seed=seed, min_rows_slice=64, kwargs_json=np.asarray(json.dumps(KWARGS[kind])),
                            learn_kwargs_json=np.asarray(json.dumps(LEARN_KWARGS[kind])),
                            margin_bins=w.bins, margin_stat=w.stat, margin_g=w.g,
                            **{'rows_' + key: rows.astype(np.int32) for key, rows in sets.items()}, **out)
        size = os.path.getsize(path)
        print(kind, 'seed', seed, 'margins: bins %.3g stat %.3g g %.3g' % (w.bins, w.stat, w.g), 'nodes',
              {name: len(json.loads(str(out['spn_json_' + name]))['nodes']) for name in FUNCTIONS}, 'bytes', size)
        for name in FUNCTIONS:
            print('   ', name, {key: out['clusters_%s_%s' % (name, key)].tolist() for key in sets})
        assert size <= MAX_BYTES, 'raise min_rows_slice or shrink the data'
        return
    raise SystemExit('no seed cleared the margins for ' + kind)


if __name__ == '__main__':
    for kind in ('cont', 'disc'):
        generate(kind)
