"""The Gaussian-mixture row split without a device: the public surface (module paths, signatures, ``split_rows_clusters``),
the draws, the argument errors that come before any device work, the restated EM (tests/learn_gmm_ref.py) against
scikit-learn from the same initial parameters, and the preconditions of the end-to-end cases of
tests/test_learn_gmm_gpu.py on the restatement alone."""
import inspect

import numpy as np
import pytest
import torch

from tests import learn_gmm_ref as ref


def problem(kind='binary'):
    from deeprob.spn.structure.leaf import Bernoulli, Gaussian
    if kind == 'binary':
        return ref.binary16(60), [Bernoulli] * 16, [[0, 1]] * 16
    return ref.three_floats(60), [Gaussian] * 3, [(-10.0, 10.0)] * 3


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_module_paths_signatures_and_defaults_are_the_references():
    from deeprob.spn.learning.splitting import cluster, rows
    import deeprob.spn.learning.splitting as splitting
    # reference splitting/cluster.py:14-20, 41-47 and splitting/rows.py:23-26: names, kinds and defaults
    for fn in (cluster.gmm, cluster.kmeans):
        params = inspect.signature(fn).parameters
        assert list(params) == ['data', 'distributions', 'domains', 'random_state', 'n']
        assert all(p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params.values())
        assert [p.default for p in params.values()] == [inspect.Parameter.empty] * 4 + [2]
    params = inspect.signature(rows.split_rows_clusters).parameters
    assert list(params) == ['data', 'clusters'] and all(p.default is inspect.Parameter.empty for p in params.values())
    assert splitting.gmm is cluster.gmm and splitting.kmeans is cluster.kmeans
    assert splitting.split_rows_clusters is rows.split_rows_clusters
    for name in ('kmeans_mb', 'dbscan', 'wald'):
        assert not hasattr(cluster, name) and name in cluster.__doc__, 'named in the module docstring as not built'


def test_split_rows_clusters_gives_the_references_slices_and_weights():
    from deeprob.spn.learning.splitting.rows import split_rows_clusters
    data = np.arange(21).reshape(7, 3)
    clusters = np.array([2, 0, 2, 5, 0, 2, 2])
    slices, weights = split_rows_clusters(data, clusters)
    # what reference rows.py:35-43 gives: the clusters in increasing order, rows in data order, shares of the rows
    assert isinstance(slices, list) and isinstance(weights, list) and len(slices) == 3
    assert np.array_equal(slices[0], data[[1, 4]]) and np.array_equal(slices[1], data[[0, 2, 5, 6]])
    assert np.array_equal(slices[2], data[[3]])
    assert weights == [2 / 7, 4 / 7, 1 / 7]
    slices, weights = split_rows_clusters(data, np.zeros(7, np.int64))
    assert len(slices) == 1 and np.array_equal(slices[0], data) and weights == [1.0]


class CountingState(np.random.RandomState):
    def __init__(self, seed):
        super().__init__(seed)
        self.calls = []

    def choice(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return super().choice(*args, **kwargs)


def test_the_draws_are_three_choices_per_task(monkeypatch):
    """``gmm`` draws ``choice(n, C, replace=False)`` three times (``kmeans`` five) and nothing else before the device is
    needed; the restatement draws the same."""
    from deeprob.spn.learning.splitting import cluster
    from deeprob.spn.learning import learnspn
    data, dists, doms = problem()

    class Stop(Exception):
        pass

    def no_device(self, *a, **k):
        raise Stop()
    monkeypatch.setattr(learnspn.DiscreteColumns, 'gmm_batch', no_device)
    monkeypatch.setattr(learnspn.DiscreteColumns, 'kmeans_batch', no_device)
    monkeypatch.setattr(learnspn.DiscreteColumns, 'upload', lambda self, d: type('D', (), dict(
        n_rows=d.shape[0], n_cols=d.shape[1], device=torch.device('cpu')))())
    for fn, draws in ((cluster.gmm, 3), (cluster.kmeans, 5)):
        rs = CountingState(4)
        with pytest.raises(Stop):
            fn(data, dists, doms, rs, n=3)
        assert len(rs.calls) == draws and all(a == (60, 3) and k == {'replace': False} for a, k in rs.calls)
    rs, twin = CountingState(4), np.random.RandomState(4)
    ref.gmm(data, [2] * 16, rs, 3)
    assert len(rs.calls) == 3
    for _ in range(3):
        twin.choice(60, 3, replace=False)
    assert rs.randint(1 << 30) == twin.randint(1 << 30), 'nothing else was drawn'


# ---- errors before any device work -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['binary', 'float'])
def test_argument_errors_come_before_any_device_work(kind, monkeypatch):
    from deeprob.hip import HipError, learn as L
    from deeprob.spn.learning import learn_spn, learn_estimator
    from deeprob.spn.learning.splitting import gmm, kmeans
    from deeprob.spn.structure.leaf import Bernoulli, Gaussian, Uniform
    monkeypatch.setattr(L, 'upload', lambda *a, **k: pytest.fail('a table was uploaded'))
    data, dists, doms = problem(kind)
    rs = np.random.RandomState(0)
    for fn in (gmm, kmeans):
        for n in (0, 9):
            with pytest.raises(ValueError, match='takes 1..8 clusters'):
                fn(data, dists, doms, rs, n=n)
            with pytest.raises(ValueError, match='takes 1..8 clusters'):
                learn_spn(data, dists, doms, split_rows=fn, split_cols='random', split_rows_kwargs={'n': n})
        with pytest.raises(TypeError, match="unexpected keyword argument 'a'"):
            learn_spn(data, dists, doms, split_rows=fn, split_cols='random', split_rows_kwargs={'a': 2.0})
        mixed = [Gaussian if kind == 'binary' else Bernoulli] + dists[1:]
        mixed_doms = [(0.0, 1.0) if kind == 'binary' else [0, 1]] + doms[1:]
        for bad, bad_doms in ((mixed, mixed_doms), ([Uniform] * len(dists), [(0.0, 1.0)] * len(dists))):
            with pytest.raises(NotImplementedError):
                fn(data, bad, bad_doms, rs)
            with pytest.raises(NotImplementedError):
                learn_spn(data, bad, bad_doms, split_rows=fn, split_cols='random')
        with pytest.raises(ValueError, match='should be >= n_clusters'):
            fn(data[:2], dists, doms, rs, n=3)
        with pytest.raises(HipError, match='no CPU fallback'):
            fn(torch.from_numpy(data), dists, doms, rs)
        for learner in (learn_spn, learn_estimator):
            with pytest.raises(HipError, match='no CPU fallback'):
                learner(torch.from_numpy(data), dists, doms, split_rows=fn, split_cols='random')
    assert rs.randint(1 << 30) == np.random.RandomState(0).randint(1 << 30), 'no draw was made'


def test_the_strings_and_other_callables_still_raise():
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting import gmm
    data, dists, doms = problem()
    for name in ('gmm', 'kmeans_mb', 'dbscan', 'wald', 'rdc'):
        with pytest.raises(NotImplementedError, match='not built'):
            learn_spn(data, dists, doms, split_rows=name, split_cols='random')
    for fn in (lambda *a, **k: gmm(*a, **k), np.argmax, inspect.signature):
        with pytest.raises(NotImplementedError, match='custom split_rows function'):
            learn_spn(data, dists, doms, split_rows=fn, split_cols='random')
    with pytest.raises(ValueError, match='Unknown split rows method called nope'):
        learn_spn(data, dists, doms, split_rows='nope', split_cols='random')


def test_the_host_m_step_of_the_binding_is_the_restated_one():
    """``deeprob.hip.learn.gmm_m_step`` on moments about a pivot gives the parameters of the restated M-step."""
    from deeprob.hip import learn as L
    rs = np.random.RandomState(0)
    X = np.concatenate([rs.randn(80, 4), 1000.0 + rs.randn(80, 1)], axis=1)
    r = rs.dirichlet([1.0, 1.0, 1.0], size=80)
    pivot = X[:3] + 0.01
    stats = np.stack([ref.mstats_entry(X, r[:, c], pivot[c])[0] for c in range(3)])
    got = L.gmm_m_step(stats, pivot, 80)
    want = ref.pack(*ref.m_step(X, r))
    scale = np.maximum(np.abs(want), 1.0)
    assert np.max(np.abs(got - want) / scale) <= 1e-9, float(np.max(np.abs(got - want) / scale))
    with pytest.raises(ValueError, match='ill-defined empirical covariance'):
        L.gmm_m_step(np.concatenate([[[1.0]], np.zeros((1, 2)), -np.ones((1, 4))], axis=1), np.zeros((1, 2)), 4)


# ---- the restated loop is scikit-learn's -----------------------------------------------------------------------------------------
SKLEARN_CASES = {'float_with_offset_column': (None, 2, 0), 'binary_c2': ([2] * 9, 2, 1), 'binary_c3': ([2] * 9, 3, 2)}


@pytest.mark.parametrize('name', sorted(SKLEARN_CASES))
def test_restated_loop_matches_sklearn_from_the_same_parameters(name):
    mixture = pytest.importorskip('sklearn.mixture')
    ks, C, seed = SKLEARN_CASES[name]
    rs = np.random.RandomState(seed)
    if ks is None:
        z = rs.rand(300) < 0.5
        data = np.where(z[:, None], rs.randn(300, 6) * [1, .3, 2, 1, 1, 1], rs.randn(300, 6) * [.4, 1.5, .5, 1, 1, 1] + [3, -2, 1, 0, 0, 0])
        data[:, 5] = 1000.0 + rs.randn(300)                       # the column an expanded quadratic form cancels on
        data = data.astype(np.float32)
    else:
        data = ref.disc.mixture(ks, 300, seed, n_clusters=C, noise=0.2)[0]
    X = ref.features(data, ks)
    labels, _ = ref.lloyd(data, ks, rs.choice(len(data), C, replace=False), C)
    stats = {}
    run = ref.em(X, ref.one_hot(labels, C), stats)
    pi, mu, sigma = ref.m_step(X, ref.one_hot(labels, C))
    sk = mixture.GaussianMixture(C, covariance_type='full', tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, weights_init=pi,
                                 means_init=mu, precisions_init=np.stack([np.linalg.inv(s) for s in sigma]))
    sk_labels = sk.fit_predict(X)
    print(name, 'iterations', run['n_iter'], sk.n_iter_, 'bound', run['lower'], sk.lower_bound_, stats)
    assert run['n_iter'] == sk.n_iter_ and run['n_iter'] >= 2
    assert abs(run['lower'] - sk.lower_bound_) <= 1e-9 * max(1.0, abs(sk.lower_bound_))
    assert np.max(np.abs(run['mu'] - sk.means_) / np.maximum(np.abs(sk.means_), 1.0)) <= 1e-9
    assert np.array_equal(run['labels'], sk_labels)


# ---- the preconditions of the end-to-end GPU cases, on the restatement alone ----------------------------------------------------------
@pytest.mark.parametrize('which', ['float', 'binary'])
def test_standalone_cases_meet_their_preconditions(which):
    data, ks, lab, km, stats = ref.standalone(which)
    print(which, stats, np.bincount(lab), np.bincount(km))
    assert ref.preconditions(stats), stats
    assert len(np.unique(lab)) == ref.STANDALONE[which]['n'] and stats['iterations'] >= 2


def test_end_to_end_cases_meet_their_preconditions():
    for name, (root, stats) in (('two_blocks', ref.e2e_cont()), ('binary16', ref.e2e_disc())):
        print(name, stats, len(ref.disc.topological_order(root)), 'nodes')
        assert ref.preconditions(stats), (name, stats)
        assert stats.get('margin', 1.0) >= 1e-3, 'every RDC decision lies 1e-3 from its threshold'
        classes = {nd['class'] for nd in ref.disc.topological_order(root)}
        assert {'Sum', 'Product'} <= classes and stats['iterations'] >= 2
