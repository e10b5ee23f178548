"""LearnSPN on continuous data, without a device: the argument checks of the all-Gaussian scope, the restatement
(tests/learn_cont_ref.py) against scipy and against itself, the host score against the restatement, and the restated score
against the scores the reference library recorded on the committed fixture (tests/golden/rdc_cont.npz, written by
tools/gen_golden_rdc_cont.py)."""
import os

import numpy as np
import pytest
import torch

from tests import learn_cont_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(n=40, m=4):
    from deeprob.spn.structure.leaf import Gaussian
    data = np.random.RandomState(0).randn(n, m).astype(np.float32)
    return data, [Gaussian] * m, [(-5.0, 5.0)] * m


# ---- argument checks (they all come before any device work) ------------------------------------------------------------------
def test_list_domains_with_gaussian_raise_value_error():
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting.rdc import rdc_scores, rdc_cols
    data, dists, doms = _args()
    bad = doms[:2] + [[0, 1]] + doms[3:]
    for call in (lambda: learn_spn(data, dists, bad, split_rows='random', split_cols='random'),
                 lambda: learn_spn(data, dists, bad, split_rows='kmeans', split_cols=rdc_cols),
                 lambda: rdc_scores(data, dists, bad, np.random.RandomState(0)),
                 lambda: rdc_cols(data, dists, bad, np.random.RandomState(0))):
        with pytest.raises(ValueError) as e:
            call()
        assert 'domain' in str(e.value)


@pytest.mark.parametrize('name', ['gvs', 'rgvs'])
def test_g_test_splits_raise_for_gaussian(name):
    from deeprob.spn.learning import learn_spn
    data, dists, doms = _args()
    with pytest.raises(NotImplementedError) as e:
        learn_spn(data, dists, doms, split_rows='random', split_cols=name)
    assert name in str(e.value) and 'table' in str(e.value)


def test_string_rdc_and_unbuilt_names_still_raise():
    from deeprob.spn.learning import learn_spn
    data, dists, doms = _args()
    with pytest.raises(NotImplementedError) as e:
        learn_spn(data, dists, doms)                                # split_cols='rdc' is the reference's default
    assert 'rdc' in str(e.value)
    for kw in (dict(split_cols='wrgvs'), dict(split_rows='gmm'), dict(learn_leaf='isotonic'), dict(split_cols=lambda *a, **k: None)):
        with pytest.raises(NotImplementedError):
            learn_spn(data, dists, doms, **dict(dict(split_rows='random', split_cols='random'), **kw))
    with pytest.raises(ValueError) as e:
        learn_spn(data, dists, doms, split_rows='random', split_cols='nope')
    assert str(e.value) == "Unknown split rows method called nope"


def test_mixed_and_uniform_still_raise():
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting.rdc import rdc_scores, rdc_cols
    from deeprob.spn.structure.leaf import Bernoulli, Gaussian, Uniform
    data, dists, doms = _args()
    data[:, 0] = data[:, 0] > 0
    for first, dom, name in ((Bernoulli, [0, 1], 'Gaussian'), (Uniform, (-5.0, 5.0), 'Uniform')):
        d2, m2 = [first] + dists[1:], [dom] + doms[1:]
        for call in (lambda: learn_spn(data, d2, m2, split_rows='random', split_cols='random'),
                     lambda: learn_spn(data, d2, m2, split_rows='random', split_cols=rdc_cols),
                     lambda: rdc_scores(data, d2, m2, np.random.RandomState(0))):
            with pytest.raises(NotImplementedError) as e:
                call()
            assert name in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        learn_spn(data, [Uniform] * 4, doms, split_rows='random', split_cols='random')
    assert 'Uniform' in str(e.value)


@pytest.mark.parametrize('kw', [dict(split_rows_kwargs={'nope': 1}), dict(split_cols_kwargs={'p': 5.0}),
                                dict(learn_leaf_kwargs={'nope': 1}), dict(split_rows='random', split_rows_kwargs={'n': 2}),
                                dict(split_cols='random', split_cols_kwargs={'d': 0.3})])
def test_unknown_keywords_raise_type_error(kw):
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting.rdc import rdc_cols
    data, dists, doms = _args()
    with pytest.raises(TypeError):
        learn_spn(data, dists, doms, **dict(dict(split_rows='kmeans', split_cols=rdc_cols), **kw))


@pytest.mark.parametrize('change, message', [
    (dict(domains=[]), "The list of domains must be non-empty"),
    (dict(min_rows_slice=0), "The minimum number of samples required to split horizontally must be positive"),
    (dict(min_cols_slice=0), "The minimum number of samples required to split vertically must be positive"),
    (dict(domains=[(-5.0, 5.0)] * 3), "Each data column should correspond to a random variable having a distribution and a domain"),
    (dict(split_rows='nope'), "Unknown split rows method called nope"),
    (dict(split_rows_kwargs={'n': 9}), "k-means on the HIP path takes 1..8 clusters"),
])
def test_argument_errors_match_the_reference(change, message):
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting.rdc import rdc_cols
    data, dists, doms = _args()
    kw = dict(distributions=dists, domains=doms, split_rows='kmeans', split_cols=rdc_cols)
    kw.update(change)
    with pytest.raises(ValueError) as e:
        learn_spn(data, **kw)
    assert str(e.value) == message


@pytest.mark.parametrize('bad', [dict(k=0), dict(k=2.5), dict(s=0.0), dict(s=-1.0), dict(d=float('nan'))])
def test_rdc_parameters_are_checked(bad):
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting.rdc import rdc_cols
    data, dists, doms = _args()
    with pytest.raises(ValueError):
        learn_spn(data, dists, doms, split_rows='random', split_cols=rdc_cols, split_cols_kwargs=bad)
    with pytest.raises(ValueError):
        rdc_cols(data, dists, doms, np.random.RandomState(0), **bad)


@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf])
def test_nan_and_inf_raise_and_nothing_is_modified(value):
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting.rdc import rdc_scores
    data, dists, doms = _args()
    data[3, 1] = value
    before = data.copy()
    for call in (lambda: learn_spn(data, dists, doms, split_rows='random', split_cols='random'),
                 lambda: rdc_scores(data, dists, doms, np.random.RandomState(0))):
        with pytest.raises(ValueError) as e:
            call()
        assert 'NaN or inf' in str(e.value)
    assert np.array_equal(data, before, equal_nan=True)


def test_cpu_tensor_raises_hip_error():
    from deeprob.hip import HipError
    from deeprob.spn.learning import learn_spn, learn_estimator
    from deeprob.spn.learning.splitting.rdc import rdc_scores
    data, dists, doms = _args()
    for call in (lambda: learn_spn(torch.from_numpy(data), dists, doms, split_rows='random', split_cols='random'),
                 lambda: learn_estimator(torch.from_numpy(data), dists, doms, split_rows='random', split_cols='random'),
                 lambda: learn_estimator(torch.from_numpy(data), dists, split_rows='random', split_cols='random'),
                 lambda: rdc_scores(torch.from_numpy(data), dists, doms, np.random.RandomState(0))):
        with pytest.raises(HipError):
            call()


def test_abi_version_and_the_new_entries_are_declared():
    from deeprob.hip import learn
    for name in ('dpl_column_moments', 'dpl_ecdf_ranks', 'dpl_rdc_gram', 'dpl_kmeansf_init', 'dpl_kmeansf_assign',
                 'dpl_kmeansf_update', 'dpl_kmeansf_inertia'):
        assert name in learn.SIGNATURES
    assert learn.DPL_GRAM_PARTIAL == learn.DPL_GRAM_TILE * learn.DPL_GRAM_TILE + learn.DPL_GRAM_TILE
    assert learn.GRAM_MAX_UNITS * learn.DPL_GRAM_PARTIAL * 8 <= 256 << 20
    assert learn.load_library().dpl_abi_version() >= 3


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_restated_ranks_are_scipys_max_ranks():
    stats = pytest.importorskip('scipy.stats')
    rs = np.random.RandomState(1)
    for n in (1, 2, 255, 300):
        for col in (rs.randn(n), np.round(rs.randn(n), 1), np.zeros(n), rs.randint(0, 3, size=n).astype(np.float64)):
            assert np.array_equal(ref.ranks(col), stats.rankdata(col, method='max').astype(np.int64))


def test_restated_moments_are_numpys():
    rs = np.random.RandomState(2)
    for n in (1, 255, 256, 257, 300, 1000):
        col = ref.as_device(rs.randn(n) * 3.0 + 100.0)
        mean, var = ref.moments(col)
        assert abs(mean - col.mean()) <= 1e-12 * abs(col.mean()) and abs(var - col.var()) <= 1e-12 * max(col.var(), 1e-300)
    assert ref.moments(np.full(300, 0.1))[1] <= ref.ZERO_VARIANCE


def test_host_score_is_the_restated_score():
    """splitting.rdc.scores_from_gram and the restatement are the same algebra written twice; both form W_p with entries
    near 1 / sqrt(lam), so they agree to rounding times that magnification, far inside the 1e-7 the ridge allows."""
    from deeprob.spn.learning.splitting import rdc as R
    x = ref.as_device(ref.two_blocks())
    x[:, 2] = 1.5                                                      # a constant column scores 0
    w, b = ref.draw_features(np.random.RandomState(3), 6, 20, 1.0 / 6.0)
    w2, b2 = R.draw_features(np.random.RandomState(3), 6, 20, 1.0 / 6.0)
    assert np.array_equal(w, w2) and np.array_equal(b, b2) and w.dtype == np.float32
    rk = np.stack([ref.ranks(x[:, p]) for p in range(6)], axis=1)
    S, G = ref.gram(ref.features(rk, w, b))
    want, got = ref.scores_from_gram(G, S, 300, 6, 20), R.scores_from_gram(G, S, 300, 6, 20)
    print('largest difference of the two host forms', float(np.abs(got - want).max()))
    assert np.abs(got - want).max() <= 1e-8
    assert np.all(got[2, [0, 1, 3, 4, 5]] == 0.0) and np.all(np.diag(got) == 1.0) and np.array_equal(got, got.T)
    assert got[0, 1] > 0.9 and got[3, 4] > 0.9
    assert np.array_equal(R.components(got > 0.3), ref.components(want > 0.3))


def test_score_is_continuous_in_the_gram_matrix():
    """The ridge makes the score a continuous function of G.  Two summation orders of a raw Gram entry differ by at most
    (n + 8) * n * 2^-53 (the bound of the device test); a perturbation of every entry by up to that much must stay below
    the 1e-6 at which a deviation of the device from the restatement would count as a finding."""
    n = 300
    x = ref.as_device(ref.two_blocks(n, seed=4))
    w, b = ref.draw_features(np.random.RandomState(5), 6, 20, 1.0 / 6.0)
    rk = np.stack([ref.ranks(x[:, p]) for p in range(6)], axis=1)
    S, G = ref.gram(ref.features(rk, w, b))
    noise = np.random.RandomState(6).uniform(-1.0, 1.0, size=G.shape) * (n + 8) * n * 2.0 ** -53
    noise = (noise + noise.T) / 2
    moved = np.abs(ref.scores_from_gram(G + noise, S, n, 6, 20) - ref.scores_from_gram(G, S, n, 6, 20)).max()
    print('largest score change under a worst-case rounding perturbation of G', float(moved))
    assert moved <= 1e-6


@pytest.mark.parametrize('case', ['n2000', 'n300', 'n64'])
def test_threshold_decisions_against_the_reference_fixture(case):
    """The restated ridge score against the reference's recorded ``rdc_scores`` (iterative CCA): the distances are printed
    (and recorded in DESIGN.md, "rdc on continuous columns"), not asserted; asserted is the decision ``score > 0.3`` on the
    fixture's pairs, which were chosen with both values at least 0.1 from 0.3."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'rdc_cont.npz'))
    rows, theirs, pairs, d = g[case + '_rows'], g[case + '_reference'], g[case + '_pairs'], float(g['d'])
    ours = ref.rdc_scores_with(ref.as_device(rows), g[case + '_w'], g[case + '_b'])
    ia, ib = np.triu_indices(rows.shape[1], 1)
    print(case, 'largest |restated - reference| over all pairs', float(np.abs(ours - theirs)[ia, ib].max()))
    assert len(pairs) >= 3
    for i, j in pairs:
        print(case, (int(i), int(j)), 'reference', float(theirs[i, j]), 'restated', float(ours[i, j]))
        assert abs(theirs[i, j] - d) >= 0.1 and abs(ours[i, j] - d) >= 0.1
        assert (ours[i, j] > d) == (theirs[i, j] > d)


def test_restated_loop_meets_the_preconditions_of_the_device_test():
    """The seed of the end-to-end device test: every score decision at least 1e-3 from d, no k-means distance tie."""
    root, stats = ref.e2e_restated()
    print(ref.E2E, stats)
    assert stats['margin'] >= 1e-3 and stats['gap'] >= 1e-9
    assert root['class'] == 'Sum' and len(root['children']) == 2
