"""RDC column splits without a device: the numpy restatement (tests/rdc_ref.py) against the reference's golden graphs
and scores, its two evaluations of the maximal correlation against each other and against hand tables, and the argument
handling of ``deeprob.spn.learning.splitting.rdc`` and of ``learn_spn(..., split_cols=rdc_cols)``."""
import json
import os

import numpy as np
import pytest
import torch

from tests import learnspn_ref as ref
from tests import rdc_cases as cases
from tests import rdc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CONFIGS = ['binary16', 'mixed10', 'cat3x12', 'wide16']

_cache = {}


def golden(name):
    if name not in _cache:
        g = np.load(os.path.join(GOLDEN, 'rdc_%s.npz' % name))
        _cache[name] = {k: g[k] for k in g.files}
    return _cache[name]


def names_of(ks):
    return ['Bernoulli' if k == 2 else 'Categorical' for k in ks]


def score_bound(ks):
    """|reference - exact| over all rows of a fixture: the float32 the reference stores for binary data, its own spread
    between two RandomStates (2e-6 measured) with a margin for categorical data."""
    return 1e-6 if max(ks) == 2 else 1e-4


# ---- the restatement against the fixtures -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CONFIGS)
def test_fixture_margin(name):
    g = golden(name)
    assert float(g['margin']) >= 1e-4 and int(g['rdc_calls']) > 0 and int(g['rdc_pairs']) > 0


@pytest.mark.parametrize('name', CONFIGS)
def test_restatement_reproduces_reference_graphs(name):
    g = golden(name)
    ks = [int(k) for k in g['ks']]
    stats = {}
    root = rdc_ref.learn_spn(g['data'], names_of(ks), ks, split_rows='random', min_rows_slice=int(g['min_rows_slice']),
                             random_state=int(g['seed']), stats=stats)
    assert stats['calls'] == int(g['rdc_calls']) and abs(stats['margin'] - float(g['margin'])) <= 1e-12
    assert ref.graphs_differ(ref.to_digraph(root), json.loads(str(g['spn_json']))) is None
    assert ref.graphs_differ(ref.to_digraph(ref.prune(root)), json.loads(str(g['est_json']))) is None


@pytest.mark.parametrize('name', CONFIGS)
def test_svd_scores_against_the_reference(name):
    g = golden(name)
    ks = [int(k) for k in g['ks']]
    got = rdc_ref.rdc_scores(g['data'], ks, np.random.RandomState(0))
    err = float(np.abs(got - g['scores_ref']).max())
    print(name, 'max |exact - reference| over all rows', err)
    assert err <= score_bound(ks)
    assert np.array_equal(np.diag(got), np.ones(len(ks)))


def test_jacobi_order_against_svd_on_the_device_tables():
    tables = cases.kernel_case()['tables']
    svd = np.array([rdc_ref.maxcorr_svd(t) for t in tables])
    jac = np.array([rdc_ref.maxcorr_jacobi(t) for t in tables])
    print('tables', len(tables), 'max |jacobi - svd|', float(np.abs(jac - svd).max()))
    assert np.all(np.abs(jac - svd) <= 1e-12) and np.all((jac >= 0.0) & (jac <= 1.0))
    assert len(np.unique(np.round(svd, 6))) > 30, 'the tables must not be degenerate'


@pytest.mark.parametrize('name, table, want', cases.hand_tables(), ids=[h[0] for h in cases.hand_tables()])
def test_hand_tables(name, table, want):
    for fn in (rdc_ref.maxcorr_svd, rdc_ref.maxcorr_jacobi):
        got = fn(table)
        assert abs(got - want) <= 1e-12 and 0.0 <= got <= 1.0, (fn.__name__, got)
        assert abs(fn(table.T) - want) <= 1e-12
    if name.startswith('one present value'):
        assert rdc_ref.maxcorr_jacobi(table) == 0.0


def test_rows_of_inverts_joint_counts():
    for _, table, _ in cases.hand_tables():
        rows = cases.rows_of(table)
        assert np.array_equal(rdc_ref.joint_counts(rows[:, 0], rows[:, 1], *table.shape), table)


def test_components_are_numbered_by_their_smallest_member():
    from deeprob.spn.learning.splitting.rdc import components
    adj = np.zeros((6, 6), bool)
    for a, b in ((0, 4), (4, 2), (1, 5)):
        adj[a, b] = adj[b, a] = True
    want = [0, 1, 0, 2, 0, 1]
    assert components(adj).tolist() == want == rdc_ref.components(adj).tolist()
    assert components(adj).dtype == np.int32


# ---- the interface ---------------------------------------------------------------------------------------------------------
def _args(ks=(2, 3, 5, 2)):
    from deeprob.spn.structure.leaf import Bernoulli, Categorical
    rs = np.random.RandomState(0)
    data = rs.randint(0, np.asarray(ks), size=(50, len(ks))).astype(np.float32)
    return data, [Bernoulli if k == 2 else Categorical for k in ks], [list(range(k)) for k in ks]


@pytest.fixture
def host_device(monkeypatch):
    """Stands in for the device: ``_to_device`` keeps the checked data on the host and ``pair_maxcorr`` is the SVD
    restatement, so that the host logic of ``rdc_scores`` / ``rdc_cols`` runs without a GPU."""
    from deeprob.hip import learn as L
    from deeprob.spn.learning import learnspn

    class Host:
        def __init__(self, data):
            self.x, (self.n_rows, self.n_cols), self.device = np.asarray(data).astype(np.int64), data.shape, 'cpu'

    def to_device(data, ks):
        assert not np.isnan(data).any() and ((data >= 0) & (data < np.asarray(ks)[None, :])).all()
        return Host(data)

    def pair_maxcorr(data, row_index, col_i, col_j, row_off, n, ki, kj):
        rows = row_index.numpy()
        return np.array([rdc_ref.maxcorr_svd(rdc_ref.joint_counts(data.x[rows[o:o + m], a], data.x[rows[o:o + m], b], ka, kb))
                         for a, b, o, m, ka, kb in zip(col_i, col_j, row_off, n, ki, kj)])

    monkeypatch.setattr(learnspn, '_to_device', to_device)
    monkeypatch.setattr(L, 'load_library', lambda: None)
    monkeypatch.setattr(L, 'pair_maxcorr', pair_maxcorr)
    monkeypatch.setattr(L, 'read', lambda t, lloyd=False: t)


def test_module_path_and_signatures():
    import inspect
    from deeprob.spn.learning import splitting
    from deeprob.spn.learning.splitting import rdc
    assert splitting.rdc_cols is rdc.rdc_cols and splitting.rdc_scores is rdc.rdc_scores
    assert list(inspect.signature(rdc.rdc_scores).parameters) == ['data', 'distributions', 'domains', 'random_state', 'k', 's']
    assert list(inspect.signature(rdc.rdc_cols).parameters) == ['data', 'distributions', 'domains', 'random_state', 'd', 'k', 's']
    defaults = {k: p.default for k, p in inspect.signature(rdc.rdc_cols).parameters.items() if p.default is not p.empty}
    assert defaults == {'d': 0.3, 'k': 20, 's': 1.0 / 6.0}
    for name in ('rdc_rows', 'rdc_transform', 'rdc_cca'):
        assert not hasattr(rdc, name) and name in rdc.__doc__


def test_scores_and_cols_on_the_host_stand_in(host_device):
    from deeprob.spn.learning.splitting.rdc import rdc_scores, rdc_cols
    data, dists, doms = _args()
    data[:, 3] = (data[:, 1] > 0)                      # columns 1 and 3 dependent, 0 and 2 on their own
    ks = [len(d) for d in doms]
    got = rdc_scores(data, dists, doms, np.random.RandomState(1))
    want = rdc_ref.rdc_scores(data, ks, np.random.RandomState(1))
    assert got.dtype == np.float64 and got.shape == (4, 4) and np.array_equal(got, want)
    assert np.array_equal(np.diag(got), np.ones(4)) and np.array_equal(got, got.T)
    labels = rdc_cols(data, dists, doms, np.random.RandomState(1), d=0.6)
    assert labels.tolist() == rdc_ref.components(want > 0.6).tolist() == [0, 1, 2, 1]


@pytest.mark.parametrize('ks, k', [((2, 3, 5, 2), 20), ((16, 2, 9), 15), ((2, 2), 1)])
def test_random_state_is_consumed_as_the_reference_consumes_it(host_device, ks, k):
    from deeprob.spn.learning.splitting.rdc import rdc_scores, rdc_cols
    data, dists, doms = _args(ks)
    for fn in (rdc_scores, rdc_cols):
        got, want = np.random.RandomState(7), np.random.RandomState(7)
        fn(data, dists, doms, got, k=k)
        for K in ks:                                    # rdc.py:170-176
            want.randn(K, k)
            want.randn(k)
        assert got.randint(0, 2 ** 31 - 1, size=4).tolist() == want.randint(0, 2 ** 31 - 1, size=4).tolist()


def test_k_too_small_raises_with_the_reason():
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting.rdc import rdc_scores, rdc_cols
    data, dists, doms = _args((2, 16, 3))
    for call in (lambda: rdc_scores(data, dists, doms, np.random.RandomState(0), k=14),
                 lambda: rdc_cols(data, dists, doms, np.random.RandomState(0), k=14),
                 lambda: learn_spn(data, dists, doms, split_rows='random', split_cols=rdc_cols, split_cols_kwargs={'k': 14})):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert 'rank limited' in str(e.value) and 'depends on the random draws' in str(e.value)


def test_nl_and_unknown_keywords_are_rejected():
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting.rdc import rdc_scores, rdc_cols
    data, dists, doms = _args()
    for fn in (rdc_scores, rdc_cols):
        for kw in ({'nl': np.sin}, {'p': 5.0}):
            with pytest.raises(TypeError) as e:
                fn(data, dists, doms, np.random.RandomState(0), **kw)
            assert 'unexpected keyword' in str(e.value)
    for kw in ({'nl': np.sin}, {'p': 5.0}, {'n': 2}):
        with pytest.raises(TypeError) as e:
            learn_spn(data, dists, doms, split_rows='random', split_cols=rdc_cols, split_cols_kwargs=kw)
        assert 'unexpected keyword' in str(e.value) and list(kw)[0] in str(e.value)


@pytest.mark.parametrize('kw', [{'s': 0.0}, {'s': -1.0}, {'s': float('nan')}, {'k': 0}, {'k': -3}, {'k': 2.5},
                                {'d': float('nan')}, {'d': float('inf')}, {'d': 'high'}, {'d': None}])
def test_bad_parameters_raise_value_error(kw):
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting.rdc import rdc_scores, rdc_cols
    data, dists, doms = _args()
    with pytest.raises(ValueError):
        rdc_cols(data, dists, doms, np.random.RandomState(0), **kw)
    with pytest.raises(ValueError):
        learn_spn(data, dists, doms, split_rows='random', split_cols=rdc_cols, split_cols_kwargs=kw)
    if 'd' not in kw:
        with pytest.raises(ValueError):
            rdc_scores(data, dists, doms, np.random.RandomState(0), **kw)


def test_continuous_distributions_raise():
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting.rdc import rdc_scores, rdc_cols
    from deeprob.spn.structure.leaf import Gaussian, Uniform
    data, dists, doms = _args()
    for cont in (Gaussian, Uniform):
        args = (data, [cont] + dists[1:], [(0.0, 1.0)] + doms[1:])
        for call in (lambda: rdc_scores(*args, np.random.RandomState(0)), lambda: rdc_cols(*args, np.random.RandomState(0)),
                     lambda: learn_spn(*args, split_rows='random', split_cols=rdc_cols)):
            with pytest.raises(NotImplementedError) as e:
                call()
            assert cont.__name__ in str(e.value)


def test_data_checks_are_those_of_learn_spn(host_device):
    from deeprob.spn.learning.splitting.rdc import rdc_scores
    data, dists, doms = _args()
    rs = np.random.RandomState(0)
    for change, message in ((dict(distributions=[]), "The list of distribution classes must be non-empty"),
                            (dict(domains=[]), "The list of domains must be non-empty"),
                            (dict(data=data[0]), "The data must be a matrix of samples by features"),
                            (dict(domains=doms[:3]), "Each data column should correspond to a random variable having a "
                                                     "distribution and a domain"),
                            (dict(random_state='seed'), "The random state must be either None, a seed integer or a Numpy "
                                                        "RandomState")):
        kw = dict(data=data, distributions=dists, domains=doms, random_state=rs)
        kw.update(change)
        with pytest.raises(ValueError) as e:
            rdc_scores(**kw)
        assert str(e.value) == message
    for bad in ([[1, 2]] + doms[1:], [list(range(17))] + doms[1:], [(0, 1)] + doms[1:]):
        with pytest.raises(ValueError):
            rdc_scores(data, dists, bad, rs)


def test_nan_and_out_of_domain_data_raise():
    """The real data path: its value checks come before the device is asked for."""
    from deeprob.spn.learning.splitting.rdc import rdc_scores
    data, dists, doms = _args()
    for r, c, v in ((3, 1, np.nan), (3, 1, 3.0), (3, 1, 0.5), (0, 0, -1.0)):
        bad = data.copy()
        bad[r, c] = v
        with pytest.raises(ValueError):
            rdc_scores(bad, dists, doms, np.random.RandomState(0))


def test_cpu_tensor_raises_hip_error_not_not_implemented():
    from deeprob.hip import HipError
    from deeprob.spn.learning import learn_spn, learn_estimator, learn_classifier
    from deeprob.spn.learning.splitting.rdc import rdc_scores, rdc_cols
    data, dists, doms = _args()
    for fn in (learn_spn, learn_estimator, learn_classifier):
        with pytest.raises(HipError):
            fn(torch.from_numpy(data), dists, doms, split_rows='random', split_cols=rdc_cols)
    for fn in (rdc_scores, rdc_cols):
        with pytest.raises(HipError):
            fn(torch.from_numpy(data), dists, doms, np.random.RandomState(0))


def test_only_the_package_function_is_recognised():
    """Identity, not name or behaviour: a wrapper of rdc_cols, a function of the same name and the string stay unbuilt."""
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting.rdc import rdc_cols as real

    def rdc_cols(*a, **k):
        return real(*a, **k)

    data, dists, doms = _args()
    for other in (rdc_cols, lambda *a, **k: real(*a, **k), 'rdc'):
        with pytest.raises(NotImplementedError):
            learn_spn(data, dists, doms, split_rows='random', split_cols=other)


def test_header_states_the_order_of_operations():
    from deeprob.hip import learn
    text = open(os.path.join(ROOT, 'include', 'deeprob_learn.h')).read()
    assert 'dpl_pair_maxcorr' in learn.SIGNATURES
    assert learn.SIGNATURES['dpl_pair_maxcorr'] == learn.SIGNATURES['dpl_pair_g']        # the pair tables, unchanged
    for words in ('2^-48', 'after 30', 'PRESENT values', 'never on M M^T'):
        assert words in text
    assert rdc_ref.JACOBI_TOL == 2.0 ** -48 and rdc_ref.JACOBI_SWEEPS == 30
