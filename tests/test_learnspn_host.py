"""LearnSPN without a device: the numpy restatement (tests/learnspn_ref.py) against the reference's golden graphs,
``prune`` against the reference's pruned graphs, the argument handling of ``learn_spn`` and its wrappers, and the
header of the learn library."""
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import learnspn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CONFIGS = ['binary16_gvs', 'binary16_rgvs', 'cat3x12_gvs', 'cat3x12_rgvs', 'mixed10_gvs', 'mixed10_rgvs']

_cache = {}


def golden(name):
    if name not in _cache:
        g = np.load(os.path.join(GOLDEN, 'learnspn_%s.npz' % name))
        _cache[name] = {k: g[k] for k in g.files}
    return _cache[name]


def names_of(ks):
    return ['Bernoulli' if k == 2 else 'Categorical' for k in ks]


def restated(name):
    """The restatement's unpruned root for a golden configuration (computed once)."""
    key = ('restated', name)
    if key not in _cache:
        g = golden(name)
        ks = [int(k) for k in g['ks']]
        _cache[key] = ref.learn_spn(g['data'], names_of(ks), ks, split_rows='random', split_cols=name.split('_')[1],
                                    min_rows_slice=int(g['min_rows_slice']), random_state=int(g['seed']))
    return _cache[key]


@pytest.mark.parametrize('name', CONFIGS)
def test_fixture_margin(name):
    g = golden(name)
    assert float(g['margin']) >= 1e-3 and int(g['gtest_calls']) > 0


@pytest.mark.parametrize('name', CONFIGS)
def test_restatement_reproduces_reference_graph(name):
    want = json.loads(str(golden(name)['spn_json']))
    assert ref.graphs_differ(ref.to_digraph(restated(name)), want) is None


@pytest.mark.parametrize('name', CONFIGS)
def test_restatement_prune_reproduces_reference_estimator(name):
    g = golden(name)
    root = ref.prune(ref.from_digraph(json.loads(str(g['spn_json']))))
    assert ref.graphs_differ(ref.to_digraph(root), json.loads(str(g['est_json']))) is None


@pytest.mark.parametrize('name', CONFIGS)
def test_prune_of_unpruned_golden_is_pruned_golden(name):
    from deeprob.spn.structure.io import load_spn_json, spn_to_digraph
    from deeprob.spn.algorithms.structure import prune
    g = golden(name)
    flat = load_spn_json(io.StringIO(str(g['spn_json'])))
    before = json.dumps(spn_to_digraph(flat))
    pruned = prune(flat)
    assert ref.graphs_differ(spn_to_digraph(pruned), json.loads(str(g['est_json']))) is None
    assert json.dumps(spn_to_digraph(flat)) == before          # the input is left alone


def test_prune_merges_a_shared_child_once():
    """A DAG: two sum children of a sum share a leaf; its weights add up (structure.py:62-73)."""
    from deeprob.spn.structure.io import FlatSpn
    from deeprob.spn.algorithms.structure import prune
    leaf = lambda p: {'class': 'Bernoulli', 'scope': [0], 'params': {'p': p}}
    nodes = {0: {'class': 'Sum', 'scope': [0], 'weights': [0.25, 0.75]}, 1: {'class': 'Sum', 'scope': [0], 'weights': [0.5, 0.5]},
             2: {'class': 'Sum', 'scope': [0], 'weights': [0.2, 0.8]}, 3: leaf(0.1), 4: leaf(0.6), 5: leaf(0.9)}
    flat = prune(FlatSpn(nodes, {0: [1, 2], 1: [3, 4], 2: [4, 5]}))
    assert flat.classes == ['Sum', 'Bernoulli', 'Bernoulli', 'Bernoulli']
    assert np.allclose(flat.child_weight[:3], [0.125, 0.125 + 0.15, 0.6], atol=1e-7)
    assert np.allclose(flat.raw0[1:], [0.1, 0.6, 0.9])


def test_compute_data_domains_matches_golden():
    from deeprob.spn.learning import compute_data_domains
    from deeprob.spn.structure.leaf import Bernoulli, Categorical
    g = golden('mixed10_gvs')
    dists = [Bernoulli if k == 2 else Categorical for k in g['ks']]
    assert compute_data_domains(g['data'].astype(np.float32), dists) == json.loads(str(g['domains_json']))


@pytest.mark.parametrize('n_clusters', sorted(ref.KMEANS_CASE_TASKS))
def test_kmeans_case_meets_the_preconditions_of_the_device_test(n_clusters):
    """The fixture of test_discrete_kmeans_against_the_restatement: the seed table gives a case for every task, every
    restart's restated centroid gap is >= 1e-6, and the case has the shape that test relies on."""
    from deeprob.hip import learn as L
    assert sorted(ref.KMEANS_CASE_TASKS) == [1, 2, L.DPL_MAX_CLUSTERS]
    case = ref.kmeans_case(n_clusters)
    assert case is not None, 'no seed of the table has a centroid gap of 1e-6'
    x, segments, tasks, want, gap = case
    print('n_clusters', n_clusters, 'centroid gap', gap)
    assert gap >= 1e-6 and all(run[3] >= 1e-6 for runs in want for run in runs)
    ks = ref.KMEANS_CASE_KS
    assert ks == [2, 2, 5, 3, 2] and x.dtype == np.uint8 and x.shape[1] == 5 and np.all(x < np.asarray(ks))
    assert [n for n, _, _ in tasks] == [300, 256, 5 if n_clusters <= 5 else 8]
    assert len(set(tuple(cols) for _, cols, _ in tasks)) == 3
    rows = np.concatenate(segments)
    assert len(np.unique(rows)) == len(rows)
    for seg, (n, cols, seeds), runs in zip(segments, tasks, want):
        assert len(seg) == n and not np.array_equal(seg, np.sort(seg)) and seg.max() - seg.min() >= n
        assert cols != sorted(cols) and min(ks[c] for c in cols) <= 2 < max(ks[c] for c in cols)
        assert seeds.shape == (ref.KMEANS_CASE_RESTARTS, n_clusters) and len(runs) == ref.KMEANS_CASE_RESTARTS
        assert all(len(np.unique(s)) == n_clusters and s.max() < n for s in seeds)


# ---- arguments ---------------------------------------------------------------------------------------------------------
def _args():
    from deeprob.spn.structure.leaf import Bernoulli
    data = (np.arange(40).reshape(10, 4) % 2).astype(np.float32)
    return data, [Bernoulli] * 4, [[0, 1]] * 4


def test_leaf_markers():
    from deeprob.spn.structure import leaf
    for cls, kind in ((leaf.Bernoulli, leaf.LeafType.DISCRETE), (leaf.Categorical, leaf.LeafType.DISCRETE),
                      (leaf.Gaussian, leaf.LeafType.CONTINUOUS), (leaf.Uniform, leaf.LeafType.CONTINUOUS)):
        assert cls.LEAF_TYPE == kind and cls.__name__ in ('Bernoulli', 'Categorical', 'Gaussian', 'Uniform')


def test_reexports():
    import deeprob.spn.learning as L
    from deeprob.spn.learning import learnspn, wrappers
    assert L.learn_spn is learnspn.learn_spn and L.learn_estimator is wrappers.learn_estimator
    assert L.learn_classifier is wrappers.learn_classifier and L.compute_data_domains is wrappers.compute_data_domains
    assert isinstance(learnspn.last_info(), dict)


@pytest.mark.parametrize('change, message', [
    (dict(distributions=[]), "The list of distribution classes must be non-empty"),
    (dict(domains=[]), "The list of domains must be non-empty"),
    (dict(min_rows_slice=0), "The minimum number of samples required to split horizontally must be positive"),
    (dict(min_cols_slice=0), "The minimum number of samples required to split vertically must be positive"),
    (dict(domains=[[0, 1]] * 3), "Each data column should correspond to a random variable having a distribution and a domain"),
    (dict(learn_leaf='nope'), "Unknown learn leaf method called nope"),
    (dict(split_rows='nope'), "Unknown split rows method called nope"),
    (dict(split_cols='nope'), "Unknown split rows method called nope"),
])
def test_argument_errors_match_the_reference(change, message):
    from deeprob.spn.learning import learn_spn
    data, dists, doms = _args()
    kw = dict(distributions=dists, domains=doms, split_rows='random', split_cols='gvs')
    kw.update(change)
    with pytest.raises(ValueError) as e:
        learn_spn(data, **kw)
    assert str(e.value) == message


def test_learn_estimator_methods():
    from deeprob.spn.learning import learn_estimator
    data, dists, doms = _args()
    with pytest.raises(ValueError) as e:
        learn_estimator(data, dists, doms, method='nope')
    assert str(e.value) == "Unknown SPN learning method called nope"
    for method in ('xpc', 'ensemble-xpc'):
        with pytest.raises(NotImplementedError):
            learn_estimator(data, dists, doms, method=method)


NOT_BUILT = [('learn_leaf', n) for n in ('isotonic', 'binary-clt')] + \
            [('split_rows', n) for n in ('kmeans_mb', 'dbscan', 'wald', 'gmm', 'rdc')] + \
            [('split_cols', n) for n in ('wrgvs', 'ebvs', 'ebvs_ae', 'gbvs', 'gbvs_ag', 'rdc')]


@pytest.mark.parametrize('arg, name', NOT_BUILT)
def test_not_built_names_raise(arg, name):
    from deeprob.spn.learning import learn_spn
    data, dists, doms = _args()
    kw = dict(split_rows='random', split_cols='gvs')
    kw[arg] = name
    with pytest.raises(NotImplementedError) as e:
        learn_spn(data, dists, doms, **kw)
    assert name in str(e.value)


def test_default_split_cols_and_callables_and_continuous_raise():
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.structure.leaf import Gaussian, Uniform
    data, dists, doms = _args()
    with pytest.raises(NotImplementedError) as e:
        learn_spn(data, dists, doms)                        # split_cols='rdc' is the reference's default
    assert 'rdc' in str(e.value)
    for arg in ('learn_leaf', 'split_rows', 'split_cols'):
        with pytest.raises(NotImplementedError):
            learn_spn(data, dists, doms, **dict(dict(split_rows='random', split_cols='gvs'), **{arg: lambda *a, **k: None}))
    for cont in (Gaussian, Uniform):
        with pytest.raises(NotImplementedError) as e:
            learn_spn(data, [cont] + dists[1:], [(0.0, 1.0)] + doms[1:], split_rows='random', split_cols='gvs')
        assert cont.__name__ in str(e.value)


@pytest.mark.parametrize('domains', [[[0, 1]] * 3 + [[1, 2]], [[0, 1]] * 3 + [[0, 2]], [[0, 1]] * 3 + [list(range(17))],
                                     [[0, 1]] * 3 + [[0, 1, 2]], [[0, 1]] * 3 + [(0, 1)]])
def test_bad_domains_raise(domains):
    from deeprob.spn.learning import learn_spn
    data, dists, _ = _args()        # (the fourth variable is Bernoulli: [0, 1, 2] is not its domain)
    with pytest.raises(ValueError):
        learn_spn(data, dists, domains, split_rows='random', split_cols='gvs')


def test_nan_raises_and_nothing_is_modified():
    from deeprob.spn.learning import learn_spn
    data, dists, doms = _args()
    data[3, 1] = np.nan
    kwargs = {'alpha': 0.5}
    before = data.copy()
    with pytest.raises(ValueError) as e:
        learn_spn(data, dists, doms, split_rows='random', split_cols='gvs', learn_leaf_kwargs=kwargs)
    assert 'NaN' in str(e.value)
    assert kwargs == {'alpha': 0.5} and np.array_equal(data, before, equal_nan=True)


def test_cpu_tensor_raises_hip_error():
    from deeprob.hip import HipError
    from deeprob.spn.learning import learn_spn, learn_estimator, learn_classifier
    data, dists, doms = _args()
    for fn in (learn_spn, learn_estimator, learn_classifier):
        with pytest.raises(HipError):
            fn(torch.from_numpy(data), dists, doms, split_rows='random', split_cols='gvs')


# ---- the header and the library ------------------------------------------------------------------------------------------
def test_learn_header_parses_and_matches_the_exports():
    from deeprob import hip
    from deeprob.hip import learn
    text = open(os.path.join(ROOT, 'include', 'deeprob_learn.h')).read()
    sigs, consts, structs = hip.parse_header(text, prefix='dpl', header='deeprob_learn.h')
    assert sigs == learn.SIGNATURES and consts['DPL_OK'] == 0 and consts['DPL_MAX_K'] == 16 and not structs
    declared = re.findall(r'\b(dpl_\w+)\s*\(', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    assert sorted(declared) == sorted(set(declared)) == sorted(sigs), 'every entry point is declared once'
    out = subprocess.run(['nm', '-D', '--defined-only', learn.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = sorted(l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith('dpl_'))
    assert exported == sorted(sigs)


def test_missing_learn_library_names_the_make_command(monkeypatch):
    from deeprob.hip import HipError, learn
    monkeypatch.setattr(learn, '_lib', None)
    monkeypatch.setattr(learn, 'LIB_PATH', os.path.join(ROOT, 'no', 'such', 'libdeeprob_learn.so'))
    with pytest.raises(HipError) as e:
        learn.load_library()
    assert 'make -C deeprob-kit_amd/csrc' in str(e.value)

