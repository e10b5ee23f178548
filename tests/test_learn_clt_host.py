"""``learn_spn(learn_leaf=learn_binary_clt)`` without a device: the header entry and its binding, the argument errors (all
raised before any device work: on a machine without a device anything later is a HipError), and the preconditions of the
goldens the device tests compare with."""
import functools
import json
import os
import re

import numpy as np
import pytest

from tests import learnspn_ref as ref
from tests import learn_clt_cases as cases

ROOT = cases.ROOT


# ---- the header and the binding -------------------------------------------------------------------------------------------
def test_header_declares_pair_ones_once_and_the_binding_parses_it():
    from deeprob import hip
    from deeprob.hip import learn
    text = open(os.path.join(ROOT, 'include', 'deeprob_learn.h')).read()
    declared = re.findall(r'\b(dpl_\w+)\s*\(', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    assert declared.count('dpl_pair_ones') == 1
    sigs, consts, _ = hip.parse_header(text, prefix='dpl', header='deeprob_learn.h')
    assert 'dpl_pair_ones' in sigs and sigs == learn.SIGNATURES
    assert consts['DPL_PAIR_TILE'] == 64 and consts['DPL_PAIR_ROW_CHUNK'] >= 64
    lib = learn.load_library()
    assert lib.dpl_abi_version() >= 4 and hasattr(lib, 'dpl_pair_ones')
    assert callable(learn.pair_ones)


def test_module_takes_the_reference_path_and_exports():
    from deeprob.spn.learning import leaf, learnspn
    for name in ('learn_binary_clt', 'learn_mle', 'learn_naive_factorization'):
        assert callable(getattr(leaf, name))
    assert learnspn.LAUNCHES_PER_GENERATION == 14 and learnspn.CLT_LAUNCHES_PER_GENERATION == 4


# ---- arguments --------------------------------------------------------------------------------------------------------------
def _args():
    from deeprob.spn.structure.leaf import Bernoulli
    data = (np.arange(40).reshape(10, 4) % 2).astype(np.float32)
    return data, [Bernoulli] * 4, [[0, 1]] * 4


BERNOULLI_ONLY = "Binary Chow-Liu trees are only available for Bernoulli data"
SHAPES = "Each data column should correspond to a random variable having a distribution and a domain"


def test_non_bernoulli_distributions_raise_the_reference_error():
    from deeprob.spn.learning import learn_spn, learn_estimator, learn_classifier
    from deeprob.spn.learning.leaf import learn_binary_clt
    from deeprob.spn.structure.leaf import Categorical, Gaussian
    data, dists, doms = _args()
    for fn in (learn_spn, learn_estimator, learn_classifier):
        with pytest.raises(ValueError) as e:
            fn(data, [Categorical] + dists[1:], [[0, 1, 2]] + doms[1:], learn_leaf=learn_binary_clt, split_rows='random',
               split_cols='gvs')
        assert str(e.value) == BERNOULLI_ONLY
    # the Gaussian kind: the same error, whatever its column split
    for split_cols in ('random', 'gvs'):
        with pytest.raises(ValueError) as e:
            learn_spn(data, [Gaussian] * 4, [(0.0, 1.0)] * 4, learn_leaf=learn_binary_clt, split_rows='random',
                      split_cols=split_cols)
        assert str(e.value) == BERNOULLI_ONLY


@pytest.mark.parametrize('kwargs, error', [
    ({'beta': 1.0}, TypeError), ({'alpha': 0.1, 'root': 0}, TypeError), ({'alpha': -1.0}, ValueError),
    ({'random_state': 'seed'}, ValueError), ({'random_state': 1.5}, ValueError)])
def test_leaf_keywords(kwargs, error):
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.leaf import learn_binary_clt
    data, dists, doms = _args()
    given = dict(kwargs)
    with pytest.raises(error) as e:
        learn_spn(data, dists, doms, learn_leaf=learn_binary_clt, split_rows='random', split_cols='gvs',
                  learn_leaf_kwargs=kwargs)
    assert kwargs == given
    if error is TypeError:
        assert 'learn_binary_clt' in str(e.value) and "unexpected keyword argument" in str(e.value)


def test_accepted_keywords_reach_the_device():
    """``to_pc``, ``alpha`` and ``random_state`` pass the checks: what stops the call on a CPU tensor is the HipError of
    the upload, the first device work."""
    import torch
    from deeprob.hip import HipError
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.leaf import learn_binary_clt
    data, dists, doms = _args()
    rs = np.random.RandomState(0)
    before = rs.get_state()[1].copy()
    for kw in ({'to_pc': True, 'alpha': 0.5, 'random_state': rs}, {'random_state': 3}, {'random_state': None}, None):
        with pytest.raises(HipError):
            learn_spn(torch.from_numpy(data), dists, doms, learn_leaf=learn_binary_clt, split_rows='random', split_cols='gvs',
                      learn_leaf_kwargs=kw, random_state=rs)
    assert np.array_equal(rs.get_state()[1], before), 'the checks draw nothing'


def test_wrappers_and_the_string_still_raise():
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.leaf import learn_binary_clt, learn_mle
    data, dists, doms = _args()
    wrappers = [lambda *a, **k: learn_binary_clt(*a, **k), functools.partial(learn_binary_clt, to_pc=True), learn_mle,
                'binary-clt']
    for leaf in wrappers:
        with pytest.raises(NotImplementedError):
            learn_spn(data, dists, doms, learn_leaf=leaf, split_rows='random', split_cols='gvs')


def test_the_function_on_its_own_raises_the_reference_errors():
    from deeprob.spn.learning.leaf import learn_binary_clt, learn_mle, learn_naive_factorization
    from deeprob.spn.structure.leaf import Categorical
    data, dists, doms = _args()
    with pytest.raises(ValueError) as e:
        learn_binary_clt(data, [Categorical] + dists[1:], doms, [0, 1, 2, 3])
    assert str(e.value) == BERNOULLI_ONLY
    for bad in (dict(scope=[0, 1, 2]), dict(domains=doms[:3])):
        kw = dict(dict(distributions=dists, domains=doms, scope=[0, 1, 2, 3]), **bad)
        for fn in (learn_binary_clt, learn_mle):
            with pytest.raises(ValueError) as e:
                fn(data, **kw)
            assert str(e.value) == SHAPES
        with pytest.raises(ValueError) as e:
            learn_naive_factorization(data, learn_leaf_func=learn_mle, **kw)
        assert str(e.value) == SHAPES
    with pytest.raises(NotImplementedError):
        learn_naive_factorization(data, dists, doms, [0, 1, 2, 3], lambda *a, **k: None)
    with pytest.raises(TypeError):
        learn_naive_factorization(data, dists, doms, [0, 1, 2, 3], learn_mle, to_pc=True)


# ---- the goldens --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', cases.CONFIGS)
def test_fixture_margin_and_shape(name):
    g = cases.golden(name)
    assert float(g['margin']) >= 1e-3 and int(g['gtest_calls']) > 0
    leaves = cases.golden_leaves(name)
    assert len(leaves) == int(g['clt_leaves']) > 0
    assert all(node['class'] == 'BinaryCLT' and len(node['scope']) > 1 and len(rows) >= 1 for node, rows in leaves)
    classes = [r['class'] for r in json.loads(str(g['clt_json']))['nodes']]
    assert classes.count('BinaryCLT') == len(leaves) and 'Sum' in classes and 'Product' in classes
    assert (name == 'a') == (int(g['leaf_seed']) >= 0)


def test_the_two_goldens_have_different_leaf_counts():
    assert int(cases.golden('a')['clt_leaves']) != int(cases.golden('b')['clt_leaves'])


@pytest.mark.parametrize('name', cases.CONFIGS)
def test_golden_leaves_follow_from_the_counts_of_their_rows(name):
    """numpy counts of a golden leaf's rows, through the host half of ``BinaryCLT.fit`` with the golden's root: the golden's
    tree exactly, its CPTs within 1e-6.  So a device run that counts right reproduces the goldens."""
    from deeprob.spn.structure.cltree import BinaryCLT
    g = cases.golden(name)
    x = g['data'].astype(np.int64)
    for node, rows in cases.golden_leaves(name):
        sub = x[rows][:, node['scope']]
        leaf = BinaryCLT(node['scope'], root=node['params']['root'])
        leaf.fit_counts(sub.T @ sub, len(rows), alpha=float(g['alpha']))
        assert list(leaf.tree) == list(node['params']['tree']), node['scope']
        err = float(np.max(np.abs(leaf.params.astype(np.float64) - np.asarray(node['params']['params']))))
        assert err <= 1e-6, (node['scope'], err)


@pytest.mark.parametrize('name', cases.CONFIGS)
def test_expansion_of_the_golden_leaves_is_the_reference_to_pc_graph(name):
    """The reference's run with ``to_pc=True`` is its run with ``to_pc=False`` with every leaf expanded by this package's
    ``to_pc_nodes``: same nodes, ids, scopes and edges, weights within 1e-6."""
    from deeprob.spn.structure.io import spn_to_digraph
    g = cases.golden(name)
    flat = cases.expand(json.loads(str(g['clt_json'])))
    assert ref.graphs_differ(spn_to_digraph(flat), json.loads(str(g['pc_json']))) is None
