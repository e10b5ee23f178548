"""BinaryCNet without a device: the numpy restatement (tests/cnet_ref.py) against the reference's goldens
(tests/golden/cnet_*.npz, tools/gen_golden_cnet.py), the stop rule and the argument handling of the package, and the
cutset-network entries of the CLT header.

The leaves' trees: see ``cnet_ref.assert_leaf_trees`` -- most leaves of a cutset network have several maximum spanning
trees (few rows, tied mutual informations), so the reference's edge set is required where it is the only one and a tree of
the same sorted weights elsewhere.  The reference's likelihoods are compared with the restatement holding the REFERENCE's
leaf trees, on every row: they do not depend on the root, but they do depend on which of several maximum spanning trees a
leaf got."""
import os
import re

import numpy as np
import pytest
import torch

from tests import cnet_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(ref.CONFIGS)


def bar(got, want):
    """The project's bar: max |got - want| / max(1, |want|)."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


# ---- the fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_fixture_holds_what_the_tests_need(name):
    g = ref.golden(name)
    n, d, k, noise, seed, alpha, min_n_samples, min_n_features, min_mean_entropy = ref.CONFIGS[name]
    data, fresh = ref.mixture(n, d, k, noise, seed)
    assert np.array_equal(g['x'], data) and np.array_equal(g['fresh'], fresh)
    assert ref.hyper(g) == dict(alpha=alpha, min_n_samples=min_n_samples, min_n_features=min_n_features,
                                min_mean_entropy=min_mean_entropy)
    assert float(g['selection_margin']) >= 1e-4 and float(g['entropy_band']) >= 1e-3 and float(g['min_abs_gain']) >= 1e-6
    assert g['ll_train'].shape == (n,) and g['ll_fresh'].shape == (ref.N_FRESH,)
    assert np.array_equal(g['is_leaf'], g['or_id'] < 0) and g['leaf_unique'][g['is_leaf']].any()
    assert os.path.getsize(os.path.join(ref.GOLDEN, 'cnet_%s.npz' % name)) <= 150 * 1000


def test_fixtures_cover_every_stop_rule_the_issue_names():
    stops = {name: ref.golden(name)['stop'] for name in NAMES}
    assert (stops['d24'] == 2).sum() == 15                   # the entropy rule
    d5 = ref.golden('d5')
    scope_sizes = np.diff(d5['leaf_scope_off'])[d5['is_leaf']]
    assert (scope_sizes == 1).sum() >= 15                    # min_n_features = 1
    d10 = ref.golden('d10')
    assert int(d10['min_n_features']) == 3 and np.diff(d10['leaf_scope_off'])[d10['is_leaf']].min() == 3
    assert [int((ref.golden(n)['or_id'] >= 0).sum()) for n in NAMES] == [68, 34, 20, 15, 25, 111]


# ---- the restatement against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_restatement_reproduces_the_or_tree(name):
    g = ref.golden(name)
    or_id, weights, scopes, edges, rows = ref.structure(ref.restated(name))
    want_or_id, want_weights, want_scopes, _, want_rows = ref.golden_structure(g)
    assert np.array_equal(or_id, want_or_id) and np.array_equal(rows, want_rows) and scopes == want_scopes
    inner = or_id >= 0
    assert np.max(np.abs(weights[inner] - want_weights[inner])) <= 1e-12
    ref.assert_leaf_trees(name, edges)


@pytest.mark.parametrize('name', NAMES)
def test_restatement_log_likelihood_reproduces_reference(name):
    g = ref.golden(name)
    model = ref.restated(name, reference_trees=True)
    assert ref.structure(model)[3] == ref.golden_structure(g)[3]
    assert bar(ref.log_likelihood(model, g['x']), g['ll_train']) <= 1e-5
    assert bar(ref.log_likelihood(model, g['fresh']), g['ll_fresh']) <= 1e-5


def test_restatement_marginal_is_the_sum_over_completions():
    model = ref.restated('d10')
    q = ref.queries('d10')
    assert np.isnan(q[0]).all() and not np.isnan(q[1]).any() and 0.3 < np.isnan(q).mean() < 0.5
    got = ref.log_likelihood(model, q)
    assert bar(got, ref.brute_marginal(model, q)) <= 1e-5
    assert abs(float(got[0])) <= 1e-5


def test_restatement_scores_are_the_reference_expressions():
    """The float64 scores against a direct float64 evaluation of cnet.py:168-198 with numpy's own sums."""
    g = ref.golden('d24')
    alpha = float(g['alpha'])
    part = g['x'][:700].astype(np.float64)
    n, d = part.shape
    mean_entropy, gains = ref.scores(part, alpha)
    ones = part.T @ part
    c = np.diag(ones)
    prior = np.stack([n - c, c], axis=1)
    joint = np.empty((d, d, 2, 2))
    joint[:, :, 1, 1], joint[:, :, 0, 1], joint[:, :, 1, 0] = ones, c[None, :] - ones, c[:, None] - ones
    joint[:, :, 0, 0] = n - c[None, :] - c[:, None] + ones
    p = (prior + 2 * alpha) / (n + 4 * alpha)
    p[:, 0] = 1.0 - p[:, 1]
    want_entropy = -(p * np.log(p)).sum() / d
    cond = (joint + 2 * alpha) / (prior[:, None, :, None] + 4 * alpha)
    h = -(cond * np.log(cond)).sum(axis=-1)                                  # [i, j, a]
    off = ~np.eye(d, dtype=bool)
    mean_h = np.array([[h[i, off[i], a].mean() for a in (0, 1)] for i in range(d)])
    want = want_entropy - (c / n * mean_h[:, 1] + (1 - c / n) * mean_h[:, 0])
    assert abs(mean_entropy - want_entropy) <= 1e-13 and np.max(np.abs(gains - want)) <= 1e-13


# ---- the package's host side -------------------------------------------------------------------------------------------------
def test_stop_rule_on_hand_made_records():
    from deeprob.spn.structure.cnet import stop_rule
    rule = dict(min_n_samples=10, min_n_features=2, min_mean_entropy=0.05)
    assert stop_rule(100, 5, 0.3, 0.01, **rule) is None
    # each rule alone
    assert stop_rule(10, 5, 0.3, 0.01, **rule) == 'samples'
    assert stop_rule(100, 2, 0.3, 0.01, **rule) == 'features'
    assert stop_rule(100, 5, 0.01, 0.01, **rule) == 'entropy'
    assert stop_rule(100, 5, 0.3, -0.01, **rule) == 'gain'
    # the edges: n <= min_n_samples, d <= min_n_features, entropy < bound (not <=), gain <= 0
    assert stop_rule(11, 3, 0.3, 0.01, **rule) is None
    assert stop_rule(100, 5, 0.05, 0.01, **rule) is None
    assert stop_rule(100, 5, np.nextafter(0.05, 0), 0.01, **rule) == 'entropy'
    assert stop_rule(100, 5, 0.3, 0.0, **rule) == 'gain'
    assert stop_rule(100, 5, 0.3, np.nextafter(0.0, 1), **rule) is None
    # the reference's order: rows, features, entropy, gain; the first two need no scores
    assert stop_rule(10, 2, 0.01, -1.0, **rule) == 'samples'
    assert stop_rule(100, 2, 0.01, -1.0, **rule) == 'features'
    assert stop_rule(100, 5, 0.01, -1.0, **rule) == 'entropy'
    assert stop_rule(0, 5, None, None, **rule) == 'samples' and stop_rule(100, 1, None, None, **rule) == 'features'


def test_constructor_and_its_errors():
    from deeprob.spn.structure.cnet import BinaryCNet, ORNode
    for weights in ([0.5, 0.6], np.array([0.2, 0.2])):
        with pytest.raises(ValueError) as e:
            BinaryCNet([0, 1], weights=weights)
        assert str(e.value) == "Weights don't sum up to 1"
    node = BinaryCNet([3, 4], weights=[0.25, 0.75], or_id=4)
    assert isinstance(node, ORNode) and node.weights.dtype == np.float32 and node.or_id == 4 and node.scope == [3, 4]
    assert node.children == [] and node.clt is None
    left, right = BinaryCNet([3]), BinaryCNet([3])
    root = BinaryCNet([3, 4], children=[left, right], weights=np.array([0.5, 0.5]), or_id=4)
    assert root.children[0] is left and root.children[1] is right
    from deeprob.hip import HipError
    with pytest.raises(HipError) as e:
        root.log_likelihood(torch.zeros(2, 2))            # a CPU tensor
    assert 'make -C deeprob-kit_amd/csrc' in str(e.value)


def test_fit_argument_errors():
    from deeprob.hip import clt
    from deeprob.spn.structure.cnet import BinaryCNet
    data = ref.golden('d5')['x']
    for kwargs in (dict(alpha=-0.5), dict(min_n_features=0), dict(min_n_samples=-1), dict(random_state='x')):
        with pytest.raises(ValueError):
            BinaryCNet(list(range(5))).fit(data, **kwargs)
    for bad in (np.nan, 2.0, 0.5, -1.0):
        spoiled = data.copy()
        spoiled[7, 3] = bad
        with pytest.raises(ValueError) as e:
            BinaryCNet(list(range(5))).fit(spoiled)
        assert 'binary' in str(e.value)
    for shape in ((5,), (4, 5, 1), (0, 5)):
        with pytest.raises(ValueError):
            BinaryCNet(list(range(5))).fit(np.zeros(shape, np.float32))
    with pytest.raises(ValueError) as e:
        BinaryCNet([0]).fit(np.zeros((2, clt.DPC_MAX_D + 1), np.float32))
    assert 'DPC_MAX_D' in str(e.value)


def test_a_leaf_without_rows_gets_the_uniform_prior_tree():
    """Every count zero: (0 + 2 alpha) / (0 + 4 alpha) = 1 / 2 everywhere, through the host half of BinaryCLT.fit."""
    from deeprob.spn.structure.cltree import BinaryCLT
    clt = BinaryCLT([4, 7, 9], root=7)
    clt.fit_counts(np.zeros((3, 3), np.int64), 0, alpha=0.01)
    assert clt.tree[1] == -1 and sorted(clt.bfs) == [0, 1, 2] and clt.params.shape == (3, 2, 2)
    assert np.max(np.abs(clt.params - np.log(0.5))) <= 1e-6
    bfs, tree, params = ref.clt_ref.fit(np.zeros((0, 3), np.float32), 1, 0.01)
    assert np.max(np.abs(params - clt.params)) <= 1e-6       # (every pair ties: the two trees need not be the same)


def test_device_tables_reject_what_is_no_cutset_network():
    """Checked on the host before anything is uploaded: the kernel indexes device memory with these tables."""
    from deeprob.hip import cnet
    half = np.full((1, 2, 2), np.log(0.5), np.float32)
    leaf = lambda col: ([col], [0], [-1], half)                     # noqa: E731
    logw = np.log(np.full((3, 2), 0.5))
    good = cnet.DeviceCNet(2, [0, -1, -1], [[1, 2], [0, -1], [1, -1]], logw, [leaf(1), leaf(1)], 'cpu')
    assert (good.levels, good.max_leaf_d, good.n_nodes, good.row_bytes) == (2, 1, 3, 12 * 2 + 8)
    for col, child, leaves in (([0, -1, -1], [[1, 1], [0, -1], [1, -1]], [leaf(1), leaf(1)]),      # a node twice
                               ([0, -1, -1], [[1, 3], [0, -1], [1, -1]], [leaf(1), leaf(1)]),      # a child out of range
                               ([0, -1, -1], [[1, 2], [0, -1], [0, -1]], [leaf(1), leaf(1)]),      # a leaf twice
                               ([0, -1, -1], [[1, 2], [0, -1], [1, -1]], [leaf(1), leaf(0)]),      # a cut column in a leaf
                               ([2, -1, -1], [[1, 2], [0, -1], [1, -1]], [leaf(1), leaf(1)]),      # a column out of range
                               ([0, 0, -1], [[1, 2], [2, 2], [0, -1]], [leaf(1)])):                # a column cut twice
        with pytest.raises(ValueError) as e:
            cnet.DeviceCNet(2, col, child, logw[:len(col)], leaves, 'cpu')
        assert str(e.value) == "the node tables do not describe one cutset network"


def test_chunking_is_bounded_by_the_scratch_caps(monkeypatch):
    from deeprob.hip import cnet
    assert cnet.chunk_tasks(200) == cnet.COUNT_INTS // 40000 and cnet.chunk_tasks(4096) == 4 and cnet.chunk_tasks(2) == 65535
    monkeypatch.setattr(cnet, 'COUNT_INTS', 0)
    assert cnet.chunk_tasks(33) == 1
    monkeypatch.setattr(cnet, 'WORK_BYTES', 0)
    assert cnet.query_rows(100) == 1024


# ---- the header and the import -----------------------------------------------------------------------------------------------
def test_cnet_header_entries_parse_and_the_module_imports():
    from deeprob import hip
    text = open(os.path.join(ROOT, 'include', 'deeprob_clt.h')).read()
    sigs, _, structs = hip.parse_header(text, prefix='dpc', header='deeprob_clt.h')
    entries = sorted(s for s in sigs if s.startswith('dpc_cnet_'))
    assert entries == ['dpc_cnet_gather_pack', 'dpc_cnet_log_likelihood', 'dpc_cnet_pair_counts', 'dpc_cnet_partition',
                       'dpc_cnet_scores'] and not structs
    declared = re.findall(r'\b(dpc_cnet_\w+)\s*\(', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    assert sorted(declared) == entries
    import deeprob.spn.structure.cnet as module
    from deeprob.spn.structure.cnet import BinaryCNet, ORNode  # noqa: F401
    assert 'mpe' in module.__doc__ and 'learn_cnet_bd' in module.__doc__ and not hasattr(BinaryCNet, 'mpe')
    from deeprob.utils.statistics import compute_joint_counts, compute_prior_counts  # noqa: F401
