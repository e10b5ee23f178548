"""The scored cutset learners without a device: the numpy restatement (tests/cnet_scored_ref.py) against the reference's
goldens (tests/golden/cnet_bd_*.npz, cnet_bic_*.npz; tools/gen_golden_cnet_scored.py), the host half of the package --
trees, scores and re-rooting from counts -- against the restatement, the argument handling, and the ``dpc_cut_*`` entry
of the CLT header.

Tolerances.  OR weights within 1e-6 of the reference's.  A score of the restatement lies within 4 x the deviation the
generator measured on the reference's run (``score_deviation``, ``helper_deviation``: the reference mixes float32 in);
the generator kept every margin that decides something at least 4 x above the same deviation.  The package's host half
against the restatement: 1e-12 relative (both are float64 sums of the same terms, ``math.fsum`` on both sides)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import clt_ref
from tests import cnet_ref
from tests import cnet_scored_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(ref.CONFIGS)


def rel(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape
    return float(np.max(np.abs(got - want) / np.abs(want))) if len(want) else 0.0


# ---- the fixtures ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_fixture_holds_what_the_tests_need(name):
    g = ref.golden(name)
    config, kind, par, k = ref.CONFIGS[name]
    data, fresh = ref.data_of(name)
    assert np.array_equal(g['x'], data) and np.array_equal(g['fresh'], fresh)
    assert (int(g['learner']), float(g['par']), int(g['n_cand_cuts'])) == (0 if kind == 'bd' else 1, par, k)
    deviation = float(g['score_deviation'])
    assert float(g['selection_margin']) >= max(1e-4, 4 * deviation) and float(g['decision_margin']) >= max(1e-4, 4 * deviation)
    assert float(g['candidate_margin']) >= 1e-6 and 0 < deviation < 1e-5 and 0 < float(g['helper_deviation']) < 1e-5
    m = len(g['or_id'])
    assert g['ll_train'].shape == (len(data),) and g['ll_fresh'].shape == (cnet_ref.N_FRESH,)
    assert g['node_score'].shape == (m,) and g['cand_off'].shape == (m + 1,) and np.array_equal(g['is_leaf'], g['or_id'] < 0)
    assert os.path.getsize(os.path.join(ref.GOLDEN, 'cnet_%s.npz' % name)) <= 150 * 1000


def test_fixtures_cover_both_learners_a_lone_leaf_and_both_candidate_counts():
    n_or = {name: int((ref.golden(name)['or_id'] >= 0).sum()) for name in NAMES}
    assert n_or == {'bd_d24': 6, 'bd_d33': 3, 'bd_d5': 0, 'bd_d10': 0, 'bic_d24': 10, 'bic_d33': 7, 'bic_d10': 1}
    assert {ref.CONFIGS[n][3] for n in NAMES} == {3, 10}
    # a candidate count below and above the number of variables left
    assert ref.CONFIGS['bic_d10'][3] >= 10 and ref.CONFIGS['bd_d33'][3] < 33


# ---- the restatement against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_restatement_reproduces_the_reference(name):
    g, model = ref.golden(name), ref.restated(name)
    or_id, weights, scopes, edges, rows = cnet_ref.structure(model)
    want_or_id, want_weights, want_scopes, want_edges, want_rows = cnet_ref.golden_structure(g)
    assert np.array_equal(or_id, want_or_id) and np.array_equal(rows, want_rows) and scopes == want_scopes
    assert np.array_equal([m['depth'] for m in model], g['node_depth'])
    inner = or_id >= 0
    if inner.any():
        assert np.max(np.abs(weights[inner] - want_weights[inner])) <= 1e-6
    for k, node in enumerate(model):
        if node['or_id'] < 0 and g['leaf_unique'][k]:
            assert edges[k] == want_edges[k], k
    bound = 4 * float(g['score_deviation'])
    assert rel([m['score'] for m in model], g['node_score']) <= bound
    for k, node in enumerate(model):
        lo, hi = g['cand_off'][k], g['cand_off'][k + 1]
        got = dict(node['candidates'])
        assert sorted(got) == g['cand_vars'][lo:hi].tolist(), k
        assert rel([got[v] for v in g['cand_vars'][lo:hi]], g['cand_scores'][lo:hi]) <= bound, k


@pytest.mark.parametrize('name', ['bd_d24', 'bic_d33'])
def test_restatement_log_likelihoods_match_the_reference(name):
    """Where every leaf has one spanning tree the restated model IS the reference's up to the roots; elsewhere the rows
    that end in such a leaf are left out."""
    g, model = ref.golden(name), ref.restated(name)
    for x, want in ((g['x'], g['ll_train']), (g['fresh'], g['ll_fresh'])):
        keep = g['leaf_unique'][cnet_ref.leaf_of_rows(model, x)]
        assert keep.mean() > 0.5
        got = cnet_ref.log_likelihood(model, x)
        assert np.max(np.abs(got[keep] - want[keep]) / np.maximum(1.0, np.abs(want[keep]))) <= 1e-5


def test_restated_helpers_match_the_reference():
    for name in NAMES:
        g = ref.golden(name)
        _, kind, par, k = ref.CONFIGS[name]
        smoothing = par if kind == 'bd' else 4 * par
        bound = 4 * float(g['helper_deviation'])
        assert rel(ref.or_bd_scores(g['x'], smoothing), g['helper_or_scores']) <= bound
        pairs = ~np.eye(int(g['n_vars']), dtype=bool)
        assert rel(ref.clt_bd_scores(g['x'], smoothing)[pairs], g['helper_clt_scores'][pairs]) <= bound
        assert sorted(ref.candidates(g['x'], smoothing / 4, min(k, int(g['n_vars'])))[0]) == g['helper_cands'].tolist()


# ---- the host half of the package ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind, par', [('bd', 0.1), ('bd', 2.0), ('bic', 0.01), ('bic', 0.5)])
def test_trees_and_scores_from_counts_match_the_restatement(kind, par):
    from deeprob.spn.learning import cnet_bayesian as cb
    data, _ = ref.data_of('bd_d24')
    scorer = cb._Scorer(kind, par, len(data))
    for depth, rows, cols in ((0, slice(None), list(range(24))), (2, data[:, 3] == 1, [0, 5, 7, 8, 20]),
                              (5, slice(0, 9), [2, 4, 6]), (1, slice(0, 40), [11])):
        part = data[rows][:, cols]
        tree, score = scorer.tree(clt_ref.counts(part), len(part), depth)
        want_tree, want = ref.fit_tree(part, kind, par, depth, len(data))
        assert np.array_equal(tree, want_tree) and tree[0] == -1
        assert abs(score - want) <= 1e-12 * abs(want)


def test_helper_scores_from_counts_match_the_restatement_and_the_fixture():
    from deeprob.spn.learning import cnet_bayesian as cb
    g = ref.golden('bd_d33')
    x, d = g['x'], 33
    ones = clt_ref.counts(x)
    got_or, got_clt = cb._or_bd_scores(np.diag(ones), len(x), 0.1), cb._family_bd_scores(cb._cells(ones, len(x)), 0.1)
    assert rel(got_or, ref.or_bd_scores(x, 0.1)) <= 1e-12 and rel(got_clt, ref.clt_bd_scores(x, 0.1)) <= 1e-12
    pairs = ~np.eye(d, dtype=bool)
    assert rel(got_clt[pairs], g['helper_clt_scores'][pairs]) <= 4 * float(g['helper_deviation'])
    tree = ref.prim0(clt_ref.mutual_information(*clt_ref.priors_joints(ones, len(x), 0.01)))
    assert abs(cb.eval_tree_score(tree, got_clt, got_or) - ref.tree_score(tree, got_clt, got_or)) <= 1e-9
    assert abs(cb.eval_tree_score(tree, got_clt, got_or) - cb._bd_tree_score(ones, len(x), tree, 0.1)) <= 1e-9


def test_candidates_are_ordered_by_gain_then_column():
    from deeprob.spn.learning.cnet_bayesian import _top_candidates
    gains = np.array([0.5, 0.7, -np.inf, 0.7, 0.1, 0.5])
    cols = np.array([0, 1, 3, 4, 5])
    assert _top_candidates(gains, cols, 3).tolist() == [1, 3, 0]
    assert _top_candidates(gains, cols, 9).tolist() == [1, 3, 0, 5, 4]
    assert _top_candidates(gains, cols, 1).tolist() == [1]


def test_reroot_keeps_the_undirected_tree():
    from deeprob.spn.learning.cnet_bayesian import _reroot
    tree = np.array([-1, 0, 0, 1, 3, 2], np.int32)
    edges = cnet_ref.edge_set(list(range(6)), tree)
    for root in range(6):
        got = _reroot(tree, root)
        assert got[root] == -1 and got.dtype == np.int32 and cnet_ref.edge_set(list(range(6)), got) == edges
        assert np.array_equal(got, ref.rerooted(tree, root))
    assert np.array_equal(tree, [-1, 0, 0, 1, 3, 2])                # the input is left alone


# ---- arguments -------------------------------------------------------------------------------------------------------------
def test_arguments_out_of_domain_raise_value_error():
    from deeprob.spn.learning import cnet_bayesian as cb
    x = ref.golden('bd_d5')['x']
    for call in (lambda: cb.learn_cnet_bd(x, ess=0.0), lambda: cb.learn_cnet_bd(x, ess=-1.0),
                 lambda: cb.learn_cnet_bic(x, alpha=-0.01), lambda: cb.learn_cnet_bd(x, n_cand_cuts=0),
                 lambda: cb.learn_cnet_bic(x, n_cand_cuts=0), lambda: cb.select_cand_cuts(x, n_cand_cuts=0),
                 lambda: cb.select_cand_cuts(x, ess=0.0), lambda: cb.compute_or_bd_scores(x, ess=0.0),
                 lambda: cb.compute_clt_bd_scores(x, ess=-0.1), lambda: cb.learn_cnet_bd(x[0]),
                 lambda: cb.learn_cnet_bic(x[:0]), lambda: cb.learn_cnet_bd(x + 1.0), lambda: cb.learn_cnet_bic(x * np.nan),
                 lambda: cb.learn_cnet_bd(np.zeros((2, 4097), np.float32))):
        with pytest.raises(ValueError):
            call()


def test_cpu_tensor_and_missing_library_raise_hip_error(monkeypatch):
    from deeprob.hip import HipError, clt
    from deeprob.spn.learning import cnet_bayesian as cb
    x = ref.golden('bd_d5')['x']
    for call in (lambda: cb.learn_cnet_bd(torch.from_numpy(x)), lambda: cb.learn_cnet_bic(torch.from_numpy(x)),
                 lambda: cb.select_cand_cuts(torch.from_numpy(x))):
        with pytest.raises(HipError) as e:
            call()
        assert 'make -C deeprob-kit_amd/csrc' in str(e.value)
    monkeypatch.setattr(clt, '_lib', None)
    monkeypatch.setattr(clt, 'LIB_PATH', os.path.join(ROOT, 'no', 'such', 'libdeeprob_clt.so'))
    for call in (lambda: cb.learn_cnet_bd(x), lambda: cb.learn_cnet_bic(x), lambda: cb.select_cand_cuts(x),
                 lambda: cb.compute_or_bd_scores(x), lambda: cb.compute_clt_bd_scores(x)):
        with pytest.raises(HipError) as e:
            call()
        assert 'make -C deeprob-kit_amd/csrc' in str(e.value)


# ---- the header and the import ---------------------------------------------------------------------------------------------
def test_cut_header_entries_parse_and_the_module_is_exported():
    import ctypes
    from deeprob import hip
    from deeprob.hip import clt
    text = open(os.path.join(ROOT, 'include', 'deeprob_clt.h')).read()
    sigs, _, structs = hip.parse_header(text, prefix='dpc', header='deeprob_clt.h')
    entries = sorted(s for s in sigs if s.startswith('dpc_cut_'))
    assert entries == ['dpc_cut_pair_counts'] and not structs
    declared = re.findall(r'\b(dpc_cut_\w+)\s*\(', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    assert sorted(declared) == entries
    restype, argtypes = sigs['dpc_cut_pair_counts']
    assert restype is ctypes.c_int and len(argtypes) == 10 and clt.SIGNATURES['dpc_cut_pair_counts'] == (restype, argtypes)
    import deeprob.spn.learning as learning
    from deeprob.spn.learning import cnet_bayesian
    assert learning.learn_cnet_bd is cnet_bayesian.learn_cnet_bd and learning.learn_cnet_bic is cnet_bayesian.learn_cnet_bic
    for name in ('select_cand_cuts', 'compute_or_bd_scores', 'compute_clt_bd_scores', 'eval_tree_score', 'last_profile'):
        assert callable(getattr(cnet_bayesian, name))
    source = open(cnet_bayesian.__file__).read()
    assert 'scipy' not in source.replace('scipy.special.gammaln', '')


def test_cut_counts_checks_its_entry_table_on_the_host():
    """The kernel indexes device memory with the table: the binding refuses what names no task or no column."""
    from deeprob.hip import cnet
    gen = cnet.Generation.__new__(cnet.Generation)
    gen.n_tasks, gen.d, gen.planes = 2, 5, None
    for tasks, cols in (([0, 2], [1, 1]), ([0, -1], [1, 1]), ([0, 1], [5, 0]), ([0, 1], [0, -1]), ([], []), ([0], [1, 2])):
        with pytest.raises(ValueError):
            gen.cut_counts(tasks, cols)
