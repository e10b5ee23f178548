"""BinaryCLT without a device: the numpy restatement (tests/clt_ref.py) against the reference's goldens, the host side of
the package (graph, statistics from given counts, constructor, ``to_pc``) against both, the argument handling, and the
header of the CLT library."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import clt_ref as ref
from tests import learnspn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bar(got, want):
    """The project's bar: max |got - want| / max(1, |want|)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


# ---- the restatement against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ref.CONFIGS)
def test_fixture_holds_what_the_tests_need(name):
    g = ref.golden(name)
    q = g['q']
    assert np.isnan(q[0]).all() and np.isnan(q[1]).sum() == 1 and not np.isnan(q[2]).any()
    assert 0.3 < np.isnan(q).mean() < 0.5
    assert int(g['tree'][int(g['ref_root'])]) == -1 and (name not in ref.EXACT_MPE or float(g['mpe_margin']) >= 1e-3)
    assert set(np.unique(g['x'])) <= {0.0, 1.0}


@pytest.mark.parametrize('name', ref.CONFIGS)
def test_restatement_fit_reproduces_reference(name):
    g = ref.golden(name)
    bfs, tree, params = ref.restated(name)
    assert np.array_equal(tree, g['tree'])
    assert np.max(np.abs(params - g['params'])) <= 1e-6
    assert sorted(bfs) == list(range(len(tree))) and bfs[0] == int(g['ref_root'])


@pytest.mark.parametrize('name', ref.CONFIGS)
def test_restatement_log_likelihood_reproduces_reference(name):
    g = ref.golden(name)
    bfs, tree, params = ref.restated(name)
    assert bar(ref.log_likelihood(bfs, tree, params, g['x']), g['ll']) <= 1e-5
    ll_mar = ref.log_likelihood(bfs, tree, params, g['q'])
    assert bar(ll_mar, g['ll_mar']) <= 1e-5
    assert abs(float(ll_mar[0])) <= 1e-5            # the all-NaN row


@pytest.mark.parametrize('name', ref.CONFIGS)
def test_restatement_mpe_is_no_less_likely_than_the_reference(name):
    g = ref.golden(name)
    bfs, tree, params = ref.restated(name)
    got = ref.mpe(bfs, tree, params, g['q'])
    obs = ~np.isnan(g['q'])
    assert np.array_equal(got[obs], g['q'][obs]) and set(np.unique(got)) <= {0.0, 1.0}
    mine, theirs = ref.log_likelihood64(tree, params, got), ref.log_likelihood64(tree, params, g['mpe_rows'])
    assert (mine >= theirs - 1e-5 * np.maximum(1.0, np.abs(theirs))).all()
    if name in ref.EXACT_MPE:
        assert np.array_equal(got, g['mpe_rows'])


def test_restatement_mpe_is_optimal_by_enumeration():
    g = ref.golden('d10')
    bfs, tree, params = ref.restated('d10')
    q = g['q'][:60]
    best = ref.log_likelihood64(tree, params, ref.mpe(bfs, tree, params, q))
    every = np.array([[(v >> i) & 1 for i in range(10)] for v in range(1024)], np.float32)
    ll_every = ref.log_likelihood64(tree, params, every)
    for r, row in enumerate(q):
        obs = ~np.isnan(row)
        agrees = (every[:, obs] == row[obs]).all(axis=1)
        assert best[r] >= ll_every[agrees].max() - 1e-9


# ---- deeprob.utils.graph -------------------------------------------------------------------------------------------------
def test_tree_node_and_build_tree_structure():
    from deeprob.utils.graph import TreeNode, build_tree_structure
    root = build_tree_structure([2, 2, -1, 0, 0, 1])
    assert root.get_id() == 2 and root.get_parent() is None and not root.is_leaf()
    assert [c.get_id() for c in root.get_children()] == [0, 1]
    assert [c.get_id() for c in root.get_children()[0].get_children()] == [3, 4]
    assert root.get_n_nodes() == 6 and root.get_children()[1].get_children()[0].is_leaf()
    assert root.get_tree_scope() == ([-1, 0, 0, 1, 1, 2], [2, 0, 1, 3, 4, 5])
    named = build_tree_structure(np.array([1, -1, 1]), scope=[7, 5, 9])
    assert named.get_id() == 5 and [c.get_id() for c in named.get_children()] == [7, 9]
    a, b = TreeNode(1), TreeNode(2)
    c = TreeNode(3, parent=a)
    c.set_parent(b)                     # a node keeps its first parent
    assert c.get_parent() is a and b.is_leaf()
    for bad, scope, msg in (([0, 1], None, "Invalid tree structure"), ([-1, -1], None, "Invalid tree structure"),
                            ([-1, 0], [3, 3], "The scope must not contain duplicates"),
                            ([-1, 0], [3], "Invalid scope's number of variables")):
        with pytest.raises(ValueError) as e:
            build_tree_structure(bad, scope)
        assert str(e.value) == msg


def test_bfs_ordering_is_children_ascending():
    from deeprob.utils.graph import compute_bfs_ordering
    assert compute_bfs_ordering([2, 2, -1, 0, 0, 1]) == [2, 0, 1, 3, 4, 5]
    assert compute_bfs_ordering([3, 3, 3, -1]) == [3, 0, 1, 2]
    chain = np.array([1, 2, 3, -1], np.int32)
    out = compute_bfs_ordering(chain)
    assert isinstance(out, np.ndarray) and out.dtype == np.int32 and out.tolist() == [3, 2, 1, 0]
    assert compute_bfs_ordering([-1]) == [0]


def test_maximum_spanning_tree_by_hand():
    from deeprob.utils.graph import maximum_spanning_tree
    w = np.array([[0, 5, 1, 1], [5, 0, 4, 1], [1, 4, 0, 3], [1, 1, 3, 0]], np.float32)     # the path 0-1-2-3
    for root, want in ((0, [-1, 0, 1, 2]), (2, [1, 2, -1, 2]), (3, [1, 2, 3, -1])):
        bfs, tree = maximum_spanning_tree(root, w)
        assert tree.tolist() == want and tree.dtype == np.int32 and bfs[0] == root and sorted(bfs) == [0, 1, 2, 3]
    bfs, tree = maximum_spanning_tree(0, np.zeros((1, 1), np.float32))
    assert bfs.tolist() == [0] and tree.tolist() == [-1]


@pytest.mark.parametrize('name', ref.CONFIGS)
def test_package_host_fit_from_counts_reproduces_reference(name):
    """The package's float32 arithmetic, spanning tree, order and CPTs from exact counts (here numpy's; on the device
    dpc_pair_counts': tests/test_clt_gpu.py)."""
    from deeprob.utils import statistics as S
    from deeprob.utils.graph import maximum_spanning_tree
    from deeprob.spn.structure.cltree import BinaryCLT
    g = ref.golden(name)
    priors, joints = S.priors_joints_from_counts(ref.counts(g['x']), len(g['x']), float(g['alpha']))
    want_priors, want_joints = ref.priors_joints(ref.counts(g['x']), len(g['x']), float(g['alpha']))
    assert np.array_equal(priors, want_priors) and np.array_equal(joints, want_joints)
    mi = S.compute_mutual_information(priors, joints)
    assert mi.dtype == np.float32 and np.array_equal(mi, mi.T) and not mi.diagonal().any()
    bfs, tree = maximum_spanning_tree(int(g['ref_root']), mi)
    assert np.array_equal(tree, g['tree']) and np.array_equal(bfs, ref.restated(name)[0])
    params = np.log(BinaryCLT.compute_clt_parameters(bfs, tree, priors, joints))
    assert np.max(np.abs(params - g['params'])) <= 1e-6


def test_mutual_information_rejects_inconsistent_tables():
    from deeprob.utils import statistics as S
    priors, joints = ref.priors_joints(ref.counts(ref.golden('d10')['x']), 600, 0.1)
    for p, j, msg in ((priors[:5], joints, "There are inconsistencies between priors and joints distributions"),
                      (priors * 0.5, joints, "The priors probability distributions are not valid"),
                      (priors, joints * 0.5, "The joints probability distributions are not valid ")):
        with pytest.raises(ValueError) as e:
            S.compute_mutual_information(p, j)
        assert str(e.value) == msg
    skew = joints.copy()
    skew[0, 1, 0, 1] += 0.25
    with pytest.raises(ValueError) as e:
        S.compute_mutual_information(priors, skew)
    assert str(e.value) == "The joints probability distributions are expected to be symmetric"
    with pytest.raises(ValueError) as e:
        S.priors_joints_from_counts(np.ones((2, 2), np.int64), 4, alpha=-0.5)
    assert str(e.value) == "The Laplace smoothing factor must be non-negative"


def test_children_lists_of_the_binding_follow_the_header():
    from deeprob.hip import clt
    for name in ('d16', 'd130'):
        bfs, tree, _ = ref.restated(name)
        off, idx = clt.children_csr(bfs, tree)
        lists = ref.children_lists(bfs, tree)
        assert off.dtype == idx.dtype == np.int32 and off[0] == 0 and off[-1] == len(tree) - 1
        assert [idx[off[i]:off[i + 1]].tolist() for i in range(len(tree))] == lists
        position = {int(v): p for p, v in enumerate(bfs)}
        assert all(position[a] > position[b] for l in lists for a, b in zip(l, l[1:]))


def test_device_tree_rejects_tables_that_are_no_tree():
    """Checked on the host before anything is uploaded: the kernels index device memory with these tables."""
    from deeprob.hip import clt
    params = np.zeros((3, 2, 2), np.float32)
    for bfs, tree in (([0, 1], [-1, 0, 0]), ([0, 1, 1], [-1, 0, 0]), ([0, 1, 3], [-1, 0, 0]), ([0, 1, 2], [-1, 2, 1]),
                      ([0, 1, 2], [-1, 0, 5]), ([0, 1, 2], [-1, -2, 0]), ([1, 0, 2], [-1, 0, 0]), ([0, 1, 2], [-1, -1, 0])):
        with pytest.raises(ValueError) as e:
            clt.DeviceTree(bfs, tree, params, 'cpu')
        assert str(e.value) == "bfs and tree do not describe one rooted tree", (bfs, tree)
    with pytest.raises(ValueError):
        clt.DeviceTree([0, 1, 2], [-1, 0, 0], params[:2], 'cpu')


# ---- the class -------------------------------------------------------------------------------------------------------------
def test_constructor_checks_and_messages():
    from deeprob.spn.structure.cltree import BinaryCLT
    from deeprob.spn.structure.leaf import Leaf, LeafType
    for kwargs, msg in ((dict(scope=[]), "The scope must not be empty"),
                        (dict(scope=[1, 1]), "The scope must not contain duplicates"),
                        (dict(scope=[4, 5], root=3), "The root variable must be in scope"),
                        (dict(scope=[4, 5], root=3, tree=[-1, 0]), "The root variable must be in scope"),
                        (dict(scope=[4, 5], tree=[-1, 0, 0]), "Invalid tree structure's number of variables"),
                        (dict(scope=[4, 5], tree=[-1, -1]), "Invalid tree structure's root node"),
                        (dict(scope=[4, 5], tree=[1, 0]), "Invalid tree structure's root node"),
                        (dict(scope=[4, 5], root=5, tree=[-1, 0]), "Invalid tree structure's root node"),
                        (dict(scope=[4, 5], params=[[[0.0, 0.0]]]), "Invalid conditional probability table (CPT) shape"),
                        (dict(scope=[4], params=[[[0.0, 0.0], [0.0, 0.0]]]),
                         "Invalid conditional probability table (CPT) values")):
        with pytest.raises(ValueError) as e:
            BinaryCLT(**kwargs)
        assert str(e.value) == msg, kwargs
    half = float(np.log(0.5))
    clt = BinaryCLT([4, 9, 6], root=9, tree=[1, -1, 1], params=[[[half, half]] * 2] * 3)
    assert isinstance(clt, Leaf) and BinaryCLT.LEAF_TYPE == LeafType.DISCRETE
    assert clt.root == 1 and clt.tree.dtype == np.int32 and list(clt.bfs) == [1, 0, 2] and clt.params.dtype == np.float32
    assert clt.params_count() == 1 + 3 + 12
    d = clt.params_dict()
    assert d['root'] == 9 and d['tree'] is clt.tree and d['params'] is clt.params
    assert BinaryCLT([4, 9]).params_dict()['root'] is None and BinaryCLT([4, 9], root=9).root == 1
    assert BinaryCLT([4, 9], tree=[1, -1]).root == 1
    assert clt.get_scopes() == [[6, 4, 9]]
    with pytest.raises(NotImplementedError) as e:
        clt.moment()
    assert str(e.value) == "Computation of moments on Binary CLTs not yet implemented"


def test_fit_argument_messages():
    from deeprob.spn.structure.cltree import BinaryCLT
    data = ref.golden('d10')['x']
    doms = [[0, 1]] * 10
    for kwargs, msg in ((dict(domain=doms[:9]), "Each data column should correspond to a random variable having a domain"),
                        (dict(domain=doms[:9] + [[0, 1, 2]]), "The domains must be binary for a Binary CLT distribution"),
                        (dict(domain=doms, alpha=-1.0), "The Laplace smoothing factor must be non-negative"),
                        (dict(domain=doms, random_state='x'),
                         "The random state must be either None, a seed integer or a Numpy RandomState object")):
        with pytest.raises(ValueError) as e:
            BinaryCLT(list(range(10))).fit(data, **kwargs)
        assert str(e.value) == msg
    for bad in (np.nan, 2.0, 0.5, -1.0):
        spoiled = data.copy()
        spoiled[7, 3] = bad
        with pytest.raises(ValueError) as e:
            BinaryCLT(list(range(10)), root=0).fit(spoiled, doms)
        assert 'binary' in str(e.value)


def test_cpu_tensor_raises_hip_error():
    from deeprob.hip import HipError
    from deeprob.spn.structure.cltree import BinaryCLT
    g = ref.golden('d10')
    with pytest.raises(HipError):
        BinaryCLT(list(range(10)), root=0).fit(torch.from_numpy(g['x']), [[0, 1]] * 10)
    clt = BinaryCLT(list(range(10)), tree=g['tree'], params=g['params'])
    for query in (clt.log_likelihood, clt.likelihood, clt.mpe, clt.sample):
        with pytest.raises(HipError) as e:
            query(torch.from_numpy(g['q']))
        assert 'make -C deeprob-kit_amd/csrc' in str(e.value)


@pytest.mark.parametrize('name', ref.CONFIGS)
def test_to_pc_is_the_reference_circuit(name):
    from deeprob.spn.structure.cltree import BinaryCLT
    from deeprob.spn.structure.io import FlatSpn, spn_to_digraph
    g = ref.golden(name)
    pc = BinaryCLT(list(range(int(g['n_vars']))), tree=g['tree'], params=g['params']).to_pc()
    assert isinstance(pc, FlatSpn)
    assert learnspn_ref.graphs_differ(spn_to_digraph(pc), json.loads(str(g['pc_json']))) is None


def test_to_pc_and_get_scopes_use_the_scope_ids():
    from deeprob.spn.structure.cltree import BinaryCLT
    from deeprob.spn.structure.io import spn_to_digraph
    half = float(np.log(0.5))
    clt = BinaryCLT([3, 0, 2, 1], tree=[-1, 0, 0, 2], params=[[[half, half]] * 2] * 4)
    assert clt.get_scopes() == [[1, 2], [1, 2, 0, 3]]
    nodes = spn_to_digraph(clt.to_pc())['nodes']
    assert nodes[0]['class'] == 'Sum' and sorted(nodes[0]['scope']) == [0, 1, 2, 3]
    assert sum(n['class'] == 'Bernoulli' for n in nodes) == 8 and sum(n['class'] == 'Sum' for n in nodes) == 7


# ---- the header and the library --------------------------------------------------------------------------------------------
def test_clt_header_parses_and_matches_the_exports():
    from deeprob import hip
    from deeprob.hip import clt
    text = open(os.path.join(ROOT, 'include', 'deeprob_clt.h')).read()
    sigs, consts, structs = hip.parse_header(text, prefix='dpc', header='deeprob_clt.h')
    assert sigs == clt.SIGNATURES and consts['DPC_OK'] == 0 and consts['DPC_MAX_D'] >= 1024 and not structs
    assert consts['DPC_MISSING'] == ref.MISSING
    declared = re.findall(r'\b(dpc_\w+)\s*\(', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    assert sorted(declared) == sorted(set(declared)) == sorted(sigs), 'every entry point is declared once'
    out = subprocess.run(['nm', '-D', '--defined-only', clt.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = sorted(l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith('dpc_'))
    assert exported == sorted(sigs)


def test_missing_clt_library_names_the_make_command(monkeypatch):
    from deeprob.hip import HipError, clt
    from deeprob.spn.structure.cltree import BinaryCLT
    monkeypatch.setattr(clt, '_lib', None)
    monkeypatch.setattr(clt, 'LIB_PATH', os.path.join(ROOT, 'no', 'such', 'libdeeprob_clt.so'))
    with pytest.raises(HipError) as e:
        clt.load_library()
    assert 'make -C deeprob-kit_amd/csrc' in str(e.value)
    g = ref.golden('d10')
    with pytest.raises(HipError) as e:
        BinaryCLT(list(range(10)), tree=g['tree'], params=g['params']).log_likelihood(g['q'])
    assert 'make -C deeprob-kit_amd/csrc' in str(e.value)
    with pytest.raises(HipError) as e:
        BinaryCLT(list(range(10)), root=0).fit(g['x'], [[0, 1]] * 10)
    assert 'make -C deeprob-kit_amd/csrc' in str(e.value)

