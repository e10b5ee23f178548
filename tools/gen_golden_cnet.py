"""Golden BinaryCNet runs of the reference (deeprob/spn/structure/cnet.py) on small binary data sets.  Outputs hold data
only: tests/golden/cnet_<config>.npz with

    data (packed bits) / n_rows / n_vars, alpha, min_n_samples, min_n_features, min_mean_entropy,
    the reference's OR tree in breadth-first order (left child before right): or_id (-1 at a leaf), weights, is_leaf,
    n_node_rows, the leaves' scopes (leaf_scopes / leaf_scope_off) and undirected edge sets as pairs of variable ids
    (leaf_edges / leaf_edge_off), leaf_unique (see below), stop (why a leaf stopped: 1 rows or features, 2 entropy,
    3 gain),
    ll_train of the training rows, fresh_bits (512 fresh rows of the same mixture) and ll_fresh,
    and the margins found: selection_margin, entropy_band, min_abs_gain.

The reference draws every leaf's root from an unseeded generator; the undirected tree and the likelihoods do not depend
on the root (the smoothed joints marginalise exactly to the smoothed priors).

The package scores cuts in float64, the reference in float32, so a fixture is written only if, on the reference's run,
  * every selection's best gain beats the second best by at least 1e-4 relative (and the float64 argmax of
    tests/cnet_ref.py is the reference's choice),
  * every mean entropy that reaches the comparison is at least 1e-3 relative away from min_mean_entropy,
  * every deciding |max gain| is at least 1e-6.

The leaves' spanning trees.  A leaf of a cutset network holds a few dozen rows, and among so few rows many pairs of
variables have the same four counts and so the same mutual information: most leaves have MORE THAN ONE maximum spanning
tree, and which one scipy's Kruskal returns is a matter of its sort.  That cannot be asserted away (no data seed avoids
it), so it is recorded: leaf_unique[k] is True iff the reference's tree is the ONLY maximum spanning tree of the float32
weights mi + 1 the reference hands scipy -- every pair outside the tree strictly lighter than the lightest edge on the
tree path between its ends, the deciding half of gen_golden_clt.tree_is_unique.  The tests compare edge sets, and the
likelihoods of the rows that end in a leaf, exactly where leaf_unique holds; elsewhere they require a tree of the same
sorted edge weights (every maximum spanning tree has them).

    cd tools && PYTHONPATH=<reference checkout> python3 gen_golden_cnet.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.append(ROOT)          # (after the reference: `deeprob` is the reference's, `tests` is this project's)

from tests import cnet_ref  # noqa: E402


def only_spanning_tree(mi, tree):
    """Whether ``tree`` is the only maximum spanning tree of the float32 weights mi + 1."""
    d = len(tree)
    q = (mi.astype(np.float32) + np.float32(1.0)).astype(np.float64)
    depth = np.zeros(d, np.int64)
    for i in range(d):
        j = i
        while tree[j] >= 0:
            j, depth[i] = tree[j], depth[i] + 1
    for u in range(d):
        for v in range(u + 1, d):
            if tree[u] == v or tree[v] == u:
                continue
            a, b, lightest = u, v, np.inf
            while a != b:
                if depth[a] < depth[b]:
                    a, b = b, a
                lightest, a = min(lightest, q[a, tree[a]]), tree[a]
            if not q[u, v] < lightest:
                return False
    return True


OUT = os.path.join(ROOT, 'tests', 'golden')
MAX_BYTES = 150 * 1000
SELECTION_MARGIN, ENTROPY_BAND, MIN_ABS_GAIN = 1e-4, 1e-3, 1e-6


def generate(name):
    from deeprob.spn.structure.cnet import BinaryCNet
    from deeprob.utils.statistics import estimate_priors_joints, compute_mutual_information
    n, d, k, noise, seed, alpha, min_n_samples, min_n_features, min_mean_entropy = cnet_ref.CONFIGS[name]
    data, fresh = cnet_ref.mixture(n, d, k, noise, seed)
    select = BinaryCNet._BinaryCNet__select_variable_entropy
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = BinaryCNet(list(range(d)))
        model.fit(data, alpha=alpha, min_n_samples=min_n_samples, min_n_features=min_n_features,
                  min_mean_entropy=min_mean_entropy)
        ll_train, ll_fresh = model.log_likelihood(data), model.log_likelihood(fresh)
    nodes, at = [model], 0
    while at < len(nodes):
        if nodes[at].clt is None:
            nodes += nodes[at].children
        at += 1
    or_id, weights, rows, stop, scopes, edges, unique = [], [], [], [], [], [], []
    selection, band, smallest_gain, depth_of = np.inf, np.inf, np.inf, {id(model): 1}
    for node in nodes:
        part = data[node.row_indices][:, node.col_indices]
        rows.append(len(node.row_indices))
        scored = part.shape[0] > min_n_samples and part.shape[1] > min_n_features
        if scored:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                ref_idx, ref_entropy, ref_gain = select(part, alpha=alpha)
            mean_entropy, gains = cnet_ref.scores(part, alpha)
            band = min(band, abs(float(ref_entropy) - min_mean_entropy) / min_mean_entropy,
                       abs(mean_entropy - min_mean_entropy) / min_mean_entropy)
            if not ref_entropy < min_mean_entropy:          # the gain decides
                smallest_gain = min(smallest_gain, abs(float(ref_gain)), abs(float(gains.max())))
        if node.clt is not None:
            assert not scored or ref_entropy < min_mean_entropy or ref_gain <= 0
            stop.append(1 if not scored else (2 if ref_entropy < min_mean_entropy else 3))
            or_id.append(-1)
            weights.append([np.nan, np.nan])
            scope = list(node.scope)
            assert scope == [int(c) for c in node.col_indices] and node.clt.scope == scope
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                mi = compute_mutual_information(*estimate_priors_joints(part, alpha=alpha))
            unique.append(len(scope) == 1 or only_spanning_tree(mi, node.clt.tree))
            scopes.append(scope)
            edges.append(cnet_ref.edge_set(scope, node.clt.tree))
            continue
        order = np.sort(gains)
        assert int(np.argmax(gains)) == int(ref_idx) == node.scope.index(node.or_id)
        selection = min(selection, (order[-1] - order[-2]) / abs(order[-1]))
        stop.append(0)
        unique.append(False)
        or_id.append(int(node.or_id))
        weights.append([float(w) for w in node.weights])
        scopes.append(None)
        edges.append(None)
        for c in node.children:
            depth_of[id(c)] = depth_of[id(node)] + 1
    assert selection >= SELECTION_MARGIN, '%s: selection margin %g' % (name, selection)
    assert band >= ENTROPY_BAND, '%s: entropy band %g' % (name, band)
    assert smallest_gain >= MIN_ABS_GAIN, '%s: smallest deciding gain %g' % (name, smallest_gain)

    scope_off = np.concatenate([[0], np.cumsum([0 if s is None else len(s) for s in scopes])])
    edge_off = np.concatenate([[0], np.cumsum([0 if e is None else len(e) for e in edges])])
    flat_edges = np.array([p for e in edges if e for p in e], np.int32).reshape(-1, 2)
    path = os.path.join(OUT, 'cnet_%s.npz' % name)
    np.savez_compressed(
        path, data=np.packbits(data.astype(bool)), n_rows=n, n_vars=d, alpha=alpha, min_n_samples=min_n_samples,
        min_n_features=min_n_features, min_mean_entropy=min_mean_entropy, or_id=np.array(or_id, np.int32),
        weights=np.array(weights, np.float64), is_leaf=np.array(or_id, np.int32) < 0, n_node_rows=np.array(rows, np.int32),
        stop=np.array(stop, np.int8), leaf_unique=np.array(unique, bool), leaf_scopes=np.array([v for s in scopes if s for v in s], np.int32),
        leaf_scope_off=scope_off.astype(np.int32), leaf_edges=flat_edges, leaf_edge_off=edge_off.astype(np.int32),
        ll_train=np.asarray(ll_train, np.float32), fresh_bits=np.packbits(fresh.astype(bool)),
        ll_fresh=np.asarray(ll_fresh, np.float32), selection_margin=selection, entropy_band=band,
        min_abs_gain=smallest_gain)
    size = os.path.getsize(path)
    n_or = int((np.array(or_id) >= 0).sum())
    print(name, 'OR nodes', n_or, 'leaves', len(or_id) - n_or, 'depth', max(depth_of.values()) - 1,
          'stops (rows/features, entropy, gain)', [stop.count(v) for v in (1, 2, 3)], 'leaves with one spanning tree', sum(unique),
          'selection margin %.3g entropy band %.3g min |gain| %.3g' % (selection, band, smallest_gain), 'bytes', size)
    assert size <= MAX_BYTES


if __name__ == '__main__':
    for config in (sys.argv[1:] or cnet_ref.CONFIGS):
        generate(config)
