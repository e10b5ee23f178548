"""Golden BinaryCLT runs of the reference (deeprob/spn/structure/cltree.py) on small binary data sets.  Outputs hold
data only: tests/golden/clt_<config>.npz with

    data (packed bits) / n_rows / n_vars, root (as passed: -1 = drawn from random_state), random_state, alpha,
    ref_root, tree, bfs (the reference's, scipy's order) and params of the fitted model, ll of the training rows,
    a query set (q_values, q_nan: packed bits) with 40 % NaN whose first three rows are all-NaN, a single NaN and
    complete, the reference's ll_mar and mpe (packed bits) on it, mpe_margin (the smallest |score_1 - score_0| over
    the reference's MPE decisions) and pc_json, the reference's save_spn_json text of to_pc().

A data seed is kept only if the maximum spanning tree is UNIQUE in the sense the tests need: the mutual informations of
the tree's edges are mutually distinct and no pair outside the tree has a mutual information equal to a tree edge's
(other ties, among the small values, are harmless: they never decide an edge), and the tree is the only maximum spanning
tree of the float32 weights mi + 1 that the reference hands scipy (the addition rounds values closer than 2^-24 together).
Then any correct spanning-tree algorithm returns the reference's `tree`.  For the configurations whose MPE rows are
compared exactly, a query seed is kept only if mpe_margin >= 1e-3.

    cd tools && PYTHONPATH=<reference checkout> python3 gen_golden_clt.py
"""
import io
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, '..', 'tests', 'golden')
MAX_BYTES = 150 * 1000
MPE_MARGIN = 1e-3

CONFIGS = {     # name -> (variables, rows, root or None, random_state, query rows, exact mpe rows)
    'd16': (16, 500, 0, None, 1000, True),
    'd33': (33, 2000, 7, None, 1000, True),
    'd130': (130, 3000, 64, None, 500, True),
    'drawn24': (24, 800, None, 5, 300, False),
    'd10': (10, 600, 3, None, 200, False),
}
ALPHA = 0.1


def mixture(n_vars, n_rows, seed, n_clusters=4, noise=0.2):
    """Rows of a mixture of ``n_clusters`` binary prototypes: a row copies its cluster's prototype, and each entry is
    replaced by a fair coin with probability ``noise``."""
    rs = np.random.RandomState(seed)
    protos = rs.randint(0, 2, size=(n_clusters, n_vars))
    x = protos[rs.randint(0, n_clusters, size=n_rows)]
    flip = rs.rand(n_rows, n_vars) < noise
    return np.where(flip, rs.randint(0, 2, size=(n_rows, n_vars)), x).astype(np.float32)


def tree_is_unique(mi, tree):
    d = len(tree)
    on_tree = np.zeros((d, d), bool)
    for i, p in enumerate(tree):
        if p >= 0:
            on_tree[i, p] = on_tree[p, i] = True
    upper = np.triu(np.ones((d, d), bool), 1)
    edges = mi[on_tree & upper]
    others = mi[~on_tree & upper]
    if len(np.unique(edges)) != len(edges) or np.isin(others, edges).any():
        return False
    # the reference hands scipy the float32 matrix -(mi + 1): adding 1 rounds mutual informations that differ by less
    # than 2^-24 to one value.  The tree is the only maximum spanning tree of THOSE weights iff every pair outside it is
    # strictly lighter than the lightest edge on the tree path between its ends.
    q = (mi.astype(np.float32) + np.float32(1.0)).astype(np.float64)
    depth = np.zeros(d, np.int64)
    for i in range(d):
        j = i
        while tree[j] >= 0:
            j, depth[i] = tree[j], depth[i] + 1
    for u in range(d):
        for v in range(u + 1, d):
            if on_tree[u, v]:
                continue
            a, b, lightest = u, v, np.inf
            while a != b:
                if depth[a] < depth[b]:
                    a, b = b, a
                lightest, a = min(lightest, q[a, tree[a]]), tree[a]
            if not q[u, v] < lightest:
                return False
    return True


def queries(data, n, seed):
    rs = np.random.RandomState(seed)
    rows = data[rs.randint(0, len(data), size=n)].copy()
    mask = rs.rand(*rows.shape) < 0.4
    mask[0] = True
    mask[1] = False
    mask[1, rows.shape[1] // 2] = True
    mask[2] = False
    rows[mask] = np.nan
    return rows


def mpe_margin(clt, x, filled):
    """The smallest |score of 1 - score of 0| over the decisions of the reference's mpe (cltree.py:297-316)."""
    mis = np.isnan(x)
    messages = clt.message_passing(x, ~mis, return_lls=False, reduce='mpe')
    smallest = np.inf
    for j in clt.bfs:
        rows = mis[:, j]
        if not rows.any():
            continue
        if j == clt.root:
            score = clt.params[j, 0] + messages[j, rows]
        else:
            score = clt.params[j, filled[rows, clt.tree[j]].astype(np.int64)] + messages[j, rows]
        smallest = min(smallest, float(np.min(np.abs(score[:, 1] - score[:, 0]))))
    return smallest


def generate(name):
    from deeprob.spn.structure.cltree import BinaryCLT
    from deeprob.spn.structure.io import save_spn_json
    from deeprob.utils.statistics import estimate_priors_joints, compute_mutual_information
    n_vars, n_rows, root, random_state, n_query, exact_mpe = CONFIGS[name]
    for data_seed in range(1, 100):
        data = mixture(n_vars, n_rows, data_seed)
        clt = BinaryCLT(list(range(n_vars)), root=root)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            clt.fit(data, [[0, 1]] * n_vars, alpha=ALPHA, random_state=random_state)
            mi = compute_mutual_information(*estimate_priors_joints(data, alpha=ALPHA))
        if tree_is_unique(mi, clt.tree):
            break
        print(name, 'data seed', data_seed, 'rejected: the spanning tree is not unique')
    else:
        raise SystemExit('no data seed gave a unique tree for ' + name)
    for query_seed in range(1000, 1200):
        q = queries(data, n_query, query_seed)
        filled = clt.mpe(q)
        margin = mpe_margin(clt, q, filled)
        if not exact_mpe or margin >= MPE_MARGIN:
            break
        print(name, 'query seed', query_seed, 'rejected: mpe margin', margin)
    else:
        raise SystemExit('no query seed gave an mpe margin of %g for %s' % (MPE_MARGIN, name))
    buf = io.StringIO()
    save_spn_json(clt.to_pc(), buf)
    nan = np.isnan(q)
    path = os.path.join(OUT, 'clt_%s.npz' % name)
    np.savez_compressed(
        path, data=np.packbits(data.astype(bool)), n_rows=n_rows, n_vars=n_vars, root=-1 if root is None else root,
        random_state=-1 if random_state is None else random_state, alpha=ALPHA, ref_root=int(clt.root),
        tree=np.asarray(clt.tree, np.int32), bfs=np.asarray(clt.bfs, np.int32), params=np.asarray(clt.params, np.float32),
        ll=np.asarray(clt.log_likelihood(data), np.float32).reshape(-1), n_query=n_query,
        q_values=np.packbits(np.nan_to_num(q).astype(bool)), q_nan=np.packbits(nan),
        ll_mar=np.asarray(clt.log_likelihood(q), np.float32).reshape(-1), mpe=np.packbits(filled.astype(bool)),
        mpe_margin=margin, pc_json=np.asarray(buf.getvalue()), data_seed=data_seed, query_seed=query_seed)
    size = os.path.getsize(path)
    print(name, 'data seed', data_seed, 'query seed', query_seed, 'mpe margin %.3g' % margin, 'bytes', size)
    assert size <= MAX_BYTES


if __name__ == '__main__':
    for config in CONFIGS:
        generate(config)
