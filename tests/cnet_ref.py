"""A numpy restatement of BinaryCNet as this project defines it (include/deeprob_clt.h, "Cutset networks"):
the OR-tree learner with the float64 scores of ``dpc_cnet_scores`` in the header's order of sums, the reference's stop
rules in the reference's order, leaves and leaf queries from tests/clt_ref.py, ``log_likelihood`` in the header's order of
operations, and a brute-force marginal.  It shares no code with the package.

A model is a list of nodes in breadth-first order (left child before right), each a dict: ``or_id`` (-1 at a leaf),
``weights`` (two Python floats), ``children`` (two positions in the list), ``scope``, ``rows`` (indices into the training
data), and at a leaf ``bfs``, ``tree``, ``params`` of its Chow-Liu tree over ``scope``.
"""
import os

import numpy as np

from tests import clt_ref

MISSING = clt_ref.MISSING
GOLDEN = clt_ref.GOLDEN
# name -> (n, d, k, noise, seed; alpha, min_n_samples, min_n_features, min_mean_entropy)
CONFIGS = {
    'd33': (2000, 33, 4, 0.2, 2, 0.01, 50, 1, 0.01),
    'd70': (4097, 70, 5, 0.2, 3, 0.01, 200, 1, 0.01),
    'd130': (4097, 130, 6, 0.2, 21, 0.01, 300, 1, 0.01),
    'd5': (300, 5, 2, 0.3, 4, 0.01, 10, 1, 0.01),
    'd10': (1000, 10, 3, 0.25, 31, 0.01, 60, 3, 0.01),
    'd24': (3000, 24, 4, 0.1, 11, 0.1, 40, 1, 0.30),
}
N_FRESH = 512
_cache = {}


# ---- data and fixtures -----------------------------------------------------------------------------------------------------
def mixture(n, d, k, noise, seed):
    """``(training rows [n, d], fresh rows [N_FRESH, d])`` float32: a prototype per row, XOR flips with probability
    ``noise``."""
    rs = np.random.RandomState(seed)
    protos = rs.rand(k, d) < 0.5

    def draw(rows):
        return (protos[rs.randint(0, k, size=rows)] ^ (rs.rand(rows, d) < noise)).astype(np.float32)
    data = draw(n)
    return data, draw(N_FRESH)


def golden(name):
    """tests/golden/cnet_<name>.npz as a dict with ``x`` (training rows) and ``fresh`` unpacked; loaded once."""
    if name not in _cache:
        f = np.load(os.path.join(GOLDEN, 'cnet_%s.npz' % name))
        g = {k: f[k] for k in f.files}
        g['x'] = clt_ref.unpack(g['data'], int(g['n_rows']), int(g['n_vars']))
        g['fresh'] = clt_ref.unpack(g['fresh_bits'], N_FRESH, int(g['n_vars']))
        _cache[name] = g
    return _cache[name]


def hyper(g):
    return dict(alpha=float(g['alpha']), min_n_samples=int(g['min_n_samples']), min_n_features=int(g['min_n_features']),
                min_mean_entropy=float(g['min_mean_entropy']))


def restated(name, reference_trees=False):
    """The restatement's model of a fixture's data, leaf roots drawn from RandomState(7); computed once.  With
    ``reference_trees`` the leaves take the reference's undirected trees from the fixture instead of learning theirs."""
    key = ('fit', name, reference_trees)
    if key not in _cache:
        g = golden(name)
        trees = golden_structure(g)[3] if reference_trees else None
        _cache[key] = learn(g['x'], random_state=np.random.RandomState(7), trees=trees, **hyper(g))
    return _cache[key]


def queries(name, n=256, share=0.4, seed=5):
    """Query rows of a fixture with ``share`` of the entries NaN: row 0 all NaN, row 1 complete, then fresh rows."""
    g = golden(name)
    rs = np.random.RandomState(seed)
    q = g['fresh'][:n].copy()
    mask = rs.rand(*q.shape) < share
    mask[0] = True
    mask[1] = False
    q[mask] = np.nan
    return q


def edge_set(scope, tree):
    """The undirected edges of a tree over ``scope`` as a sorted list of (smaller id, larger id)."""
    return sorted((min(scope[i], scope[p]), max(scope[i], scope[p])) for i, p in enumerate(tree) if p >= 0)


def golden_structure(g):
    """``(or_id [M], weights [M, 2], leaf scopes, leaf edge sets, row counts [M])`` of a fixture, breadth first."""
    scopes, edges = [], []
    for k in range(len(g['or_id'])):
        if g['or_id'][k] >= 0:
            scopes.append(None)
            edges.append(None)
            continue
        scopes.append(g['leaf_scopes'][g['leaf_scope_off'][k]:g['leaf_scope_off'][k + 1]].tolist())
        e = g['leaf_edges'][g['leaf_edge_off'][k]:g['leaf_edge_off'][k + 1]]
        edges.append(sorted((int(a), int(b)) for a, b in e))
    return g['or_id'], g['weights'], scopes, edges, g['n_node_rows']


def structure(model):
    """The same five of a restated model."""
    or_id = np.array([m['or_id'] for m in model], np.int64)
    weights = np.array([m['weights'] if m['or_id'] >= 0 else [np.nan, np.nan] for m in model], np.float64)
    scopes = [None if m['or_id'] >= 0 else list(m['scope']) for m in model]
    edges = [None if m['or_id'] >= 0 else edge_set(m['scope'], m['tree']) for m in model]
    return or_id, weights, scopes, edges, np.array([len(m['rows']) for m in model], np.int64)


# ---- learning --------------------------------------------------------------------------------------------------------------
def scores(part, alpha):
    """``(mean_entropy, gains [d])`` float64 of a partition ``[n, d]`` (its active columns only): the expressions of
    dpc_cnet_scores, every sum serial in increasing index."""
    part = np.asarray(part).astype(np.float64)
    n, d = part.shape
    ones = part.T @ part                             # (a float64 product of 0/1 values is exact below 2^53 rows)
    c = np.diag(ones).copy()
    n = float(n)
    a2, a4 = 2.0 * alpha, 4.0 * alpha
    with np.errstate(divide='ignore', invalid='ignore'):
        s = 0.0
        for i in range(d):
            p1 = (c[i] + a2) / (n + a4)
            p0 = 1.0 - p1
            s += p0 * np.log(p0) + p1 * np.log(p1)
        mean_entropy = -s / float(d)
        h1, h0 = np.zeros(d), np.zeros(d)
        den1, den0 = c + a4, (n - c) + a4
        for j in range(d):
            o, cj = ones[:, j], c[j]
            c11, c10, c01, c00 = o, c - o, cj - o, ((n - c) - cj) + o
            q0, q1 = (c10 + a2) / den1, (c11 + a2) / den1
            t1 = -(q0 * np.log(q0) + q1 * np.log(q1))
            q0, q1 = (c00 + a2) / den0, (c01 + a2) / den0
            t0 = -(q0 * np.log(q0) + q1 * np.log(q1))
            other = np.arange(d) != j
            h1[other] = h1[other] + t1[other]
            h0[other] = h0[other] + t0[other]
        if d > 1:
            h1, h0 = h1 / float(d - 1), h0 / float(d - 1)
        ratio = c / n if n > 0 else np.zeros(d)
        gains = mean_entropy - (ratio * h1 + (1.0 - ratio) * h0)
    return float(mean_entropy), gains


def rooted(scope, edges, root):
    """The predecessors (positions in ``scope``, -1 at position ``root``) of the undirected tree ``edges`` over ids."""
    position = {v: p for p, v in enumerate(scope)}
    near = [[] for _ in scope]
    for a, b in edges:
        near[position[a]].append(position[b])
        near[position[b]].append(position[a])
    tree, todo = np.full(len(scope), -2, np.int32), [root]
    tree[root] = -1
    while todo:
        i = todo.pop()
        for j in near[i]:
            if tree[j] == -2:
                tree[j] = i
                todo.append(j)
    assert (tree > -2).all() and len(edges) == len(scope) - 1
    return tree


def leaf_mutual_information(data, node, alpha):
    """The float32 mutual information matrix of a leaf's partition (tests/clt_ref.py)."""
    part = np.asarray(data)[node['rows']][:, node['scope']]
    return clt_ref.mutual_information(*clt_ref.priors_joints(clt_ref.counts(part), len(part), alpha))


def edge_weights(mi, scope, edges):
    """The weights of the undirected ``edges`` (pairs of ids) in ``mi``, sorted."""
    position = {v: p for p, v in enumerate(scope)}
    return np.sort(np.array([mi[position[a], position[b]] for a, b in edges], np.float64))


def learn(data, alpha, min_n_samples, min_n_features, min_mean_entropy, random_state=None, roots=None, trees=None,
          trace=None):
    """The model (see the module docstring).  Leaf roots: position ``roots[k]`` for the k-th leaf if given, else drawn as
    ``random_state.choice(len(scope))`` in breadth-first order.  ``trees``: per NODE in breadth-first order, an undirected
    edge set (pairs of ids) to give the leaf instead of learning its tree, or None.  ``trace``: a list that receives
    ``(rows, scope, mean_entropy, gains)`` for every scored node."""
    data = np.asarray(data)
    model = [dict(scope=list(range(data.shape[1])), rows=np.arange(len(data)))]
    at = n_leaves = 0
    while at < len(model):
        node = model[at]
        at += 1
        part = data[node['rows']][:, node['scope']]
        n, d = part.shape
        split = n > min_n_samples and d > min_n_features
        if split:
            mean_entropy, gains = scores(part, alpha)
            best = int(np.argmax(gains))
            if trace is not None:
                trace.append((node['rows'], list(node['scope']), mean_entropy, gains))
            split = not (mean_entropy < min_mean_entropy or gains[best] <= 0)
        if not split:
            root = int(random_state.choice(d)) if roots is None else int(roots[n_leaves])
            n_leaves += 1
            priors, joints = clt_ref.priors_joints(clt_ref.counts(part.reshape(n, d)), n, alpha)
            if trees is None or trees[at - 1] is None:
                tree = clt_ref.prim(root, clt_ref.mutual_information(priors, joints))
            else:
                tree = rooted(node['scope'], trees[at - 1], root)
            bfs = clt_ref.bfs_order(tree)
            node.update(or_id=-1, weights=None, children=None, bfs=bfs, tree=tree,
                        params=clt_ref.cpts(bfs, tree, priors, joints))
            continue
        left = node['rows'][part[:, best] == 0]
        right = node['rows'][part[:, best] == 1]
        left_weight = (len(left) + alpha) / (n + 2 * alpha)
        scope = [v for p, v in enumerate(node['scope']) if p != best]
        node.update(or_id=node['scope'][best], weights=[left_weight, 1 - left_weight], children=[len(model), len(model) + 1])
        model += [dict(scope=scope, rows=left), dict(scope=list(scope), rows=right)]
    return model


def leaf_of_rows(model, x):
    """The position in ``model`` of the leaf every complete row of ``x`` ends in."""
    x = np.asarray(x).astype(np.int64)
    out, stack = np.empty(len(x), np.int64), [(0, np.arange(len(x)))]
    while stack:
        k, idx = stack.pop()
        if model[k]['or_id'] < 0:
            out[idx] = k
            continue
        c = x[idx, model[k]['or_id']]
        stack += [(model[k]['children'][v], idx[c == v]) for v in (0, 1)]
    return out


# ---- queries ---------------------------------------------------------------------------------------------------------------
def lse64(a, b):
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid='ignore'):
        out = hi + np.log1p(np.exp(lo - hi))
    return np.where(hi == -np.inf, -np.inf, out)


def _path_values(model, q):
    """float64 ``[B]`` for complete rows: the log weights root to leaf, then the leaf's terms in its local order."""
    out = np.empty(len(q), np.float64)
    stack = [(0, np.arange(len(q)), np.zeros(len(q), np.float64))]
    while stack:
        k, idx, s = stack.pop()
        node = model[k]
        if node['or_id'] < 0:
            x = q[idx][:, node['scope']]
            params = np.asarray(node['params'], np.float32)
            for i, pa in enumerate(node['tree']):
                s = s + params[i, x[:, pa] if pa >= 0 else 0, x[:, i]].astype(np.float64)
            out[idx] = s
            continue
        c = q[idx, node['or_id']]
        logw = np.log(np.asarray(node['weights'], np.float64))
        for v in (0, 1):
            stack.append((node['children'][v], idx[c == v], s[c == v] + logw[v]))
    return out


def _value(model, k, q, x):
    """V(node k) float64 for the rows of ``q`` (codes) / ``x`` (floats with NaN)."""
    node = model[k]
    if len(q) == 0:
        return np.zeros(0, np.float64)
    if node['or_id'] < 0:
        return clt_ref.log_likelihood(node['bfs'], node['tree'], node['params'], x[:, node['scope']]).astype(np.float64)
    c = q[:, node['or_id']]
    logw = np.log(np.asarray(node['weights'], np.float64))
    out = np.empty(len(q), np.float64)
    branch = []
    for v in (0, 1):
        go = (c == v) | (c == MISSING)
        full = np.empty(len(q), np.float64)
        full[go] = logw[v] + _value(model, node['children'][v], q[go], x[go])
        branch.append(full)
        out[c == v] = full[c == v]
    missing = c == MISSING
    out[missing] = lse64(branch[0][missing], branch[1][missing])
    return out


def log_likelihood(model, x):
    """float32 ``[B]``, the header's two paths; NaN = marginalised."""
    x = np.asarray(x, np.float32)
    q = clt_ref.codes(x)
    out = np.empty(len(q), np.float32)
    full = ~(q == MISSING).any(axis=1)
    out[full] = _path_values(model, q[full]).astype(np.float32)
    out[~full] = _value(model, 0, q[~full], x[~full]).astype(np.float32)
    return out


def brute_marginal(model, x):
    """float64 ``[B]``: log of the sum, over every completion of a row's NaN entries, of the complete-row likelihood
    (all 2^D complete rows are evaluated once: small D only)."""
    x = np.asarray(x, np.float32)
    d = x.shape[1]
    every = np.array([[(v >> i) & 1 for i in range(d)] for v in range(2 ** d)], np.int64)
    p = np.exp(_path_values(model, every))
    out = np.empty(len(x), np.float64)
    for r, row in enumerate(x):
        obs = ~np.isnan(row)
        out[r] = np.log(p[(every[:, obs] == row[obs]).all(axis=1)].sum())
    return out


# ---- what the tests ask of the leaves' trees ---------------------------------------------------------------------------------
def assert_leaf_trees(name, edges_by_node):
    """``edges_by_node``: per node in breadth-first order, the undirected edge set of the leaf's tree (None at an OR node)
    of a model with the fixture's OR tree.  Where the reference's tree is the only maximum spanning tree (``leaf_unique``,
    tools/gen_golden_cnet.py) the edge set is the reference's.  Elsewhere -- equal mutual informations, several maximum
    spanning trees, the reference's choice an accident of scipy's sort -- the tree must be one of them: its sorted edge
    weights are the reference's.  The reference runs Kruskal on float32(mi + 1), which rounds weights closer than 2^-23
    together, so two of its maximum spanning trees can differ by less than 2^-23 per sorted weight in mi itself: that is
    the tolerance."""
    g = golden(name)
    _, _, scopes, want, _ = golden_structure(g)
    base = restated(name)
    assert len(edges_by_node) == len(want)
    for k, (got, ref) in enumerate(zip(edges_by_node, want)):
        if ref is None:
            assert got is None, k
        elif g['leaf_unique'][k]:
            assert sorted(got) == ref, k
        else:
            mi = leaf_mutual_information(g['x'], base[k], float(g['alpha']))
            a, b = edge_weights(mi, scopes[k], got), edge_weights(mi, scopes[k], ref)
            assert a.shape == b.shape and (len(a) == 0 or np.max(np.abs(a - b)) <= 2.0 ** -23), k
