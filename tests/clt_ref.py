"""A numpy restatement of BinaryCLT as this project defines it (include/deeprob_clt.h, DESIGN.md "Chow-Liu trees"):
``fit`` from exact integer counts in the float32 expressions of the reference (utils/statistics.py:33-109,
cltree.py:105-115), Prim's maximum spanning tree, the project's breadth-first order (children ascending), message
passing in the header's order of operations, and the replay of the counter-based sampler.  It shares no code with the
package: the tests hold each against the goldens and against the other.
"""
import os
from collections import deque

import numpy as np

from tests.flat_spn_query_ref import uniform01

MISSING = 2


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CONFIGS = ['d16', 'd33', 'd130', 'drawn24', 'd10']
EXACT_MPE = ['d16', 'd33', 'd130']          # the reference's smallest MPE margin is >= 1e-3 there (tools/gen_golden_clt.py)
_cache = {}


# ---- fixtures ------------------------------------------------------------------------------------------------------------
def golden(name):
    """The fixture tests/golden/clt_<name>.npz as a dict, with ``x`` (training rows), ``q`` (query rows with NaN) and
    ``mpe_rows`` (the reference's completion) unpacked; loaded once."""
    if name not in _cache:
        f = np.load(os.path.join(GOLDEN, 'clt_%s.npz' % name))
        g = {k: f[k] for k in f.files}
        g['x'] = golden_data(g)
        g['q'], g['mpe_rows'] = golden_queries(g)
        _cache[name] = g
    return _cache[name]


def restated(name):
    """``(bfs, tree, params)`` of the restatement's fit on a fixture's data; computed once."""
    key = ('fit', name)
    if key not in _cache:
        g = golden(name)
        _cache[key] = fit(g['x'], int(g['ref_root']), float(g['alpha']))
    return _cache[key]


def unpack(bits, rows, cols):
    return np.unpackbits(bits)[:rows * cols].reshape(rows, cols).astype(np.float32)


def golden_data(g):
    return unpack(g['data'], int(g['n_rows']), int(g['n_vars']))


def golden_queries(g):
    """``(query rows with NaN, the reference's mpe completion)``."""
    b, d = int(g['n_query']), int(g['n_vars'])
    q = unpack(g['q_values'], b, d)
    q[unpack(g['q_nan'], b, d) == 1] = np.nan
    return q, unpack(g['mpe'], b, d)


# ---- learning ------------------------------------------------------------------------------------------------------------
def counts(data):
    """X^T X in exact integers (a float64 product of 0/1 values is exact below 2^53 rows)."""
    x = np.asarray(data).astype(np.float64)
    return np.rint(x.T @ x).astype(np.int64)


def priors_joints(ones, n, alpha):
    d = len(ones)
    c = np.diag(ones).astype(np.int64)
    cells = np.zeros((d, d, 2, 2), np.int64)
    for i in range(d):
        cells[i, :, 1, 1] = ones[i]
        cells[i, :, 0, 1] = c - ones[i]
        cells[i, :, 1, 0] = c[i] - ones[i]
        cells[i, :, 0, 0] = n - c - c[i] + ones[i]
    denominator = n + 4 * alpha
    priors = np.zeros((d, 2), np.float32)
    priors[:, 1] = (c.astype(np.float32) + 2 * alpha) / denominator
    priors[:, 0] = 1.0 - priors[:, 1]
    joints = (cells.astype(np.float32) + alpha) / denominator
    for i in range(d):
        joints[i, i] = [[priors[i, 0], 0.0], [0.0, priors[i, 1]]]
    return priors, joints


def mutual_information(priors, joints):
    outers = np.multiply.outer(priors, priors).transpose([0, 2, 1, 3])
    with np.errstate(divide='ignore', invalid='ignore'):
        mi = np.sum(joints * (np.log(joints) - np.log(outers)), axis=(2, 3))
    np.fill_diagonal(mi, 0.0)
    return mi


def prim(root, w):
    d = len(w)
    tree, inside = np.full(d, -1, np.int32), np.zeros(d, bool)
    inside[root] = True
    while not inside.all():                # (O(D^3): the fixtures are small)
        us, vs = np.flatnonzero(inside), np.flatnonzero(~inside)
        crossing = w[np.ix_(us, vs)]
        a, b = np.unravel_index(np.argmax(crossing), crossing.shape)
        tree[vs[b]] = us[a]
        inside[vs[b]] = True
    return tree


def bfs_order(tree):
    """Breadth first from the root, the children of a node in increasing index."""
    d = len(tree)
    kids = [[j for j in range(d) if tree[j] == i] for i in range(d)]
    order, queue = [], deque([int(np.flatnonzero(np.asarray(tree) == -1)[0])])
    while queue:
        i = queue.popleft()
        order.append(i)
        queue.extend(kids[i])
    return np.asarray(order, np.int32)


def children_lists(bfs, tree):
    """The children of every node in decreasing position in ``bfs`` (the header's list order)."""
    lists = [[] for _ in tree]
    for j in list(bfs)[:0:-1]:
        lists[tree[j]].append(int(j))
    return lists


def cpts(bfs, tree, priors, joints):
    d = len(tree)
    params = np.zeros((d, 2, 2), np.float32)
    for i in range(d):
        pa = tree[i]
        for l in range(2):
            for k in range(2):
                params[i, l, k] = priors[i, k] if pa < 0 else joints[i, pa, k, l] * np.reciprocal(priors[pa, l])
    params /= np.sum(params, axis=2, keepdims=True)
    return np.log(params)


def fit(data, root, alpha):
    """``(bfs, tree, params)``."""
    priors, joints = priors_joints(counts(data), len(data), alpha)
    tree = prim(root, mutual_information(priors, joints))
    bfs = bfs_order(tree)
    return bfs, tree, cpts(bfs, tree, priors, joints)


# ---- queries -------------------------------------------------------------------------------------------------------------
def codes(x):
    x = np.asarray(x, np.float32)
    return np.where(np.isnan(x), MISSING, (np.nan_to_num(x) != 0).astype(np.int64))


def lse(a, b):
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid='ignore'):
        out = (hi + np.log1p(np.exp(lo - hi))).astype(np.float32)
    return np.where(hi == -np.inf, np.float32(-np.inf), out)


def _message(t, kids, j, b):
    m = np.zeros((2, b), np.float32)
    for c in kids[j]:
        m = m + t[c]
    return m


def _contribution(params, j, c, m, reduce):
    """t_j [2 (l), B]."""
    rows = np.arange(len(c))
    obs = c != MISSING
    k = np.where(obs, c, 0)
    out = np.empty((2, len(c)), np.float32)
    for l in range(2):
        seen = params[j, l][k] + m[k, rows]
        a0, a1 = params[j, l, 0] + m[0], params[j, l, 1] + m[1]
        out[l] = np.where(obs, seen, np.maximum(a0, a1) if reduce == 'mpe' else lse(a0, a1))
    return out


def upward(bfs, tree, params, q, reduce):
    kids = children_lists(bfs, tree)
    d, b = len(tree), q.shape[0]
    t = np.zeros((d, 2, b), np.float32)
    for j in list(bfs)[:0:-1]:
        t[j] = _contribution(params, j, q[:, j], _message(t, kids, j, b), reduce)
    return t, kids


def log_likelihood(bfs, tree, params, x):
    """float32, the header's two paths."""
    params = np.asarray(params, np.float32)
    q = codes(x)
    b, d = q.shape
    out = np.empty(b, np.float32)
    full = ~(q == MISSING).any(axis=1)
    out[full] = log_likelihood64(tree, params, q[full]).astype(np.float32)
    if (~full).any():
        qm = q[~full]
        t, kids = upward(bfs, tree, params, qm, 'mar')
        root = int(bfs[0])
        m, c, rows = _message(t, kids, root, len(qm)), qm[:, root], np.arange(len(qm))
        k = np.where(c != MISSING, c, 0)
        out[~full] = np.where(c != MISSING, params[root, 0][k] + m[k, rows],
                              lse(params[root, 0, 0] + m[0], params[root, 0, 1] + m[1]))
    return out


def log_likelihood64(tree, params, complete):
    """float64 sum of params[i][x_parent(i)][x_i] over i in order, for rows without NaN."""
    x = np.asarray(complete).astype(np.int64)
    s = np.zeros(len(x), np.float64)
    for i in range(len(tree)):
        s += np.asarray(params, np.float32)[i, x[:, tree[i]] if tree[i] >= 0 else 0, x[:, i]].astype(np.float64)
    return s


def _downward(bfs, tree, params, x, reduce, seed=0):
    params = np.asarray(params, np.float32)
    x = np.array(x, np.float32, copy=True)
    q = codes(x)
    b, d = q.shape
    t, kids = upward(bfs, tree, params, q, reduce)
    value = np.zeros((d, b), np.int64)
    near = np.zeros(b, bool)
    rows = np.arange(b)
    for j in bfs:
        pa = tree[j]
        xp = value[pa] if pa >= 0 else np.zeros(b, np.int64)
        m = _message(t, kids, j, b)
        s0, s1 = params[j, xp, 0] + m[0], params[j, xp, 1] + m[1]
        if reduce == 'mpe':
            pick = (s1 > s0).astype(np.int64)
        else:
            p = np.exp(params[j, xp, 1] + (m[1] if pa < 0 else m[xp, rows])).astype(np.float32)
            u = uniform01(seed, rows.astype(np.uint64) * np.uint64(d) + np.uint64(j))
            pick = (u < p).astype(np.int64)
            near |= (q[:, j] == MISSING) & (np.abs(u.astype(np.float64) - p.astype(np.float64)) < 1e-5)
        value[j] = np.where(q[:, j] == MISSING, pick, q[:, j])
        fill = q[:, j] == MISSING
        x[fill, j] = value[j][fill]
    return x, near


def mpe(bfs, tree, params, x):
    return _downward(bfs, tree, params, x, 'mpe')[0]


def sample_replay(bfs, tree, params, x, seed):
    """(filled inputs, rows in which a draw lies within 1e-5 of its probability)."""
    return _downward(bfs, tree, params, x, 'mar', seed)
