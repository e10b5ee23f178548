"""A numpy restatement of the posterior marginals of a Chow-Liu tree and of a cutset network (include/deeprob_clt.h,
``dpc_mar_clt`` and ``dpc_mar_cnet``), vectorised over rows and in the header's order of operations, and the
same marginals by enumeration of all 2^D rows.  It shares no code with the package; trees are ``(bfs, tree, params)`` of
tests/clt_ref.py, networks the node lists of tests/cnet_ref.py.

``dtype`` is the arithmetic of a tree's two passes: float32 is what the device runs, float64 is what the device is held
against.  The OR level of a network -- ``log P(e)``, the prefix weights, ``pi_l`` and the accumulators -- is float64 in
both, as it is on the device.
"""
import numpy as np

from tests import clt_ref
from tests import cnet_ref
from tests.clt_ref import MISSING


def lse(a, b):
    """``hi + log1p(exp(lo - hi))`` in the dtype of the arguments, -inf when hi = -inf."""
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid='ignore'):
        out = hi + np.log1p(np.exp(lo - hi))
    return np.where(hi == -np.inf, -np.inf, out).astype(hi.dtype)


def _pull(t, kids, j, b, dtype):
    m = np.zeros((2, b), dtype)
    for c in kids[j]:
        m = m + t[c]
    return m


def two_passes(bfs, tree, params, q, dtype):
    """``(V [B], p1 [B, d])`` of a tree over the codes ``q`` ``[B, d]``: V is the value the upward pass ends with at the root
    (the log marginal of the observed entries), ``p1[:, j] = exp(b_j[1])`` the posterior probability that position j is 1
    (NaN in a row whose evidence has probability zero)."""
    params = np.asarray(params, np.float32).astype(dtype)
    kids = clt_ref.children_lists(bfs, tree)
    b, d = q.shape
    rows = np.arange(b)
    ninf = dtype(-np.inf)
    t = np.zeros((d, 2, b), dtype)
    for j in list(bfs)[:0:-1]:
        m, c = _pull(t, kids, j, b, dtype), q[:, j]
        obs, k = c != MISSING, np.where(c != MISSING, c, 0)
        for l in range(2):
            t[j, l] = np.where(obs, params[j, l][k] + m[k, rows], lse(params[j, l, 0] + m[0], params[j, l, 1] + m[1]))
    root = int(bfs[0])
    m, c = _pull(t, kids, root, b, dtype), q[:, root]
    k = np.where(c != MISSING, c, 0)
    value = np.where(c != MISSING, params[root, 0][k] + m[k, rows], lse(params[root, 0, 0] + m[0], params[root, 0, 1] + m[1]))
    p1 = np.empty((b, d), dtype)
    with np.errstate(invalid='ignore'):
        for j in bfs:
            pa, c = tree[j], q[:, j]
            m = _pull(t, kids, j, b, dtype)                 # the children's slots still hold their t
            ev = [np.where(c == 1, ninf, dtype(0)), np.where(c == 0, ninf, dtype(0))]
            if pa < 0:
                a = [params[j, 0, k] + m[k] + ev[k] for k in range(2)]
            else:
                cav = [np.where(t[pa, l] == ninf, ninf, t[pa, l] - t[j, l]) for l in range(2)]
                a = [lse(cav[0] + params[j, 0, k], cav[1] + params[j, 1, k]) + m[k] + ev[k] for k in range(2)]
            z = lse(a[0], a[1])
            t[j, 0], t[j, 1] = a[0] - z, a[1] - z           # b_j takes the slot of t_j
            p1[:, j] = np.exp(t[j, 1])
    return value.astype(dtype), p1


def tree_marginals(bfs, tree, params, x, dtype=np.float64):
    """``[B, D]`` in ``dtype``: ``x`` with every NaN entry replaced by ``p(x_j = 1 | the row's observed entries)``."""
    x = np.asarray(x, np.float32)
    q = clt_ref.codes(x)
    _, p1 = two_passes(bfs, tree, params, q, dtype)
    return np.where(q == MISSING, p1, x.astype(dtype))


def _leaf(node, q, dtype):
    """``(V(leaf) float64 [n], p1 [n, d_l], holes [n, d_l])`` for the rows ``q`` (all columns)."""
    ql = q[:, node['scope']]
    value, p1 = two_passes(node['bfs'], node['tree'], node['params'], ql, dtype)
    holes = ql == MISSING
    full = ~holes.any(axis=1)
    if full.any():                                          # the gather path: a float64 sum rounded once
        value[full] = clt_ref.log_likelihood64(node['tree'], node['params'], ql[full]).astype(dtype)
    return value.astype(np.float64), p1, holes


def _value(model, k, q, dtype):
    """The first walk: V(node k) in float64."""
    node = model[k]
    if len(q) == 0:
        return np.zeros(0, np.float64)
    if node['or_id'] < 0:
        return _leaf(node, q, dtype)[0]
    c = q[:, node['or_id']]
    with np.errstate(divide='ignore'):
        logw = np.log(np.asarray(node['weights'], np.float64))
    side = []
    for v in (0, 1):
        go = (c == v) | (c == MISSING)
        full = np.full(len(q), -np.inf)
        full[go] = logw[v] + _value(model, node['children'][v], q[go], dtype)
        side.append(full)
    return np.where(c == MISSING, cnet_ref.lse64(side[0], side[1]), np.where(c == 1, side[1], side[0]))


def _spread(model, k, q, idx, prefix, log_pe, acc, dtype):
    """The second walk: adds to ``acc[idx]`` and returns S, the sum of pi_l over the consistent leaves below node k."""
    node = model[k]
    if len(idx) == 0:
        return np.zeros(0, np.float64)
    if node['or_id'] < 0:
        value, p1, holes = _leaf(node, q[idx], dtype)
        with np.errstate(invalid='ignore'):
            pi = np.exp((prefix + value) - log_pe[idx])
        use = (pi > 0) & holes.any(axis=1)
        for j, col in enumerate(node['scope']):
            at = use & holes[:, j]
            acc[idx[at], col] += pi[at] * p1[at, j].astype(np.float64)
        return pi
    col = node['or_id']
    c = q[idx, col]
    with np.errstate(divide='ignore'):
        logw = np.log(np.asarray(node['weights'], np.float64))
    side = []
    for v in (0, 1):
        go = (c == v) | (c == MISSING)
        full = np.zeros(len(idx), np.float64)
        full[go] = _spread(model, node['children'][v], q, idx[go], prefix[go] + logw[v], log_pe, acc, dtype)
        side.append(full)
    hole = c == MISSING
    acc[idx[hole], col] += side[1][hole]
    return np.where(hole, side[0] + side[1], np.where(c == 1, side[1], side[0]))


def cnet_marginals(model, x, dtype=np.float64):
    """``[B, D]`` float64: ``x`` with every NaN entry replaced by ``p(x_j = 1 | the row's observed entries)``; the leaves'
    passes in ``dtype``.  In float32 the result is rounded to float32 once, as the device rounds it."""
    x = np.asarray(x, np.float32)
    q = clt_ref.codes(x)
    b, d = q.shape
    log_pe = _value(model, 0, q, dtype)
    acc = np.zeros((b, d), np.float64)
    _spread(model, 0, q, np.arange(b), np.zeros(b, np.float64), log_pe, acc, dtype)
    acc[log_pe == -np.inf] = np.nan
    if dtype == np.float32:
        acc = acc.astype(np.float32).astype(np.float64)
    return np.where(q == MISSING, acc, x.astype(np.float64))


# ---- enumeration (small D) ---------------------------------------------------------------------------------------------------
def every_row(d):
    return ((np.arange(2 ** d)[:, None] >> np.arange(d)) & 1).astype(np.int64)


def by_enumeration(p_every, x):
    """``[B, D]`` float64 from ``p_every``, the probability of each of the 2^D complete rows of :func:`every_row`: the
    share of the mass that agrees with a row's observed entries and has a one in column j."""
    x = np.asarray(x, np.float32)
    d = x.shape[1]
    ones = every_row(d).astype(np.float64)
    number, bit = np.arange(2 ** d), 1 << np.arange(d)
    out = x.astype(np.float64)
    for r, row in enumerate(x):
        obs = ~np.isnan(row)
        agrees = (number & int(bit[obs].sum())) == int(bit[obs & (row == 1)].sum())
        p = np.where(agrees, p_every, 0.0)
        with np.errstate(invalid='ignore', divide='ignore'):
            out[r, ~obs] = ((p @ ones) / p.sum())[~obs]
    return out


def tree_by_enumeration(tree, params, x):
    d = np.asarray(x).shape[1]
    return by_enumeration(np.exp(clt_ref.log_likelihood64(tree, params, every_row(d))), x)


def cnet_by_enumeration(model, x):
    d = np.asarray(x).shape[1]
    return by_enumeration(np.exp(cnet_ref._path_values(model, every_row(d))), x)
