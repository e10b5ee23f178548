"""A numpy restatement of the two queries of a cutset network that fill a row in (include/deeprob_clt.h, ``dpc_cnq_mpe`` and
``dpc_cnq_sample``): exact conditional sampling replayed draw by draw with the counter-based generator, and
exact MPE.  It shares no code with the package; models are those of tests/cnet_ref.py (a list of nodes in breadth-first
order), leaves and their passes come from tests/clt_ref.py.

One bottom-up walk: every node returns (value, leaf).  A leaf returns (V(leaf), itself); an OR node whose variable is
observed passes its child's pair on, the log weight added; an OR node k whose variable is NaN takes both pairs,
``a_c = logw[c] + V_c`` in float64, and returns ``(lse64(a_0, a_1), leaf_1 if u < exp(a_1 - lse64) else leaf_0)`` when sampling,
``(a_1, leaf_1) if a_1 > a_0 else (a_0, leaf_0)`` for MPE.  Then the NaN cut variables on the path of the returned leaf take
the side the path went, and the leaf's NaN columns are filled in ``bfs`` order after its upward pass from
``a_k = params[j][x_parent][k] + m_j[k]`` in float32: 1 iff ``u < exp(a_1 - lse(a_0, a_1))``, or iff ``a_1 > a_0``.
Counters: ``(row0 + r) * (M + d) + k`` for OR node k, ``(row0 + r) * (M + d) + M + c`` for column c.
"""
import numpy as np

from tests import clt_ref
from tests import cnet_ref
from tests.clt_ref import MISSING, uniform01

NEAR = 1e-5             # a draw this close to its probability may fall either way on the device (tests/clt_ref.py)
#: the evidence patterns of the 5-variable fixture whose posteriors the tests enumerate, and the draws taken of each
PATTERNS_D5 = ([np.nan] * 5, [1, np.nan, np.nan, 0, np.nan], [np.nan, np.nan, 1, np.nan, np.nan])
N_DRAWS = 20000


def leaf_value(node, x, reduce):
    """float32 ``[B]``: V(leaf) -- the gather path for a row without NaN in the leaf's scope, else the upward pass with
    R = lse (``'mar'``) or max (``'mpe'``), ended at the root as the log likelihood ends it."""
    if reduce == 'mar':
        return clt_ref.log_likelihood(node['bfs'], node['tree'], node['params'], x)
    params = np.asarray(node['params'], np.float32)
    bfs, tree = node['bfs'], node['tree']
    q = clt_ref.codes(x)
    out = np.empty(len(q), np.float32)
    full = ~(q == MISSING).any(axis=1)
    out[full] = clt_ref.log_likelihood64(tree, params, q[full]).astype(np.float32)
    if (~full).any():
        qm = q[~full]
        t, kids = clt_ref.upward(bfs, tree, params, qm, 'mpe')
        root = int(bfs[0])
        m, c, rows = clt_ref._message(t, kids, root, len(qm)), qm[:, root], np.arange(len(qm))
        k = np.where(c != MISSING, c, 0)
        out[~full] = np.where(c != MISSING, params[root, 0][k] + m[k, rows],
                              np.maximum(params[root, 0, 0] + m[0], params[root, 0, 1] + m[1]))
    return out


def _walk(model, k, q, x, rows, seed, stride, near):
    """``(value float64 [n], leaf int64 [n])`` of node k for the rows ``q`` / ``x`` with absolute numbers ``rows``; ``seed``
    None = MPE.  ``near`` (indexed like ``q``) collects the draws within NEAR of their probability."""
    node = model[k]
    n = len(q)
    if n == 0:
        return np.zeros(0, np.float64), np.zeros(0, np.int64)
    if node['or_id'] < 0:
        value = leaf_value(node, x[:, node['scope']], 'mpe' if seed is None else 'mar')
        return value.astype(np.float64), np.full(n, k, np.int64)
    c = q[:, node['or_id']]
    with np.errstate(divide='ignore'):
        logw = np.log(np.asarray(node['weights'], np.float64))
    a, leaf = [], []
    for v in (0, 1):
        go = (c == v) | (c == MISSING)
        sub_near = np.zeros(int(go.sum()), bool)
        value, chosen = _walk(model, node['children'][v], q[go], x[go], rows[go], seed, stride, sub_near)
        near[go] |= sub_near
        full_a, full_leaf = np.full(n, -np.inf), np.full(n, -1, np.int64)
        full_a[go], full_leaf[go] = logw[v] + value, chosen
        a.append(full_a)
        leaf.append(full_leaf)
    missing = c == MISSING
    if seed is None:
        right = a[1] > a[0]
        both = np.where(right, a[1], a[0])
    else:
        both = cnet_ref.lse64(a[0], a[1])
        with np.errstate(invalid='ignore'):
            p1 = np.where(both == -np.inf, 0.0, np.exp(a[1] - both))
        u = uniform01(seed, rows.astype(np.uint64) * np.uint64(stride) + np.uint64(k)).astype(np.float64)
        right = u < p1
        near |= missing & (np.abs(u - p1) < NEAR)
    right = np.where(missing, right, c == 1)
    value = np.where(missing, both, np.where(c == 1, a[1], a[0]))
    return value, np.where(right, leaf[1], leaf[0])


def _fill(model, x, seed, row0=0):
    x = np.asarray(x, np.float32)
    q = clt_ref.codes(x)
    b, d = q.shape
    m = len(model)
    stride = m + d
    rows = np.arange(b, dtype=np.int64) + row0
    near = np.zeros(b, bool)
    _, leaf = _walk(model, 0, q, x, rows, seed, stride, near)
    filled = x.copy()
    parent = {c: (k, v) for k, node in enumerate(model) if node['or_id'] >= 0 for v, c in enumerate(node['children'])}
    for k in np.unique(leaf):
        at = np.flatnonzero(leaf == k)
        up = int(k)
        while up in parent:                     # the NaN cut variables of the path take the side it went
            up, side = parent[up]
            col = model[up]['or_id']
            hole = at[q[at, col] == MISSING]
            filled[hole, col] = side
        node = model[int(k)]
        scope = np.asarray(node['scope'], np.int64)
        params = np.asarray(node['params'], np.float32)
        bfs, tree = node['bfs'], node['tree']
        ql = q[at][:, scope]
        t, kids = clt_ref.upward(bfs, tree, params, ql, 'mpe' if seed is None else 'mar')
        n = len(at)
        value = np.zeros((len(scope), n), np.int64)
        for j in bfs:
            pa = tree[j]
            xp = value[pa] if pa >= 0 else np.zeros(n, np.int64)
            msg = clt_ref._message(t, kids, j, n)
            a0, a1 = params[j, xp, 0] + msg[0], params[j, xp, 1] + msg[1]
            hole = ql[:, j] == MISSING
            if seed is None:
                pick = (a1 > a0).astype(np.int64)
            else:
                with np.errstate(invalid='ignore'):
                    p1 = np.exp(a1 - clt_ref.lse(a0, a1)).astype(np.float32)
                u = uniform01(seed, rows[at].astype(np.uint64) * np.uint64(stride) + np.uint64(m + int(scope[j])))
                pick = (u < p1).astype(np.int64)
                near[at] |= hole & (np.abs(u.astype(np.float64) - p1.astype(np.float64)) < NEAR)
            value[j] = np.where(hole, pick, ql[:, j])
            filled[at[hole], scope[j]] = value[j][hole]
    return filled, leaf, near


def sample_replay(model, x, seed, row0=0):
    """``(filled rows [B, D] float32, the drawn leaf's position in ``model`` [B], near [B])``: ``near[r]`` is true when any
    draw of row r lies within NEAR of its probability -- such a row may differ on the device."""
    return _fill(model, x, int(seed), row0)


def mpe(model, x):
    """``(filled rows [B, D] float32, the winning leaf's position in ``model`` [B])``."""
    filled, leaf, _ = _fill(model, x, None)
    return filled, leaf


# ---- enumeration (small D) ---------------------------------------------------------------------------------------------------
def every_row(d):
    return np.array([[(v >> i) & 1 for i in range(d)] for v in range(2 ** d)], np.int64)


def posterior(model, row):
    """``(every complete row [2^D, D], its posterior probability given the observed entries of ``row``)`` by enumeration."""
    row = np.asarray(row, np.float32)
    every = every_row(len(row))
    p = np.exp(cnet_ref._path_values(model, every))
    obs = ~np.isnan(row)
    p = np.where((every[:, obs] == row[obs]).all(axis=1), p, 0.0)
    return every, p / p.sum()


def deviations(model, row, samples, groups=None):
    """The worst |frequency - probability| in binomial standard errors over the completions of ``row`` (or over the groups
    ``groups[i]`` of complete row i, given ``samples`` as group labels), and the mass drawn outside the support."""
    every, p = posterior(model, row)
    n = len(samples)
    if groups is None:
        index = (np.asarray(samples).astype(np.int64) << np.arange(every.shape[1])).sum(axis=1)
        counts = np.bincount(index, minlength=len(every)).astype(np.float64)
    else:
        labels = np.unique(groups)
        p = np.array([p[groups == g].sum() for g in labels])
        counts = np.array([(np.asarray(samples) == g).sum() for g in labels], np.float64)
        assert counts.sum() == n
    support = p > 0
    se = np.sqrt(p[support] * (1.0 - p[support]) / n)
    worst = float(np.max(np.abs(counts[support] / n - p[support]) / np.maximum(se, 1e-300)))
    return worst, float(counts[~support].sum() / n)
