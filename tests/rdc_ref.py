"""A numpy float64 restatement of the RDC column split for discrete data as this project defines it
(include/deeprob_learn.h, "Maximal correlation"; DESIGN.md, "rdc column splits"): the score of two columns is the
largest singular value of their normalised, centred contingency table -- the largest canonical correlation of the two
indicator spaces, which is what reference splitting/rdc.py:85-134 estimates through random features and CCA.

Three things live here, none of which imports the package:
  * ``maxcorr_svd``: the score by ``np.linalg.svd``;
  * ``maxcorr_jacobi``: the score in the header's order of operations (one-sided Jacobi, plain Python floats);
  * ``learn_spn``: the task loop of tests/learnspn_ref.py with the rdc branch (rdc.py:16-48) for column splits.
"""
import math
from collections import deque

import numpy as np

from tests import learnspn_ref as ref

JACOBI_TOL = 2.0 ** -48         # rotate when |gamma| > JACOBI_TOL * sqrt(alpha * beta)
JACOBI_SWEEPS = 30              # the sweep cap


def joint_counts(xi, xj, ki, kj):
    """Exact joint counts; a value >= K is not counted (the header's rule)."""
    xi, xj = np.asarray(xi).astype(np.int64), np.asarray(xj).astype(np.int64)
    keep = (xi < ki) & (xj < kj)
    return np.bincount(xi[keep] * kj + xj[keep], minlength=ki * kj).reshape(ki, kj)


def present_table(joint):
    """(counts over present values, row sums, column sums, counted rows) as Python ints, or None when a side has fewer
    than two present values."""
    c = np.asarray(joint).astype(np.int64)
    r, s = c.sum(axis=1), c.sum(axis=0)
    pa, pb = np.flatnonzero(r > 0), np.flatnonzero(s > 0)
    if len(pa) < 2 or len(pb) < 2:
        return None
    return c[np.ix_(pa, pb)], r[pa], s[pb], int(c.sum())


def centred(c, r, s, n):
    """M[a][b] = (c[a][b] n - r[a] s[b]) / (n sqrt(r[a] s[b])): the numerator in exact integers."""
    num = (c * n - np.outer(r, s)).astype(np.float64)
    den = float(n) * np.sqrt(np.outer(r, s).astype(np.float64))
    return num / den


def maxcorr_svd(joint):
    t = present_table(joint)
    if t is None:
        return 0.0
    return float(min(1.0, max(0.0, np.linalg.svd(centred(*t), compute_uv=False)[0])))


def maxcorr_jacobi(joint):
    """The header's order: the 2 x 2 closed form, else cyclic one-sided Jacobi over the vectors of the shorter side."""
    t = present_table(joint)
    if t is None:
        return 0.0
    c, r, s, n = t
    if c.shape == (2, 2):
        num = abs(int(c[0, 0]) * int(c[1, 1]) - int(c[0, 1]) * int(c[1, 0]))
        den = math.sqrt(float(int(r[0]) * int(r[1])) * float(int(s[0]) * int(s[1])))
        return min(1.0, float(num) / den)
    m = centred(c, r, s, n)
    w = [[float(v) for v in row] for row in (m if m.shape[0] <= m.shape[1] else m.T)]    # the shorter side's vectors
    p, length = len(w), len(w[0])
    for _ in range(JACOBI_SWEEPS):
        rotated = False
        for i in range(p - 1):
            for j in range(i + 1, p):
                alpha = beta = gamma = 0.0
                for e in range(length):
                    alpha = alpha + w[i][e] * w[i][e]
                    beta = beta + w[j][e] * w[j][e]
                    gamma = gamma + w[i][e] * w[j][e]
                if not abs(gamma) > JACOBI_TOL * math.sqrt(alpha * beta):
                    continue
                rotated = True
                zeta = (beta - alpha) / (2.0 * gamma)
                tan = (1.0 if zeta >= 0.0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                cos = 1.0 / math.sqrt(1.0 + tan * tan)
                sin = cos * tan
                for e in range(length):
                    wi, wj = w[i][e], w[j][e]
                    w[i][e] = cos * wi - sin * wj
                    w[j][e] = sin * wi + cos * wj
        if not rotated:
            break
    best = 0.0
    for v in range(p):
        q = 0.0
        for e in range(length):
            q = q + w[v][e] * w[v][e]
        best = q if q > best else best
    return min(1.0, math.sqrt(best))


def rdc_scores(data, ks, rs, k=20, score=maxcorr_svd):
    """The [D, D] float64 score matrix; consumes ``rs`` as rdc.py:170-176 does (the draws cancel out of the value)."""
    data = np.asarray(data)
    nf = data.shape[1]
    for i in range(nf):
        rs.randn(ks[i], k)
        rs.randn(k)
    out = np.ones((nf, nf), np.float64)
    for a in range(nf):
        for b in range(a + 1, nf):
            out[a, b] = out[b, a] = score(joint_counts(data[:, a], data[:, b], ks[a], ks[b]))
    return out


def components(adjacent):
    """Labels of the connected components, numbered by each component's smallest member (what scipy's
    ``connected_components`` returns, rdc.py:47)."""
    nf = len(adjacent)
    labels, nxt = np.full(nf, -1, np.int64), 0
    for start in range(nf):
        if labels[start] >= 0:
            continue
        labels[start] = nxt
        queue = deque([start])
        while queue:
            f = queue.popleft()
            for o in np.flatnonzero(adjacent[f]):
                if labels[o] < 0:
                    labels[o] = nxt
                    queue.append(int(o))
        nxt += 1
    return labels


def rdc_cols(data, ks, rs, d=0.3, k=20, score=maxcorr_svd, stats=None):
    scores = rdc_scores(data, ks, rs, k, score)
    if stats is not None:
        off = scores[~np.eye(len(scores), dtype=bool)]
        stats['margin'] = min(stats.get('margin', np.inf), float(np.min(np.abs(off - d))))
        stats['calls'] = stats.get('calls', 0) + 1
    return components(scores > d)


def learn_spn(data, names, ks, split_rows='random', min_rows_slice=256, min_cols_slice=2, random_state=None, alpha=0.1,
              d=0.3, k=20, a=2.0, b=2.0, n=2, score=maxcorr_svd, stats=None, kmeans=ref.kmeans):
    """The task loop of tests/learnspn_ref.py:learn_spn with ``rdc_cols`` as the column split.  ``kmeans(rows, ks, rs, n,
    stats)`` gives the labels of a k-means row split: the restatement's own, or a test's."""
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    data = np.asarray(data).astype(np.int64)
    tmp = ref.node('Product', range(data.shape[1]))
    tasks = deque([dict(parent=tmp, data=data, scope=list(range(data.shape[1])), ncs=False, nrs=False, first=True)])
    while tasks:
        t = tasks.popleft()
        x, scope = t['data'], t['scope']
        ns, nf = x.shape
        zero = np.array([np.all(x[:, i] == x[0, i]) for i in range(nf)])
        lks = [ks[s] for s in scope]
        if zero.all():
            t['parent']['children'].append(ref.naive(names, ks, x, scope, alpha))
        elif zero.any():
            nd = ref.node('Product', scope)
            nd['children'].append(ref.naive(names, ks, x[:, zero], [scope[i] for i in np.flatnonzero(zero)], alpha))
            first = t['first'] and len(tasks) == 0
            tasks.append(dict(parent=nd, data=x[:, ~zero], scope=[scope[i] for i in np.flatnonzero(~zero)], ncs=False, nrs=False,
                              first=first))
            t['parent']['children'].append(nd)
        elif t['nrs'] or nf < min_cols_slice or ns < min_rows_slice:
            if nf == 1:
                t['parent']['children'].append(ref.mle_leaf(names[scope[0]], scope[0], x[:, 0], ks[scope[0]], alpha))
            else:
                t['parent']['children'].append(ref.naive(names, ks, x, scope, alpha))
        elif t['ncs'] or t['first']:
            if split_rows == 'random':
                q = rs.beta(a, b)
                clusters = rs.binomial(1, q, size=ns)
            else:
                clusters = kmeans(x, lks, rs, n, stats)
            present = np.unique(clusters)
            if len(present) == 1:
                tasks.append(dict(parent=t['parent'], data=x, scope=scope, ncs=False, nrs=True, first=False))
                continue
            nd = ref.node('Sum', scope, weights=[float(np.sum(clusters == c)) / ns for c in present])
            for c in present:
                tasks.append(dict(parent=nd, data=x[clusters == c], scope=scope, ncs=False, nrs=False, first=False))
            t['parent']['children'].append(nd)
        else:
            clusters = rdc_cols(x, lks, rs, d, k, score, stats)
            present = np.unique(clusters)
            if len(present) == 1:
                tasks.append(dict(parent=t['parent'], data=x, scope=scope, ncs=True, nrs=False, first=False))
                continue
            nd = ref.node('Product', scope)
            for c in present:
                tasks.append(dict(parent=nd, data=x[:, clusters == c], scope=[scope[i] for i in np.flatnonzero(clusters == c)],
                                  ncs=False, nrs=False, first=False))
            t['parent']['children'].append(nd)
    return tmp['children'][0]
