"""A numpy float64 restatement of LearnSPN on all-Gaussian data (deeprob/spn/learning/learnspn_cont.py and the last section
of include/deeprob_learn.h), in the manner of tests/learnspn_ref.py: plain loops over the reference's FIFO task queue,
one task at a time, on data slices.  The HIP path batches a generation of tasks; this file does not, and the two must
give the same graph.

Restated here, operation by operation where the header fixes an order: the two-pass moments (256 interleaved partial sums
added in order), the "max" ranks, the random features ``sin(rank / n * w + b)``, their sums and raw Gram matrix (numpy's
own summation order: the tests bound the difference), the ridge-regularised score, the float k-means and the task loop.
The data is taken as float32 values, as the device holds it.
"""
from collections import deque

import numpy as np

from tests.learnspn_ref import inertia_sum as sum256, node, RESTARTS, MAX_ITER

ZERO_VARIANCE, MIN_STDDEV, RIDGE, ZERO_TRACE = 1e-8, 1e-5, 1e-8, 1e-12


def as_device(data):
    """The float32 values of the data, as float64."""
    return np.asarray(data).astype(np.float32).astype(np.float64)


def moments(col):
    """(mean, population variance) of a float64 column in the header's order."""
    n = float(len(col))
    mean = sum256(col) / n
    d = col - mean
    return mean, sum256(d * d) / n


def ranks(col):
    """scipy.stats.rankdata(col, method='max') as integers: the number of entries <= each entry."""
    return np.searchsorted(np.sort(col), col, side='right').astype(np.int64)


def draw_features(rs, m, k, s):
    """rdc.py:170-176 for m continuous columns: (w, b), [m, k] float32 each, drawn column by column."""
    w, b = np.empty((m, k), np.float32), np.empty((m, k), np.float32)
    for p in range(m):
        w[p] = (np.sqrt(s) * rs.randn(1, k)).astype(np.float32)[0]
        b[p] = (np.sqrt(s) * rs.randn(k)).astype(np.float32)
    return w, b


def features(rk, w, b):
    """phi [n, m * k] float64 from the ranks rk [n, m] and the float32 draws."""
    n, m = rk.shape
    u = rk.astype(np.float64) / float(n)
    return np.concatenate([np.sin(u[:, p:p + 1] * w[p].astype(np.float64)[None, :] + b[p].astype(np.float64)[None, :])
                           for p in range(m)], axis=1)


def gram(phi):
    """(S, G): the column sums and the raw Gram matrix."""
    return phi.sum(axis=0), phi.T @ phi


def scores_from_gram(G, S, n, m, k):
    C = G / float(n) - np.outer(S, S) / (float(n) * float(n))
    blocks = [slice(p * k, (p + 1) * k) for p in range(m)]
    W = []
    for bp in blocks:
        trace = float(np.trace(C[bp, bp]))
        if not trace > ZERO_TRACE * k:
            W.append(None)
            continue
        lam = RIDGE * trace / k
        ev, V = np.linalg.eigh(C[bp, bp])
        W.append(V @ np.diag(1.0 / np.sqrt(np.maximum(ev, 0.0) + lam)) @ V.T)
    out = np.ones((m, m))
    for p in range(m):
        for q in range(p + 1, m):
            v = 0.0 if W[p] is None or W[q] is None else \
                min(1.0, float(np.linalg.svd(W[p] @ C[blocks[p], blocks[q]] @ W[q], compute_uv=False)[0]))
            out[p, q] = out[q, p] = v
    return out


def rdc_scores(data, rs, k=20, s=1.0 / 6.0):
    """The [D, D] score matrix of float64 data columns, with the draws of ``rs``."""
    w, b = draw_features(rs, data.shape[1], k, s)
    return rdc_scores_with(data, w, b)


def rdc_scores_with(data, w, b):
    """The same from given draws ``w``, ``b`` ([D, k] float32)."""
    (n, m), k = data.shape, w.shape[1]
    if m < 2:
        return np.ones((m, m))
    rk = np.stack([ranks(data[:, p]) for p in range(m)], axis=1)
    S, G = gram(features(rk, w, b))
    return scores_from_gram(G, S, n, m, k)


def components(adjacent):
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


def rdc_cols(data, rs, d=0.3, k=20, s=1.0 / 6.0, stats=None):
    sc = rdc_scores(data, rs, k, s)
    if stats is not None and len(sc) > 1:
        off = sc[np.triu_indices(len(sc), 1)]
        stats['margin'] = min(stats.get('margin', np.inf), float(np.min(np.abs(off - d))))
    return components(sc > d)


# ---- k-means on float columns ------------------------------------------------------------------------------------------
def sq_dist(data, cen):
    """[n] squared distances of the rows to ONE centroid ([ncols]), accumulated column by column."""
    d = np.zeros(len(data))
    for p in range(data.shape[1]):
        u = data[:, p] - cen[p]
        d = d + u * u
    return d


def kmeans_restart(data, seed, n_clusters):
    """One restart: (labels, centroids [C, ncols], inertia, sizes, smallest relative gap between a row's two nearest
    centroids over all its assignment steps)."""
    cen = np.stack([data[seed[c]].copy() for c in range(n_clusters)])
    labels, gap = None, np.inf
    for it in range(MAX_ITER):
        dist = np.stack([sq_dist(data, cen[c]) for c in range(n_clusters)], axis=1)
        new = np.argmin(dist, axis=1)                    # (the first minimum: ties to the lower index)
        if n_clusters > 1:
            two = np.sort(dist, axis=1)[:, :2]
            gap = min(gap, float(np.min((two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300))))
        same = labels is not None and np.array_equal(new, labels)
        labels = new
        if same or it == MAX_ITER - 1:
            break
        for c in range(n_clusters):
            size = int(np.sum(labels == c))
            if size == 0:
                continue
            for p in range(data.shape[1]):
                cen[c, p] = sum256(np.where(labels == c, data[:, p], 0.0)) / float(size)
    own = np.zeros(len(data))
    for c in range(n_clusters):
        own[labels == c] = sq_dist(data[labels == c], cen[c])
    return labels, cen, sum256(own), np.bincount(labels, minlength=n_clusters), gap


def kmeans(data, rs, n_clusters=2, stats=None):
    seeds = [rs.choice(len(data), n_clusters, replace=False) for _ in range(RESTARTS)]
    best = None
    for seed in seeds:
        run = kmeans_restart(data, seed, n_clusters)
        if stats is not None:
            stats['gap'] = min(stats.get('gap', np.inf), run[4])          # (every restart runs on the device)
        if best is None or run[2] < best[2]:
            best = run
    return best[0]


# ---- the task loop -------------------------------------------------------------------------------------------------------
def leaf(var, col):
    mean, var_ = moments(col)
    return node('Gaussian', [var], params={'mean': mean, 'stddev': max(float(np.sqrt(var_)), MIN_STDDEV)})


def naive(data, scope):
    out = node('Product', scope)
    for i, s in enumerate(scope):
        out['children'].append(leaf(s, data[:, i]))
    return out


def learn_spn(data, split_rows='kmeans', split_cols='rdc', min_rows_slice=256, min_cols_slice=2, random_state=None, d=0.3, k=20,
              s=1.0 / 6.0, a=2.0, b=2.0, n=2, stats=None):
    """The task loop on all-Gaussian data; returns the root (dict form).  ``stats``: 'margin' (the smallest distance of a
    score to ``d``) and 'gap' (the smallest relative k-means distance gap)."""
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    data = as_device(data)
    tmp = node('Product', range(data.shape[1]))
    tasks = deque([dict(parent=tmp, data=data, scope=list(range(data.shape[1])), ncs=False, nrs=False, first=True)])
    while tasks:
        t = tasks.popleft()
        x, scope = t['data'], t['scope']
        ns, nf = x.shape
        zero = np.array([moments(x[:, i])[1] <= ZERO_VARIANCE for i in range(nf)])
        if zero.all():
            t['parent']['children'].append(naive(x, scope))
        elif zero.any():
            nd = node('Product', scope)
            nd['children'].append(naive(x[:, zero], [scope[i] for i in np.flatnonzero(zero)]))
            tasks.append(dict(parent=nd, data=x[:, ~zero], scope=[scope[i] for i in np.flatnonzero(~zero)], ncs=False, nrs=False,
                              first=t['first'] and len(tasks) == 0))
            t['parent']['children'].append(nd)
        elif t['nrs'] or nf < min_cols_slice or ns < min_rows_slice:
            t['parent']['children'].append(leaf(scope[0], x[:, 0]) if nf == 1 else naive(x, scope))
        elif t['ncs'] or t['first']:
            if split_rows == 'random':
                q = rs.beta(a, b)
                clusters = rs.binomial(1, q, size=ns)
            else:
                clusters = kmeans(x, rs, n, stats)
            present = np.unique(clusters)
            if len(present) == 1:
                tasks.append(dict(parent=t['parent'], data=x, scope=scope, ncs=False, nrs=True, first=False))
                continue
            nd = node('Sum', scope, weights=[float(np.sum(clusters == c)) / ns for c in present])
            for c in present:
                tasks.append(dict(parent=nd, data=x[clusters == c], scope=scope, ncs=False, nrs=False, first=False))
            t['parent']['children'].append(nd)
        else:
            if split_cols == 'random':
                q = rs.beta(a, b)
                clusters = rs.binomial(1, q, size=nf)
            else:
                clusters = rdc_cols(x, rs, d, k, s, stats)
            present = np.unique(clusters)
            if len(present) == 1:
                tasks.append(dict(parent=t['parent'], data=x, scope=scope, ncs=True, nrs=False, first=False))
                continue
            nd = node('Product', scope)
            for c in present:
                tasks.append(dict(parent=nd, data=x[:, clusters == c], scope=[scope[i] for i in np.flatnonzero(clusters == c)],
                                  ncs=False, nrs=False, first=False))
            t['parent']['children'].append(nd)
    return tmp['children'][0]


def two_blocks(n=300, seed=0):
    """n rows of 6 columns: two well-separated clusters; columns 0-2 and 3-5 are two blocks, strongly dependent within
    (one latent each, with small noise) and independent across."""
    rs = np.random.RandomState(seed)
    z = rs.randint(0, 2, size=n)
    la, lb = rs.randn(n), rs.randn(n)
    x = np.stack([la, 2.0 * la + 0.05 * rs.randn(n), -la + 0.05 * rs.randn(n),
                  lb, lb + 0.05 * rs.randn(n), 0.5 * lb + 0.05 * rs.randn(n)], axis=1)
    return (x + 12.0 * z[:, None]).astype(np.float32)


#: the end-to-end case of tests/test_learn_cont_gpu.py; the seed was chosen on the CPU with this file alone so that every
#: score decision lies at least 1e-3 from d and no k-means distance ties (tests/test_learn_cont_host.py asserts both)
E2E = dict(split_rows='kmeans', split_cols='rdc', min_rows_slice=64, random_state=5)
_e2e = {}


def e2e_restated():
    """(root of the restated loop on ``two_blocks()``, its stats), computed once."""
    if not _e2e:
        stats = {}
        _e2e['root'] = learn_spn(two_blocks(), stats=stats, **E2E)
        _e2e['stats'] = stats
    return _e2e['root'], _e2e['stats']
