"""A numpy restatement of the mixture of Chow-Liu trees (include/deeprob_clt.h, last section): the
mixture log likelihood over the tree pass of tests/clt_ref.py, the responsibilities, the weighted statistics of
``dpc_mix_em_stats``, the two updates of batch EM (reference cltree.py:127-155, node.py:100-111) and its loop
(learning/em.py:84-107).  Everything is float64 unless a function says otherwise.  It shares no code with the package.
"""
import os

import numpy as np

from tests import clt_ref

GOLDEN = os.path.join(clt_ref.GOLDEN, 'clt_mixture_em.npz')
_cache = {}


def golden():
    """The fixture tests/golden/clt_mixture_em.npz as a dict (tools/gen_golden_clt_mixture.py); loaded once."""
    if 'g' not in _cache:
        f = np.load(GOLDEN)
        _cache['g'] = {k: f[k] for k in f.files}
    return _cache['g']


# ---- likelihood ----------------------------------------------------------------------------------------------------------
def component_lls(trees, params, x):
    """``[B, K]`` float32: tests/clt_ref.log_likelihood (the header's two paths) of every tree ``(bfs, tree)``."""
    return np.stack([clt_ref.log_likelihood(bfs, tree, p, x) for (bfs, tree), p in zip(trees, params)], axis=1)


def complete_lls(trees, params, x, dtype=np.float64):
    """``[B, K]``: the sum of ``params[i][x_parent(i)][x_i]`` over i in order for complete rows, accumulated in float64 from
    parameters of type ``dtype`` and rounded to ``dtype``."""
    x = np.asarray(x).astype(np.int64)
    out = np.zeros((len(x), len(trees)), np.float64)
    for k, ((_, tree), p) in enumerate(zip(trees, params)):
        p = np.asarray(p, dtype)
        for i in range(len(tree)):
            out[:, k] += p[i, x[:, tree[i]] if tree[i] >= 0 else 0, x[:, i]].astype(np.float64)
    return out.astype(dtype)


def mix(comp_ll, logw, dtype=np.float64):
    """``(ll [B], resp [B, K])`` in ``dtype``, in the order of the header: a_k = logw_k + comp_ll_k, M = max_k a_k,
    L = log(sum_k exp(a_k - M)) with k increasing from 0, ll = M + L, resp_k = exp((a_k - M) - L); ll = -inf and resp = 0 where
    M = -inf."""
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        a = (np.asarray(logw, dtype)[None, :] + np.asarray(comp_ll, dtype)).astype(dtype)
        top = a.max(axis=1)
        dead = top == -np.inf
        safe = np.where(dead, dtype(0), top).astype(dtype)
        s = np.zeros(len(a), dtype)
        for k in range(a.shape[1]):
            s = (s + np.exp((a[:, k] - safe).astype(dtype)).astype(dtype)).astype(dtype)
        log_s = np.log(s).astype(dtype)
        ll = np.where(dead, dtype(-np.inf), (safe + log_s).astype(dtype)).astype(dtype)
        resp = np.exp(((a - safe[:, None]).astype(dtype) - log_s[:, None]).astype(dtype)).astype(dtype)
        resp[dead] = 0
    return ll, resp


def ll_bound(comp_ll, logw):
    """The bound on ``|ll - exact|`` of the float32 mixing, per row: ``2^-23 (max_k |a_k| + K + 4)``.  One rounded add per
    a_k (|a_k| 2^-24 each, and M is one of them); the K terms expf(a_k - M) <= 1 carry the rounding of the subtraction
    (relative 2^-24 |a_k - M| <= 2^-23 max|a|, absorbed by the first term since d/dx log sum exp <= 1) and of expf, and
    their K - 1 additions round by at most 2^-24 K each relative to a sum >= 1; logf and the final add are a few ulp of
    numbers <= max|a| + log K."""
    with np.errstate(invalid='ignore'):
        a = np.asarray(logw, np.float64)[None, :] + np.asarray(comp_ll, np.float64)
    finite = np.where(np.isfinite(a), np.abs(a), 0.0)
    return 2.0 ** -23 * (finite.max(axis=1) + a.shape[1] + 4)


def resp_bound(comp_ll, logw):
    """The bound on ``|resp - exact|`` of the float32 mixing, per row: ``2^-25 max_k |a_k| + 2^-21``.  The exact value is the
    softmax of the unrounded a; the float32 a_j is off by at most 2^-24 |a_j|, and d resp_k / d a_j = resp_k ([k = j] -
    resp_j), so that these roundings move resp_k by at most resp_k 2 (1 - resp_k) 2^-24 max|a| <= 2^-25 max|a|.  What follows
    works on numbers <= 1: the differences with M and L, L's own error and expf are a few relative ulp, 2^-21 in all."""
    with np.errstate(invalid='ignore'):
        a = np.asarray(logw, np.float64)[None, :] + np.asarray(comp_ll, np.float64)
    finite = np.where(np.isfinite(a), np.abs(a), 0.0)
    return 2.0 ** -25 * finite.max(axis=1) + 2.0 ** -21


# ---- statistics ------------------------------------------------------------------------------------------------------------
def em_stats(x, resp, parents):
    """``[K, 1 + 2 D]`` float64: per component the sum of resp, of resp * x_j and of resp * x_j * x_parent(j) (0 at the
    root); x: complete 0 / 1 rows (anything that is not 1 counts as 0)."""
    x = (np.asarray(x) == 1).astype(np.float64)
    g = np.asarray(resp).astype(np.float64)
    k, d = g.shape[1], x.shape[1]
    out = np.zeros((k, 1 + 2 * d), np.float64)
    for c in range(k):
        pa = np.asarray(parents[c])
        xp = np.where(pa[None, :] >= 0, x[:, np.maximum(pa, 0)], 0.0)
        out[c, 0] = g[:, c].sum()
        out[c, 1:1 + d] = g[:, c] @ x
        out[c, 1 + d:] = g[:, c] @ (x * xp)
    return out


# ---- the two updates ---------------------------------------------------------------------------------------------------------
def tree_update(params, tree, root, stats, step_size, dtype=np.float64):
    """cltree.py:131-155 in ``dtype`` from the tree's row of statistics."""
    f = dtype
    params, tree = np.asarray(params, f), np.asarray(tree)
    d = len(tree)
    alpha = f(2.0 ** -10)                           # np.finfo(np.float16).eps
    total = f(stats[0])
    ones = np.asarray(stats[1:1 + d]).astype(f)
    both = np.asarray(stats[1 + d:]).astype(f)
    priors = np.empty((d, 2), f)
    priors[:, 1] = (ones + f(2) * alpha) / (total + f(4) * alpha)
    priors[:, 0] = f(1) - priors[:, 1]
    cond = np.stack([ones - both, both], axis=1).astype(f)           # [j][l]: x_j = 1 and x_parent = l
    new = np.empty((d, 2, 2), f)
    new[:, :, 1] = (cond + alpha) / (total * priors[tree] + f(4) * alpha)
    new[:, :, 0] = f(1) - new[:, :, 1]
    new[root, 0] = new[root, 1] = priors[root]
    new = (f(1.0 - step_size) * np.exp(params) + f(step_size) * new).astype(f)
    new /= new.sum(axis=2, keepdims=True)
    with np.errstate(divide='ignore'):
        return np.log(new).astype(f)


def weight_update(weights, stats, step_size, dtype=np.float64):
    """node.py:107-111 in ``dtype``: weights * sum_i exp(ll_ik - ll_i) is the sum of the responsibilities, stats[:, 0]."""
    f = dtype
    weights = np.asarray(weights, f)
    unnorm = np.asarray(stats)[:, 0].astype(f) + f(np.finfo(np.float32).eps)
    return (f(1.0 - step_size) * weights + f(step_size) * (unnorm / unnorm.sum())).astype(f)


# ---- the loop ------------------------------------------------------------------------------------------------------------------
def em_init(random_state, trees_roots, n_vars, dtype=np.float64):
    """The reference's random initialisation (node.py:97-98, cltree.py:121-125): ``(weights, params [K, D, 2, 2])``; the
    draws pass through float32 as they do there."""
    weights = random_state.dirichlet(np.ones(len(trees_roots))).astype(np.float32).astype(dtype)
    params = []
    for root in trees_roots:
        probs = random_state.rand(n_vars, 2)
        probs[root, 0] = probs[root, 1]
        p = np.empty((n_vars, 2, 2), np.float32)
        p[:, :, 1] = probs
        p[:, :, 0] = 1.0 - probs
        params.append(np.log(p.astype(dtype)))
    return weights, np.stack(params)


def em_run(trees, roots, params, weights, data, index, step_size, dtype=np.float64, init=None, update=None):
    """Batch EM over the batches ``index`` ``[num_iter, batch]``: ``(weights, params, mean batch ll per iteration)``.
    ``trees``: ``(bfs, tree)`` per component; ``init``: a RandomState for the random initialisation, or None; ``update``: the
    tree update ``(params, tree, root, stats row, step_size) -> params`` to run instead of :func:`tree_update` (the
    package's pure-numpy one).  In float32 the likelihoods and the mixing follow the device's order and the statistics are
    float64 sums of float32 responsibilities, as the header states them."""
    f = dtype
    if init is not None:
        weights, params = em_init(init, roots, data.shape[1], f)
    weights, params = np.asarray(weights, f), np.asarray(params, f).copy()
    means = []
    for rows in index:
        x = data[rows]
        with np.errstate(divide='ignore'):
            ll, resp = mix(complete_lls(trees, params, x, f), np.log(weights).astype(f), f)
        means.append(float(np.mean(ll.astype(np.float64))) if len(ll) else float('nan'))
        stats = em_stats(x, resp, [t for _, t in trees])
        weights = weight_update(weights, stats, step_size, f)
        for k, ((_, tree), root) in enumerate(zip(trees, roots)):
            params[k] = (update(params[k], tree, root, stats[k], step_size) if update is not None
                         else tree_update(params[k], tree, root, stats[k], step_size, f))
    return weights, params, np.asarray(means)


def mean_ll(trees, params, weights, x):
    """The mean float64 log likelihood of complete rows."""
    with np.errstate(divide='ignore'):
        return float(np.mean(mix(complete_lls(trees, params, x), np.log(np.asarray(weights, np.float64)))[0]))


def prob_err(got_w, got_p, want_w, want_p):
    """``(weights, CPTs)``: the largest absolute difference of a probability."""
    return (float(np.max(np.abs(np.asarray(got_w, np.float64) - np.asarray(want_w, np.float64)))),
            float(np.max(np.abs(np.exp(np.asarray(got_p, np.float64)) - np.exp(np.asarray(want_p, np.float64))))))
