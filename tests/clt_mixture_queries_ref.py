"""A numpy restatement of the posterior queries of a mixture of Chow-Liu trees (include/deeprob_clt.h, the ``dpc_mixq_*``
section): the mixture level in float64, the posterior marginals, the replay of the sampler draw by draw,
the max-product MPE -- and the same three by enumeration of all ``2^D`` rows.  It shares no code with the package.  A model
is ``(trees, logw)``: ``trees`` a list of ``(bfs, tree, params)`` of tests/clt_ref.py, ``logw`` ``[K]`` float32.

``dtype`` is the arithmetic of a tree's passes: float32 is what the device runs, float64 is what it is held against.  The
mixture level -- a_k, M, S, T, pi_k, the accumulators -- is float64 in both, as it is on the device.

It also builds the models and batches the host and the device tests share (:func:`random_model`, :func:`batch`), so that
what the host test says about the rows set aside (``near``) is said of the rows the device test draws.
"""
import numpy as np

from tests import clt_ref
from tests import marginals_ref as mref
from tests.clt_ref import MISSING, uniform01
from tests.cnet_queries_ref import NEAR

DS, KS = (1, 2, 10, 33, 130), (1, 2, 3, 64)
BATCHES = (1, 64, 65, 200)
_cache = {}


# ---- models and rows -------------------------------------------------------------------------------------------------------
def random_tree(rs, d, lo=0.05):
    """``(bfs, tree, params)``: a uniformly grown random tree with CPT entries in ``[lo, 1 - lo]``."""
    order = rs.permutation(d)
    tree = np.full(d, -1, np.int32)
    for i in range(1, d):
        tree[order[i]] = order[rs.randint(i)]
    p1 = rs.uniform(lo, 1.0 - lo, (d, 2))
    p1[order[0], 1] = p1[order[0], 0]
    params = np.log(np.stack([1.0 - p1, p1], axis=2)).astype(np.float32)
    return clt_ref.bfs_order(tree), tree, params


def random_model(d, k, seed=0):
    """``(trees, logw)`` of ``k`` seeded random trees over ``d`` variables with Dirichlet weights; built once."""
    key = ('model', d, k, seed)
    if key not in _cache:
        rs = np.random.RandomState(1000 * d + 10 * k + seed)
        trees = [random_tree(rs, d) for _ in range(k)]
        w = rs.dirichlet(2.0 * np.ones(k)).astype(np.float32)
        _cache[key] = (trees, np.log(w))
        _cache[('weights',) + key[1:]] = w
    return _cache[key]


def random_weights(d, k, seed=0):
    """The float32 weights of :func:`random_model`: its ``logw`` is their float32 logarithm."""
    random_model(d, k, seed)
    return _cache['weights', d, k, seed]


def zero_weight_model():
    """d = 10, K = 3 with the weight of component 1 zero (``logw`` = -inf)."""
    trees, logw = random_model(10, 3, seed=1)
    logw = logw.copy()
    logw[1] = -np.inf
    return trees, logw


def impossible_model():
    """d = 5, K = 2, every tree with x1 = x0 for certain (-inf CPT entries): a row with x0 != x1 is impossible under both;
    the second tree also rules out x0 = 1."""
    key = 'impossible'
    if key not in _cache:
        rs = np.random.RandomState(77)
        trees = []
        for c in range(2):
            tree = np.array([-1, 0, 1, 1, 0], np.int32)
            p1 = rs.uniform(0.1, 0.9, (5, 2))
            p1[0, 1] = p1[0, 0] = 0.0 if c == 1 else p1[0, 0]
            p1[1] = [0.0, 1.0]
            with np.errstate(divide='ignore'):
                params = np.log(np.stack([1.0 - p1, p1], axis=2)).astype(np.float32)
            trees.append((clt_ref.bfs_order(tree), tree, params))
        _cache[key] = (trees, np.log(np.array([0.4, 0.6], np.float32)))
    return _cache[key]


def impossible_rows():
    nan = np.nan
    return np.array([[0, 1, nan, nan, 1], [1, 0, nan, 1, nan], [nan, nan, nan, nan, nan], [1, nan, nan, 0, nan],
                     [0, nan, 1, nan, nan], [1, 0, 1, 1, 0], [1, 1, 0, 1, 0]], np.float32)


def batch(d, n=200, seed=0, frac=0.3):
    """``[n, d]`` float32 0 / 1 rows with ``frac`` NaN; row 0 is all NaN, row 1 complete, and of the others every 16th is
    complete and every 16th all NaN, so that every prefix in BATCHES holds the three patterns."""
    rs = np.random.RandomState(5000 + 7 * d + seed)
    x = (rs.rand(n, d) < 0.5).astype(np.float32)
    holes = rs.rand(n, d) < frac
    holes[0] = True
    holes[1::16] = False
    holes[8::16] = True
    x[holes] = np.nan
    return x


# ---- a tree's passes in `dtype` ------------------------------------------------------------------------------------------------
def _pull(t, kids, j, b, dtype):
    m = np.zeros((2, b), dtype)
    for c in kids[j]:
        m = m + t[c]
    return m


def upward(bfs, tree, params, q, reduce, dtype):
    """``(t [d, 2, B], V [B], kids)``: the messages of every node but the root in the header's order with R = lse
    (``'mar'``) or max (``'mpe'``), and the value at the root."""
    params = np.asarray(params, np.float32).astype(dtype)
    kids = clt_ref.children_lists(bfs, tree)
    b, d = q.shape
    rows = np.arange(b)
    t = np.zeros((d, 2, b), dtype)

    def node(j):
        m, c = _pull(t, kids, j, b, dtype), q[:, j]
        obs, k = c != MISSING, np.where(c != MISSING, c, 0)
        out = []
        for l in range(2):
            a0, a1 = params[j, l, 0] + m[0], params[j, l, 1] + m[1]
            out.append(np.where(obs, params[j, l][k] + m[k, rows], np.maximum(a0, a1) if reduce == 'mpe' else mref.lse(a0, a1)))
        return out

    for j in list(bfs)[:0:-1]:
        t[j, 0], t[j, 1] = node(j)
    return t, node(int(bfs[0]))[0].astype(dtype), kids


def values(trees, q, reduce, dtype):
    """``[B, K]`` in ``dtype``: V_k -- the float64 gather rounded once for a row without NaN, else the upward pass."""
    full = ~(q == MISSING).any(axis=1)
    out = np.empty((len(q), len(trees)), dtype)
    for k, (bfs, tree, params) in enumerate(trees):
        out[full, k] = clt_ref.log_likelihood64(tree, params, q[full]).astype(dtype)
        if (~full).any():
            out[~full, k] = upward(bfs, tree, params, q[~full], reduce, dtype)[1]
    return out


def fill(bfs, tree, params, q, reduce, dtype, seed=None, rows=None):
    """``(value [B, d] int64, near [B])``: the NaN positions filled in ``bfs`` order after the upward pass, by the rule of
    dpc_clt_mpe (``'mpe'``) or by the normalised conditional against the draws u(1 + j) of the absolute rows ``rows``."""
    p = np.asarray(params, np.float32).astype(dtype)
    t, _, kids = upward(bfs, tree, params, q, reduce, dtype)
    b, d = q.shape
    value = np.zeros((d, b), np.int64)
    near = np.zeros(b, bool)
    for j in bfs:
        pa = tree[j]
        xp = value[pa] if pa >= 0 else np.zeros(b, np.int64)
        m = _pull(t, kids, j, b, dtype)
        a0, a1 = p[j, xp, 0] + m[0], p[j, xp, 1] + m[1]
        hole = q[:, j] == MISSING
        if reduce == 'mpe':
            pick = (a1 > a0).astype(np.int64)
        else:
            with np.errstate(invalid='ignore'):
                p1 = np.exp(a1 - mref.lse(a0, a1)).astype(dtype)
                u = uniform01(seed, rows.astype(np.uint64) * np.uint64(1 + d) + np.uint64(1 + int(j)))
                pick = (u < p1).astype(np.int64)
                near |= hole & (np.abs(u.astype(np.float64) - p1.astype(np.float64)) < NEAR)
        value[j] = np.where(hole, pick, q[:, j])
    return value.T, near


# ---- the mixture level ---------------------------------------------------------------------------------------------------------
def level(v, logw):
    """``(a [B, K], M [B], pi [B, K])`` in float64 from the trees' values ``v``: a_k = logw_k + V_k, M = max_k a_k,
    S = sum_k exp(a_k - M) with k increasing from 0.0, T = M + log(S), pi_k = exp(a_k - T); pi = 0 where M = -inf."""
    with np.errstate(invalid='ignore', divide='ignore'):
        a = np.asarray(logw, np.float32).astype(np.float64)[None, :] + np.asarray(v).astype(np.float64)
        top = a.max(axis=1)
        dead = ~(top > -np.inf)
        safe = np.where(dead, 0.0, top)
        s = np.zeros(len(a), np.float64)
        for k in range(a.shape[1]):
            s = s + np.exp(a[:, k] - safe)
        total = safe + np.log(s)
        pi = np.exp(a - total[:, None])
    pi[dead] = 0.0
    return a, np.where(dead, -np.inf, top), pi


def posterior(model, x, dtype=np.float64):
    """``[B, K]`` float64: pi_k, the posterior probability of every component given the observed entries."""
    trees, logw = model
    return level(values(trees, clt_ref.codes(x), 'mar', dtype), logw)[2]


# ---- the three queries ---------------------------------------------------------------------------------------------------------
def marginals(model, x, dtype=np.float64):
    """``[B, D]`` float64: ``x`` with every NaN entry replaced by ``sum_k pi_k p_k(x_j = 1 | e)``, k increasing over
    pi_k > 0; NaN where M = -inf.  In float32 the result is rounded to float32 once, as the device rounds it."""
    trees, logw = model
    x = np.asarray(x, np.float32)
    q = clt_ref.codes(x)
    out = x.astype(np.float64)
    idx = np.flatnonzero((q == MISSING).any(axis=1))
    if len(idx) == 0:
        return out
    qn = q[idx]
    passes = [mref.two_passes(bfs, tree, params, qn, dtype) for bfs, tree, params in trees]
    _, top, pi = level(np.stack([v for v, _ in passes], axis=1), logw)
    acc = np.zeros(qn.shape, np.float64)
    for k, (_, p1) in enumerate(passes):
        use = pi[:, k] > 0
        acc[use] += pi[use, k][:, None] * p1[use].astype(np.float64)
    acc[top == -np.inf] = np.nan
    if dtype == np.float32:
        acc = acc.astype(np.float32).astype(np.float64)
    out[idx] = np.where(qn == MISSING, acc, out[idx])
    return out


def sample_replay(model, x, seed, row0=0):
    """``(filled rows [B, D] float32, component [B], near [B])``, draw by draw in the device's float32: ``near[r]`` is true
    when any draw of row r lies within NEAR of its probability (u(0) of a boundary c_k) -- such a row may differ on the
    device.  A row with M = -inf keeps its NaN and has component -1."""
    trees, logw = model
    x = np.asarray(x, np.float32)
    q = clt_ref.codes(x)
    b, d = q.shape
    rows = np.arange(b, dtype=np.int64) + row0
    _, top, pi = level(values(trees, q, 'mar', np.float32), logw)
    u0 = uniform01(int(seed), rows.astype(np.uint64) * np.uint64(1 + d)).astype(np.float64)
    c = np.zeros(b, np.float64)
    comp, last = np.full(b, -1, np.int64), np.full(b, -1, np.int64)
    near = np.zeros(b, bool)
    for k in range(len(trees)):
        c = c + pi[:, k]
        last = np.where(pi[:, k] > 0, k, last)
        comp = np.where((comp < 0) & (u0 < c), k, comp)
        near |= np.abs(u0 - c) < NEAR
    comp = np.where(comp < 0, last, comp)
    dead = top == -np.inf
    comp[dead], near[dead] = -1, False
    filled = x.copy()
    holes = q == MISSING
    for k, (bfs, tree, params) in enumerate(trees):
        at = np.flatnonzero((comp == k) & holes.any(axis=1))
        if len(at):
            value, close = fill(bfs, tree, params, q[at], 'mar', np.float32, int(seed), rows[at])
            filled[at] = np.where(holes[at], value, filled[at])
            near[at] |= close
    return filled, comp, near


def mpe(model, x, dtype=np.float32):
    """``(filled rows [B, D] float32, component [B])``: the smallest k attaining max_k a_k with R = max, and that tree's
    completion by the rule of dpc_clt_mpe.  A row with M = -inf keeps its NaN and has component -1."""
    trees, logw = model
    x = np.asarray(x, np.float32)
    q = clt_ref.codes(x)
    a, top, _ = level(values(trees, q, 'mpe', dtype), logw)
    comp = np.where(top == -np.inf, -1, np.argmax(np.where(np.isnan(a), -np.inf, a), axis=1))
    filled = x.copy()
    holes = q == MISSING
    for k, (bfs, tree, params) in enumerate(trees):
        at = np.flatnonzero((comp == k) & holes.any(axis=1))
        if len(at):
            value, _ = fill(bfs, tree, params, q[at], 'mpe', dtype)
            filled[at] = np.where(holes[at], value, filled[at])
    return filled, comp


def log_joint(model, comp, rows):
    """``[B]`` float64: ``log(w_k p_k(row))`` of the complete rows ``rows`` under their components ``comp``."""
    trees, logw = model
    rows = np.asarray(rows, np.float32).astype(np.int64)
    out = np.empty(len(rows), np.float64)
    for r, (k, row) in enumerate(zip(comp, rows)):
        out[r] = float(logw[k]) + clt_ref.log_likelihood64(trees[k][1], trees[k][2], row[None, :])[0]
    return out


# ---- enumeration (small D) -----------------------------------------------------------------------------------------------------
def joint_every(model):
    """``[K, 2^D]`` float64: ``log(w_k p_k(x))`` for each of the complete rows of ``marginals_ref.every_row``."""
    trees, logw = model
    every = mref.every_row(len(trees[0][1]))
    with np.errstate(invalid='ignore'):
        return np.stack([float(lw) + clt_ref.log_likelihood64(tree, params, every) for (_, tree, params), lw in zip(trees, logw)])


def agrees(row):
    """Which of the ``2^D`` complete rows agree with the observed entries of ``row``."""
    row = np.asarray(row, np.float32)
    every = mref.every_row(len(row))
    obs = ~np.isnan(row)
    return (every[:, obs] == row[obs]).all(axis=1)


def marginals_by_enumeration(model, x):
    with np.errstate(invalid='ignore'):
        return mref.by_enumeration(np.exp(joint_every(model)).sum(axis=0), x)


def joint_posterior(model, row):
    """``[K, 2^D]`` float64: the posterior of (component, completion) given the observed entries of ``row``."""
    p = np.where(agrees(row)[None, :], np.exp(joint_every(model)), 0.0)
    return p / p.sum()


def best_by_enumeration(model, x):
    """``[B]`` float64: max over (k, completion of the row) of ``log(w_k p_k(x))``."""
    lj = joint_every(model)
    return np.array([np.where(agrees(row)[None, :], lj, -np.inf).max() for row in np.asarray(x, np.float32)])
