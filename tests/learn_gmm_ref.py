"""A numpy float64 restatement of the Gaussian-mixture row split (include/deeprob_learn.h, "Gaussian-mixture
row splits"), in the manner of tests/learn_cont_ref.py: plain loops, one task at a time.  The EM is scikit-learn's
``GaussianMixture(covariance_type='full', tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=3)`` stated operation by
operation, from this project's Lloyd initialisations; the two device entries are restated with the summation orders the
header fixes (the quadratic form of the E-step) and with the terms of the sums it leaves to the partitioning (the moments:
the tests bound any order by the terms' absolute sum).

Margins recorded per run in ``stats``: ``lp_gap`` (the smallest gap between a row's two largest ``lp``, over every E-step
and the label pass), ``tol_margin`` (the smallest ``| |change| - 1e-3 |``), ``bound_gap`` (the smallest gap between the two
best initialisations' bounds of a task whose labels differ) and ``gap`` (the k-means distance gap).
"""
import numpy as np

from tests import learnspn_ref as disc, learn_cont_ref as cont
from tests.learn_cont_ref import sum256

N_INIT, TOL, REG, MAX_ITER = 3, 1e-3, 1e-6, 100
EPS64 = float(np.finfo(np.float64).eps)


# ---- features --------------------------------------------------------------------------------------------------------
def features(data, ks=None):
    """[n, F] float64: a float column (``ks`` None) or a column with K <= 2 is one feature, a column with K > 2 is K
    indicator features."""
    if ks is None:
        return cont.as_device(data)
    out = []
    for p, k in enumerate(ks):
        v = np.asarray(data)[:, p].astype(np.int64)
        out += [v.astype(np.float64)] if k <= 2 else [(v == q).astype(np.float64) for q in range(k)]
    return np.stack(out, axis=1)


# ---- the definition ----------------------------------------------------------------------------------------------------
def m_step(X, r):
    """(pi [C], mu [C, F], Sigma [C, F, F]) from responsibilities r [n, C]."""
    n, F = X.shape
    N = r.sum(axis=0) + 10.0 * EPS64
    mu = (r.T @ X) / N[:, None]
    sigma = np.empty((r.shape[1], F, F))
    for c in range(r.shape[1]):
        d = X - mu[c]
        sigma[c] = (r[:, c, None] * d).T @ d / N[c] + REG * np.eye(F)
    return N / n, mu, sigma


def log_prob(X, pi, mu, sigma):
    """lp [n, C]; ValueError when a covariance has no Cholesky factor."""
    n, F = X.shape
    lp = np.empty((n, len(pi)))
    for c in range(len(pi)):
        try:
            chol = np.linalg.cholesky(sigma[c])
        except np.linalg.LinAlgError:
            raise ValueError('ill-defined empirical covariance') from None
        y = np.linalg.solve(chol, (X - mu[c]).T).T
        lp[:, c] = -0.5 * (F * np.log(2.0 * np.pi) + np.sum(y * y, axis=1)) - np.sum(np.log(np.diag(chol))) + np.log(pi[c])
    return lp


def logsumexp(lp):
    m = lp.max(axis=1)
    return m + np.log(np.exp(lp - m[:, None]).sum(axis=1))


def lp_gap(lp):
    if lp.shape[1] < 2:
        return np.inf
    two = np.sort(lp, axis=1)[:, -2:]
    return float(np.min(two[:, 1] - two[:, 0]))


def em(X, r0, stats=None):
    """The loop of DESIGN.md 14.5 from the responsibilities ``r0``: a dict with ``labels``, ``lower``, ``n_iter``, ``pi``,
    ``mu``, ``sigma``."""
    stats = {} if stats is None else stats
    params, lower, n_iter = m_step(X, r0), -np.inf, 0
    for it in range(1, MAX_ITER + 1):
        lp = log_prob(X, *params)
        lse = logsumexp(lp)
        stats['lp_gap'] = min(stats.get('lp_gap', np.inf), lp_gap(lp))
        bound = float(np.mean(lse))
        params = m_step(X, np.exp(lp - lse[:, None]))
        change, lower, n_iter = bound - lower, bound, it
        if np.isfinite(change):
            stats['tol_margin'] = min(stats.get('tol_margin', np.inf), abs(abs(change) - TOL))
        if abs(change) < TOL:
            break
    lp = log_prob(X, *params)
    stats['lp_gap'] = min(stats.get('lp_gap', np.inf), lp_gap(lp))
    return dict(labels=np.argmax(lp, axis=1), lower=lower, n_iter=n_iter, pi=params[0], mu=params[1], sigma=params[2])


def one_hot(labels, C):
    return (labels[:, None] == np.arange(C)[None, :]).astype(np.float64)


def lloyd(data, ks, seed, C):
    """(labels, k-means gap) of one Lloyd restart of the project's k-means from the rows ``seed``."""
    if ks is None:
        run = cont.kmeans_restart(cont.as_device(data), seed, C)
        return run[0], run[4]
    run = disc.kmeans_restart(data, ks, seed, C)
    return run[0], run[3]


def gmm(data, ks, rs, n=2, stats=None):
    """The labels of the winning initialisation; three ``rs.choice`` draws."""
    stats = {} if stats is None else stats
    if len(data) < n:
        raise ValueError("n_samples={} should be >= n_clusters={}".format(len(data), n))
    seeds = [rs.choice(len(data), n, replace=False) for _ in range(N_INIT)]
    X, runs = features(data, ks), []
    for seed in seeds:
        labels, gap = lloyd(data, ks, seed, n)
        stats['gap'] = min(stats.get('gap', np.inf), gap)
        runs.append(em(X, one_hot(labels, n), stats))
    order = sorted(range(N_INIT), key=lambda i: -runs[i]['lower'])      # (stable: the first one on a tie)
    best = runs[order[0]]
    for i in order[1:]:
        if not np.array_equal(runs[i]['labels'], best['labels']):
            stats['bound_gap'] = min(stats.get('bound_gap', np.inf), best['lower'] - runs[i]['lower'])
            break
    stats['iterations'] = stats.get('iterations', 0) + max(r['n_iter'] for r in runs)
    return best['labels']


def kmeans(data, ks, rs, n=2, stats=None):
    """The project's k-means for one task (5 restarts)."""
    if ks is None:
        return cont.kmeans(cont.as_device(data), rs, n, stats)
    return disc.kmeans(np.asarray(data).astype(np.int64), ks, rs, n, stats)


# ---- the two existing task loops with gmm as the row split ---------------------------------------------------------------
def learn_spn_cont(data, stats=None, **kw):
    """tests/learn_cont_ref.learn_spn with the row clustering replaced by ``gmm``."""
    old = cont.kmeans
    cont.kmeans = lambda x, rs, n=2, st=None: gmm(x.astype(np.float32), None, rs, n, st)
    try:
        return cont.learn_spn(data, split_rows='kmeans', stats=stats, **kw)
    finally:
        cont.kmeans = old


def learn_spn_disc(data, names, ks, stats=None, **kw):
    """tests/learnspn_ref.learn_spn with the row clustering replaced by ``gmm``."""
    old = disc.kmeans
    disc.kmeans = lambda d, lks, rs, n=2, st=None: gmm(d, lks, rs, n, st)
    try:
        return disc.learn_spn(data, names, ks, split_rows='kmeans', stats=stats, **kw)
    finally:
        disc.kmeans = old


# ---- the two entries ----------------------------------------------------------------------------------------------------
def pack(pi, mu, sigma):
    """The parameters as the entries take them: [C, 1 + F + F * F] = k_c, mu_c, W_c = L_c^-1 (upper triangle 0.0)."""
    C, F = mu.shape
    out = np.zeros((C, 1 + F + F * F))
    for c in range(C):
        chol = np.linalg.cholesky(sigma[c])
        out[c, 0] = np.log(pi[c]) - 0.5 * F * np.log(2.0 * np.pi) - np.sum(np.log(np.diag(chol)))
        out[c, 1:1 + F] = mu[c]
        out[c, 1 + F:] = np.tril(np.linalg.inv(chol)).reshape(-1)
    return out


def estep_entry(X, par):
    """(lp [n, C], resp [n, C], labels [n], lse [n], the summed lse) of dpl_gmm_estep, the quadratic form in the header's
    order of operations; exp and log are numpy's."""
    n, F = X.shape
    C = len(par)
    lp = np.empty((n, C))
    for c in range(C):
        mu, W = par[c, 1:1 + F], par[c, 1 + F:].reshape(F, F)
        d = X - mu[None, :]
        y = np.zeros((n, F))
        for j in range(F):
            y = y + W[:, j][None, :] * d[:, j:j + 1]
        q = np.zeros(n)
        for i in range(F):
            q = q + y[:, i] * y[:, i]
        lp[:, c] = par[c, 0] + (-0.5 * q)
    m = lp.max(axis=1)
    s = np.zeros(n)
    for c in range(C):
        s = s + np.exp(lp[:, c] - m)
    lse = m + np.log(s)
    return lp, np.exp(lp - lse[:, None]), np.argmax(lp, axis=1), lse, sum256(lse)


def mstats_entry(X, w, pivot):
    """(stats [1 + F + F * F], absolute sums of the terms, same shape) of dpl_gmm_mstats for ONE component: N, s, M with
    M[g][f] = sum_r (w_r a_rf) a_rg; the sums are numpy's (the tests bound any order by the absolute sums)."""
    n, F = X.shape
    a = X - pivot[None, :]
    wa = w[:, None] * a
    terms = wa[:, None, :] * a[:, :, None]                      # [n, g, f]
    stats = np.concatenate([[w.sum()], wa.sum(axis=0), terms.sum(axis=0).reshape(-1)])
    bound = np.concatenate([[np.abs(w).sum()], np.abs(wa).sum(axis=0), np.abs(terms).sum(axis=0).reshape(-1)])
    return stats, bound


# ---- the end-to-end cases of tests/test_learn_gmm_gpu.py; the seeds were chosen on the CPU with this file alone so that the
# preconditions hold (tests/test_learn_gmm_host.py asserts them): lp gap >= 1e-6, tolerance margin >= 1e-7, k-means gap >=
# 1e-9, bound gap >= 1e-9
def three_floats(n=600, seed=0):
    """n rows of 3 float columns: two clusters that differ in location and in shape."""
    rs = np.random.RandomState(seed)
    z = rs.rand(n) < 0.4
    a = rs.randn(n, 3) * np.array([1.0, 0.3, 2.0]) + np.array([0.0, 0.0, 0.0])
    b = rs.randn(n, 3) * np.array([0.4, 1.5, 0.5]) + np.array([3.0, -2.0, 1.0])
    return np.where(z[:, None], a, b).astype(np.float32)


def binary16(n=400, seed=3, n_clusters=3, noise=0.15):
    """n rows of 16 binary columns from a mixture of noisy prototypes."""
    return disc.mixture([2] * 16, n, seed, n_clusters=n_clusters, noise=noise)[0]


def binary16_e2e():
    return binary16(n_clusters=2, noise=0.3)


STANDALONE = dict(float=dict(seed=0, n=2), binary=dict(seed=1, n=2))
E2E_CONT = dict(split_cols='rdc', min_rows_slice=128, random_state=17)
E2E_DISC = dict(split_cols='gvs', min_rows_slice=100, random_state=59)
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def standalone(which):
    """(data, ks, restated gmm labels, restated kmeans labels, stats) of a stand-alone case."""
    def make():
        data, ks = (three_floats(), None) if which == 'float' else (binary16(), [2] * 16)
        cfg, stats = STANDALONE[which], {}
        lab = gmm(data, ks, np.random.RandomState(cfg['seed']), cfg['n'], stats)
        km = kmeans(data, ks, np.random.RandomState(cfg['seed']), cfg['n'], stats)
        return data, ks, lab, km, stats
    return cached(('standalone', which), make)


def e2e_cont():
    def make():
        stats = {}
        return learn_spn_cont(cont.two_blocks(), stats=stats, **E2E_CONT), stats
    return cached('e2e_cont', make)


def e2e_disc():
    def make():
        stats = {}
        return learn_spn_disc(binary16_e2e(), ['Bernoulli'] * 16, [2] * 16, stats=stats, **E2E_DISC), stats
    return cached('e2e_disc', make)


def preconditions(stats):
    """Whether a run's margins allow an exact comparison of labels."""
    return (stats.get('lp_gap', np.inf) >= 1e-6 and stats.get('tol_margin', np.inf) >= 1e-7 and stats.get('gap', np.inf) >= 1e-9
            and stats.get('bound_gap', np.inf) >= 1e-9)
