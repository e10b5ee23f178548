"""Float64 oracle (test helper, numpy / scipy) for the posterior queries of a node-graph SPN: ``E[x_j^k | e]`` and
``p(x_j = v | e)`` as RATIOS OF TWO FORWARD EVALUATIONS -- the circuit with every leaf over ``j`` replaced by the constant
``m_k(L)`` (or ``p_L(v)``), over the plain forward -- so nothing here shares a backward pass with the kernel under test.
The root polynomial is linear in the leaves of one variable, which makes the ratio exact.  Leaf moments come from
scipy.stats, as the reference takes them (leaf.py ``moment``), not from the closed forms of include/deeprob_spnq.h.

Values are kept as (sign, log |value|), because odd moments can be negative and densities underflow a linear float64.
Beside each entry the oracle returns its scale ``sum_L r_L |m_k(L)|``: the size of the terms the entry is a sum of, which
is what an error is measured against where the terms cancel.

Checked against enumeration and the reference's goldens by tests/test_flat_spn_posterior_host.py."""
import copy
import warnings

import numpy as np
import scipy.stats as ss

from oracle import flat_spn_oracle as forc

LEAVES = ('Bernoulli', 'Categorical', 'Uniform', 'Gaussian')


class Oracle:
    def __init__(self, d):
        self.nodes, self.children = forc.load(copy.deepcopy(d))
        self.order = forc.evaluation_order(self.children)
        self.n_features = 1 + max(v for n in self.nodes.values() for v in n['scope'])
        self.var_leaves = {}
        for i in sorted(self.nodes):
            if self.nodes[i]['class'] in LEAVES:
                self.var_leaves.setdefault(int(self.nodes[i]['scope'][0]), []).append(i)
        self._moments = {}
        self.parents = {i: [] for i in self.nodes}
        for i, kids in self.children.items():
            for c in kids:
                self.parents[c].append(i)

    # ---- leaves ----------------------------------------------------------------------------------------------------------
    def leaf_ll(self, i, col):
        """log density of leaf i on a float32 column in float64 (NaN: log 1); the forward pass's support rules."""
        n = self.nodes[i]
        p, name = n['params'], n['class']
        col = np.asarray(col, np.float32).astype(np.float64)
        out = np.zeros(len(col))
        live = ~np.isnan(col)
        v = col[live]
        with np.errstate(divide='ignore', invalid='ignore'):
            if name == 'Bernoulli':
                q = float(p['p'])
                r = np.where(v == 1.0, np.log(q) if q > 0 else -np.inf,
                             np.where(v == 0.0, np.log1p(-q) if q < 1 else -np.inf, -np.inf))
            elif name == 'Categorical':
                r = np.full(len(v), -np.inf)
                cat = v.astype(np.int64)
                for c, q in zip(p['categories'], np.asarray(p['probabilities'], np.float32).astype(np.float64)):
                    r[cat == int(c)] = np.log(q)
            elif name == 'Uniform':
                z = (v - float(p['start'])) / float(p['width'])
                r = np.where((z >= 0.0) & (z <= 1.0), -np.log(float(p['width'])), -np.inf)
            else:
                z = (v - float(p['mean'])) / float(p['stddev'])
                r = -0.5 * z * z - 0.5 * np.log(2.0 * np.pi) - np.log(float(p['stddev']))
        out[live] = r
        return out

    def leaf_moment(self, i, k):
        """Non-central moment of order k of leaf i, from scipy.stats as the reference's leaves take it."""
        if (i, k) not in self._moments:
            n = self.nodes[i]
            p, name = n['params'], n['class']
            if name == 'Bernoulli':
                m = ss.bernoulli.moment(k, float(p['p']))
            elif name == 'Categorical':
                cats = np.asarray(p['categories'], np.int64)
                probs = np.asarray(p['probabilities'], np.float32).astype(np.float64)
                m = float(np.sum(cats.astype(np.float64) ** k * probs))      # (rv_discrete.moment: the same sum)
            elif name == 'Uniform':
                m = ss.uniform.moment(k, float(p['start']), float(p['width']))
            else:
                m = ss.norm.moment(k, float(p['mean']), float(p['stddev']))
            self._moments[(i, k)] = float(m)
        return self._moments[(i, k)]

    def leaf_prob(self, i, v):
        n = self.nodes[i]
        p, name = n['params'], n['class']
        if name == 'Bernoulli':
            return float(p['p']) if v == 1.0 else 1.0 - float(p['p']) if v == 0.0 else 0.0
        if name == 'Categorical':
            for c, q in zip(p['categories'], np.asarray(p['probabilities'], np.float32).astype(np.float64)):
                if int(c) == int(v):
                    return float(q)
        return 0.0

    # ---- forward, (sign, log |value|) ---------------------------------------------------------------------------------------
    def forward(self, x, replaced=None, var=None, plain=None, tables=False):
        """(sign [B], log |root| [B]); ``replaced``: {leaf id: real values [B]} taken in place of the leaf's density.
        ``tables``: return the per-node dicts instead.  ``plain`` (the tables of a plain forward on the rows that ``x``
        repeats ``len(x) / len(plain rows)`` times) with ``var``: a node whose scope does not hold ``var`` has its plain
        value, which is repeated instead of computed again."""
        x = np.asarray(x)
        B = len(x)
        replaced = replaced or {}
        sg, lg = {}, {}
        if plain is not None:
            reps = B // len(plain[0][0])
            for i in self.order:
                if var not in self.nodes[i]['scope'] and any(var in self.nodes[q]['scope'] for q in self.parents[i]):
                    sg[i], lg[i] = np.tile(plain[0][i], reps), np.tile(plain[1][i], reps)
        with warnings.catch_warnings(), np.errstate(divide='ignore', invalid='ignore'):
            warnings.simplefilter('ignore')
            for i in self.order:
                n, kids = self.nodes[i], self.children[i]
                if i in lg or (plain is not None and var not in n['scope']):
                    continue
                if n['class'] == 'Sum':
                    w = np.asarray(n['weights'], np.float32).astype(np.float64)
                    # signed log-sum-exp, written out (scipy's costs several times as much per call on these shapes)
                    a = np.stack([lg[c] for c in kids], axis=1)
                    b = np.stack([sg[c] for c in kids], axis=1) * w[None, :]
                    top = np.max(a, axis=1)
                    top = np.where(np.isfinite(top), top, 0.0)
                    s = np.sum(b * np.exp(a - top[:, None]), axis=1)
                    lg[i] = np.where(s == 0, -np.inf, np.log(np.abs(s)) + top)
                    sg[i] = np.where(s < 0, -1.0, 1.0)
                elif n['class'] == 'Product':
                    lg[i] = np.sum(np.stack([lg[c] for c in kids], axis=1), axis=1)
                    sg[i] = np.prod(np.stack([sg[c] for c in kids], axis=1), axis=1)
                elif i in replaced:
                    r = np.broadcast_to(np.asarray(replaced[i], np.float64), (B,))
                    lg[i] = np.log(np.abs(r))
                    sg[i] = np.where(r < 0, -1.0, 1.0)
                else:
                    lg[i] = self.leaf_ll(i, x[:, n['scope'][0]])
                    sg[i] = np.ones(B)
        return (sg, lg) if tables else (sg[0], lg[0])

    def log_likelihood(self, x):
        return self.forward(x)[1]

    def _ratios(self, x, j, columns, plain):
        """[len(columns), B]: root with the leaves over j replaced by columns[c][leaf], over the plain root; NaN where the
        evidence has probability zero.  ``plain``: forward(x, tables=True)."""
        x = np.asarray(x, np.float32)
        B, C = len(x), len(columns)
        big = np.tile(x, (C, 1))
        replaced = {L: np.repeat(np.asarray([col[L] for col in columns], np.float64), B) for L in self.var_leaves[j]}
        s, l = self.forward(big, replaced, var=j, plain=plain)
        den = plain[1][0]
        with np.errstate(invalid='ignore'):
            out = s.reshape(C, B) * np.exp(l.reshape(C, B) - den[None, :])
        out[:, ~np.isfinite(den)] = np.nan
        return out

    # ---- the queries ---------------------------------------------------------------------------------------------------------
    def moments(self, x, n_orders):
        """(want, scale), each [n_orders, B, D] float64, with the conventions of DPQ_MODE_MOMENTS."""
        x = np.asarray(x, np.float32)
        B, D = x.shape
        want = np.empty((n_orders, B, D))
        scale = np.empty((n_orders, B, D))
        plain = self.forward(x, tables=True)
        for j in range(D):
            col = x[:, j].astype(np.float64)
            if j not in self.var_leaves:
                want[:, :, j] = col[None, :]
                scale[:, :, j] = np.abs(col)[None, :]
                continue
            cols = [{L: self.leaf_moment(L, k) for L in self.var_leaves[j]} for k in range(1, n_orders + 1)]
            cols += [{L: abs(m) for L, m in c.items()} for c in cols]
            r = self._ratios(x, j, cols, plain)
            nan = np.isnan(col)
            for k in range(n_orders):
                want[k, :, j] = np.where(nan, r[k], col ** (k + 1))
                scale[k, :, j] = np.where(nan, r[n_orders + k], np.abs(col) ** (k + 1))
        return want, scale

    def posterior(self, x, var, values):
        """[B, V] float64 with the conventions of DPQ_MODE_VALUES."""
        x = np.asarray(x, np.float32)
        values = np.asarray(values, np.float32)
        r = self._ratios(x, var, [{L: self.leaf_prob(L, float(v)) for L in self.var_leaves[var]} for v in values],
                         self.forward(x, tables=True)).T
        col = x[:, var]
        seen = ~np.isnan(col)
        out = np.where(seen[:, None], (values[None, :] == col[:, None]).astype(np.float64), r)
        out[~np.isfinite(self.log_likelihood(x))] = np.nan
        return out


def statistics(m):
    """(variance, skewness, kurtosis) in float64 from non-central moments m [4, ...]: the textbook central moments."""
    m1, m2, m3, m4 = (np.asarray(v, np.float64) for v in m)
    with np.errstate(divide='ignore', invalid='ignore'):
        var = m2 - m1 ** 2
        skew = (m3 - 3 * m1 * m2 + 2 * m1 ** 3) / var ** 1.5
        kurt = (m4 - 4 * m1 * m3 + 6 * m1 ** 2 * m2 - 3 * m1 ** 4) / var ** 2 - 3.0
    return var, skew, kurt


def enumerate_binary(oracle: Oracle, x):
    """E[x_j | e] [B, D] of a circuit over binary variables by enumerating every completion of every row."""
    x = np.asarray(x, np.float32)
    B, D = x.shape
    grid = np.array([[(s >> v) & 1 for v in range(D)] for s in range(1 << D)], np.float32)
    joint = np.exp(oracle.log_likelihood(grid))
    out = np.empty((B, D))
    for b in range(B):
        seen = ~np.isnan(x[b])
        ok = (grid[:, seen] == x[b, seen]).all(axis=1)
        with np.errstate(invalid='ignore', divide='ignore'):
            out[b] = (joint[ok, None] * grid[ok]).sum(axis=0) / joint[ok].sum()
    return out
