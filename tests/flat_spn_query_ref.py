"""CPU restatement (test helper, numpy / scipy) of the node-graph SPN queries of the reference on its JSON export:
``mpe`` (deeprob/spn/algorithms/inference.py:61-126 over evaluation.py:99-177), ``eval_backward`` (gradient.py:13-63),
one EM step (learning/em.py:84-107 with node.py:100-111 and leaf.py:167-174, 281-293, 536-545) in the reference's own
precision (float32 tables) and in float64, and a replay of the HIP sampler's documented counters
(csrc/flat_spn_queries.hip).  Pinned to the reference's goldens by tests/test_flat_spn_queries_host.py."""
import copy
import warnings

import numpy as np
import scipy.stats as ss
from scipy.special import logsumexp

from oracle import flat_spn_oracle as forc

FLOOR = -1e31
GROUPS = ('sum_w', 'bern_p', 'cat_p', 'gauss_mean', 'gauss_std')


class State:
    """Mutable parameters of a circuit: ``weights[i]`` of sum nodes, ``params[i]`` of leaves; dtype = the precision of
    the node tables (float32 = the reference's)."""

    def __init__(self, d, dtype=np.float32):
        self.nodes, self.children = forc.load(copy.deepcopy(d))
        self.dtype = dtype
        self.order = forc.evaluation_order(self.children)
        self.n = max(self.nodes) + 1
        wt = np.float32 if dtype == np.float32 else np.float64
        self.weights, self.params = {}, {}
        for i, n in self.nodes.items():
            if n['class'] == 'Sum':
                self.weights[i] = np.array(n['weights'], dtype=np.float32).astype(wt)      # node.py:83-84
            elif n['class'] != 'Product':
                p = dict(n['params'])
                if n['class'] == 'Categorical':                                        # leaf.py:236-241
                    p['categories'] = np.array(p['categories'], np.int64)
                    p['probabilities'] = np.array(p['probabilities'], np.float32).astype(wt)
                self.params[i] = p

    def bfs(self):
        seen, queue, out = {0}, [0], []
        while queue:
            n = queue.pop(0)
            out.append(n)
            for c in self.children[n]:
                if c not in seen:
                    seen.add(c)
                    queue.append(c)
        return out


def params_of(st: State):
    """The parameter groups in node-id order (sum weights in child order)."""
    g = {k: [] for k in GROUPS}
    for i in sorted(st.nodes):
        name = st.nodes[i]['class']
        if name == 'Sum':
            g['sum_w'] += list(np.asarray(st.weights[i], np.float64))
        elif name == 'Bernoulli':
            g['bern_p'].append(float(st.params[i]['p']))
        elif name == 'Categorical':
            g['cat_p'] += list(np.asarray(st.params[i]['probabilities'], np.float64))
        elif name == 'Gaussian':
            g['gauss_mean'].append(float(st.params[i]['mean']))
            g['gauss_std'].append(float(st.params[i]['stddev']))
    return {k: np.asarray(v, np.float64) for k, v in g.items()}


def flat_params(spn):
    """The same groups from a deeprob.spn.structure.io.FlatSpn."""
    from deeprob.spn.structure.io import KIND
    g = {k: [] for k in GROUPS}
    for i in range(spn.n_nodes):
        k = spn.kind[i]
        if k == KIND['Sum']:
            g['sum_w'] += list(spn.child_weight[spn.arg0[i]:spn.arg0[i] + spn.arg1[i]].astype(np.float64))
        elif k == KIND['Bernoulli']:
            g['bern_p'].append(spn.raw0[i])
        elif k == KIND['Categorical']:
            g['cat_p'] += list(spn.probabilities[spn.arg1[i]:spn.arg1[i] + spn.arg2[i]])
        elif k == KIND['Gaussian']:
            g['gauss_mean'].append(spn.raw0[i])
            g['gauss_std'].append(spn.raw1[i])
    return {k: np.asarray(v, np.float64) for k, v in g.items()}


def _leaf_ll(name, p, col, dtype):
    lls = np.zeros(len(col), dtype=dtype)
    live = ~np.isnan(col)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if name == 'Bernoulli':
            lls[live] = ss.bernoulli.logpmf(col[live], p['p'])
        elif name == 'Categorical':
            cat = col[live].astype(np.int64)
            v = np.full(len(cat), -np.inf)
            for c, q in zip(p['categories'], p['probabilities']):
                v[cat == c] = np.log(np.float64(q))
            lls[live] = v
        elif name == 'Uniform':
            lls[live] = ss.uniform.logpdf(col[live], p['start'], p['width'])
        else:
            lls[live] = ss.norm.logpdf(col[live], p['mean'], p['stddev'])
    return lls


def forward(st: State, x):
    """[n_nodes, B] node values (inference.py:94-103; clamped at -1e31, stored in st.dtype)."""
    x = np.asarray(x)
    ls = np.empty((st.n, len(x)), dtype=st.dtype)
    for i in st.order:
        n, kids = st.nodes[i], st.children[i]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if n['class'] == 'Sum':
                v = logsumexp(np.stack([ls[c] for c in kids], axis=1), b=st.weights[i], axis=1)
            elif n['class'] == 'Product':
                v = np.sum(np.stack([ls[c] for c in kids], axis=1), axis=1)
            else:
                v = _leaf_ll(n['class'], st.params[i], x[:, n['scope'][0]], st.dtype)
        ls[i] = np.maximum(v, FLOOR)
    return ls


def near_tie(best, second):
    """A sum node's two best candidates differ by more than zero and less than 1e-4 max(1, |best|)."""
    with np.errstate(invalid='ignore'):
        diff = best.astype(np.float64) - second.astype(np.float64)
        return (diff > 0) & (diff < 1e-4 * np.maximum(1.0, np.abs(best.astype(np.float64))))


def mpe(st: State, x, lls=None):
    """(filled inputs, rows that meet a near-tie at a sum node they reach)."""
    x = np.array(x, copy=True)
    lls = forward(st, x) if lls is None else lls
    masks = np.zeros((st.n, len(x)), bool)
    masks[0] = True
    near = np.zeros(len(x), bool)
    for i in reversed(st.order):
        n, kids = st.nodes[i], st.children[i]
        if n['class'] == 'Sum':
            with np.errstate(divide='ignore'):
                wl = np.stack([lls[c] for c in kids], axis=1) + np.log(st.weights[i])      # inference.py:125
            branch = np.argmax(wl, axis=1)
            if len(kids) > 1:
                srt = np.sort(wl, axis=1)
                near |= masks[i] & near_tie(srt[:, -1], srt[:, -2])
            for k, c in enumerate(kids):
                masks[c] |= masks[i] & (branch == k)
        elif n['class'] == 'Product':
            for c in kids:
                masks[c] |= masks[i]
        else:
            v, p = n['scope'][0], st.params[i]
            sel = masks[i] & np.isnan(x[:, v])
            if n['class'] == 'Bernoulli':
                x[sel, v] = 0 if p['p'] < 0.5 else 1
            elif n['class'] == 'Categorical':
                x[sel, v] = p['categories'][np.argmax(p['probabilities'])]
            elif n['class'] == 'Uniform':
                x[sel, v] = p['start']
            else:
                x[sel, v] = p['mean']
    return x, near


def backward(st: State, lls):
    """gradient.py:13-63 on the table of forward(); result in st.dtype."""
    grads = np.empty(lls.shape, dtype=st.dtype)
    cached = {i: [] for i in st.nodes}
    grads[0] = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for i in reversed(st.order):
            if i != 0:
                grads[i] = logsumexp(cached[i], axis=0)
                cached[i] = None
            n = st.nodes[i]
            if n['class'] == 'Sum':
                for c, w in zip(st.children[i], st.weights[i]):
                    cached[c].append(grads[i] + np.log(w))
            elif n['class'] == 'Product':
                for c in st.children[i]:
                    cached[c].append(grads[i] + lls[i] - lls[c])
    return grads


def em_init(st: State, rs):
    order = st.bfs()
    for i in order:
        if st.nodes[i]['class'] == 'Sum':
            st.weights[i] = rs.dirichlet(np.ones(len(st.children[i]))).astype(np.float32).astype(st.weights[i].dtype)
    for i in order:
        name = st.nodes[i]['class']
        if name == 'Bernoulli':
            st.params[i]['p'] = rs.rand()
        elif name == 'Categorical':
            st.params[i]['probabilities'] = rs.dirichlet(np.ones(len(st.params[i]['categories'])))
        elif name == 'Gaussian':
            st.params[i]['mean'] = 1e-1 * rs.randn()
            st.params[i]['stddev'] = 0.5 + 1e-1 * np.tanh(rs.randn())
        elif name == 'Uniform':
            raise NotImplementedError


def em_step(st: State, batch, eta):
    """One iteration of em.py:84-107 on `batch`; every statistic is taken before any parameter changes.  Returns the
    batch mean log-likelihood."""
    lls = forward(st, batch)
    root_ll = lls[0]
    grads = backward(st, lls)
    eps, alpha = np.finfo(np.float32).eps, np.finfo(np.float16).eps
    if st.dtype != np.float32:
        eps, alpha = float(eps), float(alpha)
    new_w, new_p = {}, {}
    for i, n in st.nodes.items():
        name = n['class']
        if name == 'Sum':
            stats = np.exp(lls[st.children[i]] - root_ll + grads[i])
            w = st.weights[i]
            un = w * np.sum(stats, axis=1) + eps
            new_w[i] = (1.0 - eta) * w + eta * (un / np.sum(un))
        elif name != 'Product':
            stats = np.exp(lls[i] - root_ll + grads[i])
            data, p = batch[:, n['scope'][0]], dict(st.params[i])
            if st.dtype != np.float32:
                data = data.astype(np.float64)
            total = np.sum(stats)
            if name == 'Bernoulli':
                p['p'] = (1.0 - eta) * p['p'] + eta * ((np.dot(stats, data) + alpha) / (total + 2 * alpha))
            elif name == 'Categorical':
                K = len(p['categories'])
                est = np.empty(K, np.float32 if st.dtype == np.float32 else np.float64)
                for k, c in enumerate(p['categories']):
                    est[k] = (np.sum(stats[data == c]) + alpha) / (total + K * alpha)
                p['probabilities'] = (1.0 - eta) * p['probabilities'] + eta * est
            elif name == 'Gaussian':
                total = total + eps
                mean = np.sum(stats * data) / total
                sd = max(np.sqrt(np.sum(stats * (data - mean) ** 2.0) / total), 1e-5)
                p['mean'] = (1.0 - eta) * p['mean'] + eta * mean
                p['stddev'] = (1.0 - eta) * p['stddev'] + eta * sd
            else:
                raise NotImplementedError
            new_p[i] = p
    st.weights.update(new_w)
    st.params.update(new_p)
    return float(np.mean(root_ll))


def em_run(d, data, index, eta, dtype, random_init_state=None):
    """EM over the given batch-index rows; returns the State."""
    st = State(d, dtype)
    if random_init_state is not None:
        em_init(st, random_init_state)
    for rows in index:
        em_step(st, data[rows], eta)
    return st


def to_json(st: State, d):
    """The export `d` with the State's parameters (full precision)."""
    out = copy.deepcopy(d)
    for n in out['nodes']:
        i = int(n['id'])
        if n['class'] == 'Sum':
            n['weights'] = [float(w) for w in st.weights[i]]
        elif n['class'] != 'Product':
            n['params'] = {k: (np.asarray(v).tolist() if isinstance(v, np.ndarray) else float(v))
                           for k, v in st.params[i].items()}
    return out


# ---- replay of the HIP sampler (counter layout: header of csrc/flat_spn_queries.hip) --------------------------------
def uniform01(seed, ctr):
    with np.errstate(over='ignore'):
        z = np.uint64(seed) + np.asarray(ctr, np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def _inverse_cdf(t, u):
    """first k with u * total < t_0 + .. + t_k (float32, in order), else the last k with t_k > 0; and whether u lies
    within 1e-5 of a boundary of the normalised CDF."""
    cum = np.cumsum(t, axis=1, dtype=np.float32)
    total = cum[:, -1]
    target = (u * total).astype(np.float32)
    hit = target[:, None] < cum
    pick = np.where(hit.any(axis=1), np.argmax(hit, axis=1), 0)
    lastpos = t.shape[1] - 1 - np.argmax((t > 0)[:, ::-1], axis=1)
    pick = np.where(hit.any(axis=1), pick, lastpos)
    edge = np.min(np.abs(u[:, None].astype(np.float64) - cum.astype(np.float64) / total[:, None].astype(np.float64)), axis=1)
    return pick, edge < 1e-5


def sample_replay(st: State, x, seed, n_vars):
    """(filled inputs, rows that used a uniform within 1e-5 of an inverse-CDF boundary)."""
    x = np.array(x, copy=True)
    B = len(x)
    lls = forward(st, x)
    sums = [i for i in sorted(st.nodes) if st.nodes[i]['class'] == 'Sum']
    sidx = {i: s for s, i in enumerate(sums)}
    K = len(sums) + 2 * n_vars
    ctr0 = np.arange(B, dtype=np.uint64) * np.uint64(K)
    masks = np.zeros((st.n, B), bool)
    masks[0] = True
    near = np.zeros(B, bool)
    for i in reversed(st.order):
        n, kids = st.nodes[i], st.children[i]
        if n['class'] == 'Sum':
            with np.errstate(divide='ignore'):
                l = np.stack([lls[c] for c in kids], axis=1).astype(np.float32)
                lw = np.log(st.weights[i]).astype(np.float32)[None, :]
            j = np.argmax(l + lw, axis=1)[:, None]
            with np.errstate(invalid='ignore'):
                t = np.exp((l - np.take_along_axis(l, j, 1)) + (lw - lw[0][j])).astype(np.float32)
            branch, edge = _inverse_cdf(t, uniform01(seed, ctr0 + np.uint64(sidx[i])))
            near |= masks[i] & edge
            for k, c in enumerate(kids):
                masks[c] |= masks[i] & (branch == k)
        elif n['class'] == 'Product':
            for c in kids:
                masks[c] |= masks[i]
        else:
            v, p = n['scope'][0], st.params[i]
            sel = masks[i] & np.isnan(x[:, v])
            u1 = uniform01(seed, ctr0 + np.uint64(len(sums) + 2 * v))
            u2 = uniform01(seed, ctr0 + np.uint64(len(sums) + 2 * v + 1))
            if n['class'] == 'Bernoulli':
                pf = np.float32(p['p'])
                x[sel, v] = (u1 < pf)[sel].astype(np.float32)
                near |= sel & (np.abs(u1.astype(np.float64) - float(pf)) < 1e-5)
            elif n['class'] == 'Categorical':
                t = np.tile(np.asarray(p['probabilities'], np.float32)[None, :], (B, 1))
                pick, edge = _inverse_cdf(t, u1)
                x[sel, v] = p['categories'][pick][sel]
                near |= sel & edge
            elif n['class'] == 'Uniform':
                x[sel, v] = (np.float32(p['start']) + np.float32(p['width']) * u1)[sel]
            else:
                z = np.sqrt(-2.0 * np.log(1.0 - u1.astype(np.float64))) * np.cos(2.0 * np.pi * u2.astype(np.float64))
                x[sel, v] = (p['mean'] + p['stddev'] * z)[sel].astype(np.float32)
    return x, near
