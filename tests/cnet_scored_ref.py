"""A numpy / ``math.lgamma`` restatement of the scored cutset learners as this project defines them:
``learn_cnet_bd`` and ``learn_cnet_bic`` with counts by boolean indexing, the float64 gains of tests/cnet_ref.py, the
float32 mutual information and tables of tests/clt_ref.py, and scores summed with ``math.fsum``.  It shares no code with
the package.

A model is the list of nodes of tests/cnet_ref.py (breadth first, left child before right) with three more keys per node:
``depth``, ``score`` (the score of the node's single tree) and ``candidates`` (``[(variable, score of cutting there)]`` in
the order they were tried).  ``cnet_ref.structure`` and ``cnet_ref.log_likelihood`` take it as it is.

The spanning tree is Prim's from position 0 by the rule of §17: the next position is the LOWEST one among those with the
heaviest link to the tree, and a position's link moves to a newer tree position only for a strictly heavier edge.
"""
import math
import os

import numpy as np

from tests import clt_ref, cnet_ref

GOLDEN = clt_ref.GOLDEN
BD_TREE_ALPHA = 0.01
# fixture -> (data config of cnet_ref.CONFIGS, learner, its parameter, n_cand_cuts)
CONFIGS = {
    'bd_d24': ('d24', 'bd', 0.1, 3),
    'bd_d33': ('d33', 'bd', 0.1, 3),
    'bd_d5': ('d5', 'bd', 0.1, 3),
    'bd_d10': ('d10', 'bd', 0.1, 3),
    'bic_d24': ('d24', 'bic', 0.01, 10),
    'bic_d33': ('d33', 'bic', 0.01, 3),
    'bic_d10': ('d10', 'bic', 0.01, 10),
}
_cache = {}


def data_of(name):
    """``(training rows, fresh rows)`` of a fixture's configuration."""
    return cnet_ref.mixture(*cnet_ref.CONFIGS[CONFIGS[name][0]][:5])


def golden(name):
    """tests/golden/cnet_<name>.npz as a dict with ``x`` and ``fresh`` unpacked; loaded once."""
    if name not in _cache:
        f = np.load(os.path.join(GOLDEN, 'cnet_%s.npz' % name))
        g = {k: f[k] for k in f.files}
        g['x'] = clt_ref.unpack(g['data'], int(g['n_rows']), int(g['n_vars']))
        g['fresh'] = clt_ref.unpack(g['fresh_bits'], cnet_ref.N_FRESH, int(g['n_vars']))
        _cache[name] = g
    return _cache[name]


def restated(name, seed=7):
    """The restatement's model of a fixture's data, leaf roots drawn from RandomState(seed); computed once."""
    key = ('fit', name, seed)
    if key not in _cache:
        _, kind, par, k = CONFIGS[name]
        _cache[key] = learn(golden(name)['x'], kind, par, k, random_state=np.random.RandomState(seed))
    return _cache[key]


# ---- scores ----------------------------------------------------------------------------------------------------------------
def cells_of(part):
    """``(n, cells [d, d, 2, 2])`` int64 by boolean indexing: ``cells[i, j, k, l]`` = rows with x_i = k and x_j = l."""
    b = np.asarray(part) == 1
    n, d = b.shape
    cells = np.zeros((d, d, 2, 2), np.int64)
    for k in (0, 1):
        for l in (0, 1):
            cells[:, :, k, l] = (b == bool(k)).T.astype(np.int64) @ (b == bool(l)).astype(np.int64)
    return n, cells


def or_bd_scores(part, ess):
    """``[d]``: lgamma(ess) - lgamma(n + ess) + sum over k of (lgamma(N_i(k) + ess / 2) - lgamma(ess / 2))."""
    b = np.asarray(part) == 1
    n = len(b)
    out = []
    for i in range(b.shape[1]):
        c1 = int(b[:, i].sum())
        out.append((math.lgamma(ess) - math.lgamma(n + ess)) + (math.lgamma(n - c1 + ess / 2) - math.lgamma(ess / 2))
                   + (math.lgamma(c1 + ess / 2) - math.lgamma(ess / 2)))
    return np.array(out, np.float64)


def family_bd(cell, ess):
    """The BDeu score of a child given a parent from ``cell[k, l]`` (child = k, parent = l)."""
    total = []
    for l in (0, 1):
        total.append((math.lgamma(ess / 2) - math.lgamma(int(cell[0, l] + cell[1, l]) + ess / 2))
                     + (math.lgamma(int(cell[0, l]) + ess / 4) - math.lgamma(ess / 4))
                     + (math.lgamma(int(cell[1, l]) + ess / 4) - math.lgamma(ess / 4)))
    return total[0] + total[1]


def clt_bd_scores(part, ess):
    """``[d, d]``, ``[i, j]`` = the BDeu score of i with parent j."""
    _, cells = cells_of(part)
    d = len(cells)
    return np.array([[family_bd(cells[i, j], ess) for j in range(d)] for i in range(d)], np.float64)


def tree_score(tree, clt_scores, or_scores):
    root = int(np.flatnonzero(np.asarray(tree) < 0)[0])
    return math.fsum([clt_scores[i, p] for i, p in enumerate(tree) if p >= 0] + [or_scores[root]])


def candidates(part, smoothing, k):
    """The positions of the ``k`` columns of largest gain (cnet_ref.scores with ``alpha = smoothing``), larger gain first,
    ties to the lower position; and the gains."""
    _, gains = cnet_ref.scores(part, smoothing)
    order = sorted(range(part.shape[1]), key=lambda i: (-gains[i], i))
    return order[:k], gains


def prim0(w):
    """Prim's maximum spanning tree from position 0 by the rule in the module docstring."""
    d = len(w)
    tree = np.full(d, -1, np.int32)
    link = np.zeros(d, np.int64)
    best = [float(w[0, v]) for v in range(d)]
    outside = [v for v in range(1, d)]
    while outside:
        v = max(outside, key=lambda u: (best[u], -u))
        tree[v] = link[v]
        outside.remove(v)
        for u in outside:
            if float(w[v, u]) > best[u]:
                best[u], link[u] = float(w[v, u]), v
    return tree


def rerooted(tree, root):
    scope = list(range(len(tree)))
    return cnet_ref.rooted(scope, [(i, int(p)) for i, p in enumerate(tree) if p >= 0], root)


def fit_tree(part, kind, par, depth, n_total):
    """``(tree from position 0, score)`` of a partition at ``depth``."""
    part = np.asarray(part)
    n, d = part.shape
    ones = clt_ref.counts(part)
    if kind == 'bd':
        ess = par / 2.0 ** depth
        tree = prim0(clt_ref.mutual_information(*clt_ref.priors_joints(ones, n, BD_TREE_ALPHA)))
        _, cells = cells_of(part)
        terms = [family_bd(cells[i, p], ess) for i, p in enumerate(tree) if p >= 0]
        return tree, math.fsum(terms + [float(or_bd_scores(part[:, :1], ess)[0])])
    priors, joints = clt_ref.priors_joints(ones, n, par)
    tree = prim0(clt_ref.mutual_information(priors, joints))
    with np.errstate(divide='ignore'):
        params = clt_ref.cpts(clt_ref.bfs_order(tree), tree, priors, joints).astype(np.float64)
    b = part == 1
    terms = []
    for i, p in enumerate(tree):
        for l in (0, 1):
            for k in (0, 1):
                count = int((b[:, i] == bool(k)).sum()) if p < 0 else int(((b[:, i] == bool(k)) & (b[:, p] == bool(l))).sum())
                if count and (p >= 0 or l == 0):
                    terms.append(count * float(params[i, l, k]))
    return tree, math.fsum(terms) - 0.5 * math.log(n_total) * (2 * d - 1)


def learn(data, kind, par, n_cand_cuts, random_state=None, roots=None):
    """The model (see the module docstring).  Leaf roots: position ``roots[k]`` for the k-th leaf if given, else
    ``random_state.choice(len(scope))`` per leaf in breadth-first order."""
    data = np.asarray(data)
    n_total, d = data.shape
    tree, score = fit_tree(data, kind, par, 0, n_total)
    model = [dict(scope=list(range(d)), rows=np.arange(n_total), depth=0, score=score, tree0=tree)]
    at = 0
    while at < len(model):
        node = model[at]
        at += 1
        part = data[node['rows']][:, node['scope']]
        n, width = part.shape
        depth = node['depth']
        ess = par / 2.0 ** depth
        node.update(or_id=-1, weights=None, children=None, candidates=[])
        if width == 1:
            continue
        order, _ = candidates(part, ess / 4 if kind == 'bd' else par, min(n_cand_cuts, width))
        best = None
        for i in order:
            right = part[:, i] == 1
            n_left, n_right = int((~right).sum()), int(right.sum())
            if n_left == 0 or n_right == 0:
                continue
            rest = [p for p in range(width) if p != i]
            sides = [fit_tree(part[side][:, rest], kind, par, depth + 1, n_total) for side in (~right, right)]
            if kind == 'bd':
                left_weight = (n_left + ess / 2) / (n + ess)
                own = float(or_bd_scores(part[:, i:i + 1], ess)[0])
            else:
                left_weight = (n_left + par) / (n + 2 * par)
                own = n_left * math.log(left_weight) + n_right * math.log(1 - left_weight) - 0.5 * math.log(n_total)
            total = math.fsum([sides[0][1], sides[1][1], own])
            node['candidates'].append((node['scope'][i], total))
            if best is None or total > best[0]:
                best = (total, i, right, left_weight, sides)
        if best is None or not best[0] > node['score']:
            continue
        _, i, right, left_weight, sides = best
        scope = [v for p, v in enumerate(node['scope']) if p != i]
        node.update(or_id=node['scope'][i], weights=[left_weight, 1 - left_weight], children=[len(model), len(model) + 1])
        model += [dict(scope=list(scope), rows=node['rows'][side], depth=depth + 1, score=s, tree0=t)
                  for side, (t, s) in zip((~right, right), sides)]
    n_leaves = 0
    for node in model:                                  # breadth first: the order of the draws
        if node['or_id'] >= 0:
            continue
        part = data[node['rows']][:, node['scope']]
        width = part.shape[1]
        root = int(random_state.choice(width)) if roots is None else int(roots[n_leaves])
        n_leaves += 1
        leaf_alpha = par / 2.0 ** node['depth'] / 4 if kind == 'bd' else par
        priors, joints = clt_ref.priors_joints(clt_ref.counts(part), len(part), leaf_alpha)
        tree = rerooted(node['tree0'], root)
        bfs = clt_ref.bfs_order(tree)
        with np.errstate(divide='ignore'):
            node.update(bfs=bfs, tree=tree, params=clt_ref.cpts(bfs, tree, priors, joints))
    return model
