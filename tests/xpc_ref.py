"""A numpy restatement of the XPC learners as this project defines them (DESIGN.md "XPCs"): the random partition tree with
the reference's order of random draws, the leaves (naive factorizations, conjunctions, deterministic disjunctions,
Chow-Liu trees from tests/clt_ref.py), the trees of structured-decomposable circuits, and the evaluation of the circuit
in float64 with NaN marginalised.  It filters the data rows directly -- no histograms, no device -- and shares no code with
the package.

A partition is a dict: ``rows`` (ascending indices into the training data), ``cols``, ``uncond`` (the columns still free
for conjunctions), ``subs`` (sub-partitions), ``naive``, ``conj``, ``disc`` (sorted tuples over ``cols``, or None), and
after learning ``leaf``: ('conj', values) | ('naive', p) | ('disj', weights, assignments) |
('clt', scope, bfs, tree, params).
"""
import itertools
import os

import numpy as np

from tests import clt_ref, cnet_ref

GOLDEN = clt_ref.GOLDEN
N_FRESH = cnet_ref.N_FRESH
SD_LEVEL_0, SD_LEVEL_1, SD_LEVEL_2 = 0, 1, 2
GLOBAL_SEED = 11            # np.random.seed in front of learn_expc: the members' orderings come from the global generator

# name -> (learner, (n, d, k, noise, seed) of cnet_ref.mixture, keyword arguments).  The seeds are the first from 1 .. 7
# upwards that tools/gen_golden_xpc.py --search accepts: a Chow-Liu leaf that learns its own tree must have ONE maximum
# spanning tree, or the likelihoods depend on which of several a routine returns.  The non-SD ensemble has some 65 such
# leaves of as few as 64 rows, 5 to 15 of them tied whatever the seed (none of 200 seeds passes), so it is the configuration
# with use_clt=False; leaves that learn their own trees are covered by a12 and b24det.
CONFIGS = {
    'a12': ('xpc', (600, 12, 3, 0.2, 2), dict(det=False, sd=False, min_part_inst=32, conj_len=2, arity=3, n_max_parts=40)),
    'b24det': ('xpc', (2000, 24, 4, 0.2, 9), dict(det=True, sd=False, min_part_inst=64, conj_len=3, arity=4, n_max_parts=50)),
    'c24sd': ('xpc', (2000, 24, 4, 0.2, 4), dict(det=False, sd=True, min_part_inst=32, conj_len=2, arity=3, n_max_parts=50)),
    'd40sd': ('xpc', (4097, 40, 5, 0.2, 4), dict(det=True, sd=True, min_part_inst=64, conj_len=3, arity=4, n_max_parts=60)),
    'e40naive': ('xpc', (4097, 40, 5, 0.2, 5), dict(det=False, sd=False, min_part_inst=32, conj_len=3, arity=3, n_max_parts=60,
                                                    use_clt=False)),
    'f24greedy': ('xpc', (2000, 24, 4, 0.2, 6), dict(det=False, sd=True, min_part_inst=32, conj_len=2, arity=4, n_max_parts=40,
                                                     use_greedy_ordering=True)),
    'g24e0': ('expc', (2000, 24, 4, 0.2, 7), dict(ensemble_dim=4, det=False, sd_level=0, min_part_inst=64, conj_len=2, arity=3,
                                                  n_max_parts=40, use_clt=False)),
    'g24e1': ('expc', (2000, 24, 4, 0.2, 7), dict(ensemble_dim=4, det=True, sd_level=1, min_part_inst=64, conj_len=2, arity=3,
                                                  n_max_parts=40)),
    'g24e2': ('expc', (2000, 24, 4, 0.2, 7), dict(ensemble_dim=4, det=False, sd_level=2, min_part_inst=32, conj_len=3, arity=4,
                                                  n_max_parts=40)),
}
_cache = {}


# ---- fixtures --------------------------------------------------------------------------------------------------------------
def golden(name):
    """tests/golden/xpc_<name>.npz as a dict with ``x`` (training rows) and ``fresh`` unpacked; loaded once."""
    if name not in _cache:
        f = np.load(os.path.join(GOLDEN, 'xpc_%s.npz' % name))
        g = {k: f[k] for k in f.files}
        g['x'] = clt_ref.unpack(g['data'], int(g['n_rows']), int(g['n_vars']))
        g['fresh'] = clt_ref.unpack(g['fresh_bits'], N_FRESH, int(g['n_vars']))
        _cache[name] = g
    return _cache[name]


def queries(fresh, n=256, share=0.4, seed=5):
    """Query rows with ``share`` of the entries NaN: row 0 all NaN, row 1 complete, then fresh rows."""
    rs = np.random.RandomState(seed)
    q = np.array(fresh[:n], np.float32)
    mask = rs.rand(*q.shape) < share
    mask[0] = True
    mask[1] = False
    q[mask] = np.nan
    return q


def restated(name):
    """The restatement's model of a configuration's data; computed once."""
    key = ('model', name)
    if key not in _cache:
        learner, _, kw = CONFIGS[name]
        _cache[key] = learn(learner, golden(name)['x'], kw)
    return _cache[key]


def learn(learner, data, kw):
    if learner == 'xpc':
        return learn_xpc(data, **kw)
    np.random.seed(GLOBAL_SEED)
    return learn_expc(data, **kw)


# ---- the partition tree ------------------------------------------------------------------------------------------------------
def _part(rows, cols, uncond, parent=None, naive=False, conj=False):
    node = dict(rows=np.asarray(rows, np.int64), cols=[int(c) for c in cols], uncond=[int(c) for c in uncond], subs=[],
                naive=naive, conj=conj, disc=None, leaf=None)
    if parent is not None:
        parent['subs'].append(node)
    return node


def _horizontal(data, node, min_part_inst, conj_len, arity, sd, rs):
    """None (no split; nothing drawn when the partition is too small), or (conjunction, [rows of the discarded, rows of
    every chosen assignment ...])."""
    rows = node['rows']
    if len(node['uncond']) < conj_len or len(rows) < 2 * min_part_inst:
        return None
    order = list(node['uncond'])
    if not sd:
        rs.shuffle(order)
    conj = order[:conj_len]
    assignments = [list(a) for a in itertools.product([0, 1], repeat=conj_len)]
    rs.shuffle(assignments)
    block = data[rows][:, conj]
    left, groups = rows, []
    for a in assignments:
        hit = rows[(block == np.asarray(a)).all(axis=1)]
        if len(hit) < min_part_inst:
            continue
        if len(hit) == len(rows):
            return conj, [rows]
        if len(left) - len(hit) >= min_part_inst:
            left = np.setdiff1d(left, hit)
            groups.append(hit)
            if len(groups) == arity - 1 or len(left) < 2 * min_part_inst:
                break
    return (conj, [left] + groups) if groups else None


def partitioning(data, min_part_inst, n_max_parts, conj_len, arity, sd, ordering, rs):
    """``(root, leaf partitions for Chow-Liu trees, the conjunctions in order of first use, number of partitions)``."""
    root = _part(np.arange(len(data)), ordering, ordering)
    n_parts, conj_l, cl_parts, leaves = 0, [], [], [root]
    while leaves and n_parts + len(leaves) < n_max_parts:
        node = leaves.pop(rs.randint(len(leaves)))
        split = _horizontal(data, node, min_part_inst, conj_len, arity, sd, rs)
        if split is None:
            n_parts += 1
            cl_parts.append(node)
            continue
        conj, groups = split
        if conj not in conj_l:
            conj_l.append(conj)
        rest = [v for v in node['uncond'] if v not in conj]
        under = [c for c in node['cols'] if c in conj]               # in the order of the partition's columns
        free = set(itertools.product([0, 1], repeat=conj_len))
        first_naive = None
        for k, rows in enumerate(groups):
            sub = _part(rows, node['cols'], rest, node)
            if not rest:                                             # nothing but the conjunction: no vertical split
                leaves.append(sub)
                continue
            n_parts += 1
            naive = _part(rows, under, [], sub, naive=True, conj=k > 0)
            if k == 0:
                first_naive = naive
            else:
                free.remove(tuple(int(v) for v in data[rows[0]][under]))
            leaves.append(_part(rows, rest, rest, sub))
        if first_naive is not None:
            first_naive['disc'] = sorted(free)
    return root, cl_parts + leaves, conj_l, n_parts + len(leaves)


def preorder(root):
    out, stack = [], [root]
    while stack:
        node = stack.pop()
        out.append(node)
        stack.extend(node['subs'][::-1])
    return out


# ---- orderings and trees -------------------------------------------------------------------------------------------------------
def _mutual_information(part, alpha):
    return clt_ref.mutual_information(*clt_ref.priors_joints(clt_ref.counts(part), len(part), alpha))


def greedy_ordering(data, conj_len, alpha=0.01):
    mi = _mutual_information(data, alpha)
    total = mi.sum(axis=0)
    order, left = [], list(range(data.shape[1]))
    while left:
        head = left[int(np.argmax(total[left]))]
        left.remove(head)
        order.append(head)
        if len(left) > conj_len - 1:
            near = [left[i] for i in np.argpartition(-mi[head][left], conj_len - 1)[:conj_len - 1]]
        else:
            near = list(left)
        order += near
        left = list(set(left) - set(near))          # (a Python set's order, as in the reference)
    return order


def cumulative_information(data, cl_parts_l, alpha):
    """The float32 mutual information of every leaf partition's slice, summed in float64 over the partitions in order."""
    d = data.shape[1]
    info = np.zeros((d, d))
    for cl_parts in cl_parts_l:
        for node in cl_parts:
            cols = np.asarray(node['cols'])
            info[cols[:, None], cols] += _mutual_information(data[node['rows']][:, cols], alpha)
    return info


def trees_dict(data, cl_parts_l, conj_l, alpha, rs):
    d = data.shape[1]
    info = cumulative_information(data, cl_parts_l, alpha)
    free = list(set(np.arange(d)) - set(v for conj in conj_l for v in conj))        # (a Python set's order, as above)
    scopes = conj_l + [free] if free else conj_l
    trees = []
    for scope in scopes:
        root = scope.index(rs.choice(scope))
        trees.append([int(t) for t in clt_ref.prim(root, info[scope][:, scope])])
    out, tree, scope = {}, list(trees[-1]), [int(v) for v in scopes[-1]]
    for k in range(len(trees) - 2, -1, -1):
        out[len(scope)] = (list(tree), list(scope))
        upper = [t + len(scope) if t >= 0 else -1 for t in trees[k]]
        tree[tree.index(-1)] = len(scope) + upper.index(-1)
        tree, scope = tree + upper, scope + [int(v) for v in scopes[k]]
    return out


# ---- leaves ----------------------------------------------------------------------------------------------------------------------
def _leaf(data, node, use_clt, trees, det, alpha, leaf_rs):
    part = data[node['rows']][:, node['cols']]
    n = len(part)
    if node['conj']:
        return ('conj', [int(v) for v in part[0]])
    if node['naive'] or not use_clt:
        if not det or len(node['disc']) == 2 ** len(node['cols']):
            return ('naive', (part.astype(np.float64).sum(axis=0) + alpha) / (n + 2 * alpha))
        counts = np.array([(part == np.asarray(a)).all(axis=1).sum() for a in node['disc']], np.float64)
        return ('disj', (counts + alpha) / (counts + alpha).sum(), [list(a) for a in node['disc']])
    if trees is not None:
        tree, scope = trees[len(node['cols'])]
        tree = np.asarray(tree, np.int32)
    else:
        tree, scope = None, list(node['cols'])
        root = int(leaf_rs.choice(len(scope)))
    part = data[node['rows']][:, scope]
    priors, joints = clt_ref.priors_joints(clt_ref.counts(part), n, 0.01)
    if tree is None:
        tree = clt_ref.prim(root, clt_ref.mutual_information(priors, joints))
    bfs = clt_ref.bfs_order(tree)
    return ('clt', scope, bfs, tree, clt_ref.cpts(bfs, tree, priors, joints))


def _build(data, root, use_clt, trees, det, alpha, leaf_rs):
    """Leaves in the order the circuit is built: depth first, sub-partitions in order."""
    for node in preorder(root):
        if not node['subs']:
            node['leaf'] = _leaf(data, node, use_clt, trees, det, alpha, leaf_rs)


# ---- the learners ------------------------------------------------------------------------------------------------------------------
def learn_xpc(data, det, sd, min_part_inst, conj_len, arity, n_max_parts=200, use_clt=True, use_greedy_ordering=False,
              alpha=0.01, random_seed=42):
    data = np.asarray(data)
    rs, leaf_rs = np.random.RandomState(random_seed), np.random.RandomState(random_seed)
    if use_greedy_ordering:
        ordering = greedy_ordering(data, conj_len)
    else:
        ordering = np.arange(data.shape[1]).tolist()
        rs.shuffle(ordering)
    root, cl_parts, conj_l, n_parts = partitioning(data, min_part_inst, n_max_parts, conj_len, arity, sd, ordering, rs)
    assert n_parts > 1
    trees = trees_dict(data, [cl_parts], conj_l, alpha, rs) if sd and use_clt else None
    _build(data, root, use_clt, trees, det, alpha, leaf_rs)
    return dict(members=[dict(root=root, cl_parts=cl_parts, conj_vars_l=conj_l, n_parts=n_parts, trees_dict=trees)])


def learn_expc(data, ensemble_dim, det, sd_level, min_part_inst, conj_len, arity, n_max_parts=200, use_clt=True, alpha=0.01,
               random_seed=42):
    """The members' orderings are shuffled with the GLOBAL numpy generator (np.random.seed first)."""
    data = np.asarray(data)
    rs, leaf_rs = np.random.RandomState(random_seed), np.random.RandomState(random_seed)
    sd = sd_level in (SD_LEVEL_1, SD_LEVEL_2)
    ordering = greedy_ordering(data, conj_len) if sd_level == SD_LEVEL_2 else np.arange(data.shape[1]).tolist()
    members = []
    for _ in range(ensemble_dim):
        if sd_level != SD_LEVEL_2:
            np.random.shuffle(ordering)
        root, cl_parts, conj_l, n_parts = partitioning(data, min_part_inst, n_max_parts, conj_len, arity, sd, list(ordering), rs)
        members.append(dict(root=root, cl_parts=cl_parts, conj_vars_l=conj_l, n_parts=n_parts, trees_dict=None))
    if sd_level == SD_LEVEL_2 and use_clt:
        shared = trees_dict(data, [m['cl_parts'] for m in members], max([m['conj_vars_l'] for m in members], key=len), alpha, rs)
        for m in members:
            m['trees_dict'] = shared
    for m in members:
        if sd_level == SD_LEVEL_1 and use_clt:
            m['trees_dict'] = trees_dict(data, [m['cl_parts']], m['conj_vars_l'], alpha, rs)
        _build(data, m['root'], use_clt, m['trees_dict'], det, alpha, leaf_rs)
    return dict(members=members)


# ---- evaluation ------------------------------------------------------------------------------------------------------------------
def _logsumexp(terms):
    """float64 ``[B]`` of a list of ``[B]`` arrays; -inf where every term is."""
    stack = np.stack(terms)
    top = stack.max(axis=0)
    safe = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(divide='ignore'):
        return np.where(np.isfinite(top), safe + np.log(np.exp(stack - safe).sum(axis=0)), -np.inf)


def _indicators(x, cols, values):
    """Sum over ``cols`` of log [x_c = value_c], NaN marginalised."""
    block = x[:, cols]
    clash = (~np.isnan(block)) & (block != np.asarray(values, np.float64))
    return np.where(clash.any(axis=1), -np.inf, 0.0)


def _value(node, x):
    if node['subs']:
        kids = [_value(sub, x) for sub in node['subs']]
        if len(node['rows']) > len(node['subs'][0]['rows']):
            return _logsumexp([np.log(len(sub['rows']) / len(node['rows'])) + v for sub, v in zip(node['subs'], kids)])
        return np.sum(kids, axis=0)
    leaf = node['leaf']
    if leaf[0] == 'conj':
        return _indicators(x, node['cols'], leaf[1])
    if leaf[0] == 'naive':
        block, p = x[:, node['cols']], np.asarray(leaf[1], np.float64)
        terms = np.where(np.isnan(block), 0.0, np.where(block == 1, np.log(p), np.log1p(-p)))
        return terms.sum(axis=1)
    if leaf[0] == 'disj':
        return _logsumexp([np.log(w) + _indicators(x, node['cols'], a) for w, a in zip(leaf[1], leaf[2])])
    _, scope, bfs, tree, params = leaf
    return clt_ref.log_likelihood(bfs, tree, params, x[:, scope].astype(np.float32)).astype(np.float64)


def log_likelihood(model, x):
    """float64 ``[B]``; NaN = marginalised.  An ensemble is the uniform mixture of its members."""
    x = np.asarray(x, np.float64)
    values = [_value(m['root'], x) for m in model['members']]
    if len(values) == 1:
        return values[0]
    return _logsumexp([np.log(1.0 / len(values)) + v for v in values])


# ---- what the fixtures hold and the tests compare --------------------------------------------------------------------------------
def tree_record(root, n_rows):
    """The partition tree in pre-order: ``(row masks [P, ceil(n_rows / 8)] uint8, cols and their offsets, flags [P, 2],
    disc assignments and their offsets)``."""
    nodes = preorder(root)
    masks = np.zeros((len(nodes), n_rows), bool)
    for i, node in enumerate(nodes):
        masks[i, node['rows']] = True
    cols = [list(node['cols']) for node in nodes]
    disc = [[] if node['disc'] is None else [v for a in node['disc'] for v in a] for node in nodes]
    return dict(masks=np.packbits(masks, axis=1),
                cols=np.array([c for l in cols for c in l], np.int32),
                col_off=np.concatenate([[0], np.cumsum([len(l) for l in cols])]).astype(np.int32),
                flags=np.array([[node['naive'], node['conj']] for node in nodes], np.uint8),
                n_subs=np.array([len(node['subs']) for node in nodes], np.int32),
                disc=np.array([v for l in disc for v in l], np.int8),
                disc_off=np.concatenate([[0], np.cumsum([len(l) for l in disc])]).astype(np.int32),
                has_disc=np.array([node['disc'] is not None for node in nodes], np.uint8))


def same_tree(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


def trees_record(trees):
    """``trees_dict`` as ``(keys, predecessors and scopes concatenated, offsets)``; empty arrays for None."""
    keys = sorted(trees) if trees else []
    return dict(keys=np.array(keys, np.int32),
                tree=np.array([t for k in keys for t in trees[k][0]], np.int32),
                scope=np.array([v for k in keys for v in trees[k][1]], np.int32),
                off=np.concatenate([[0], np.cumsum([k for k in keys])]).astype(np.int32),
                given=np.array([trees is not None], np.uint8))


def segments(trees):
    """The trees a ``trees_dict`` is chained from, bottom first: ``[(scope, predecessors within the scope)]`` from its
    LARGEST entry (every smaller entry is a prefix of it) -- the root of a segment hangs under the previous segment's root
    and is given -1 here."""
    if not trees:
        return []
    keys = sorted(trees)
    tree, scope = trees[keys[-1]]
    out, lo = [], 0
    for hi in keys:
        out.append(([int(v) for v in scope[lo:hi]], [int(t) - lo if lo <= t < hi else -1 for t in tree[lo:hi]]))
        lo = hi
    return out


def golden_trees(g, m):
    """``trees_dict`` of member ``m`` of a fixture: ``{scope length: (predecessors, scope)}`` or None."""
    if not int(g['m%d_given' % m][0]):
        return None
    keys, off = g['m%d_keys' % m], g['m%d_off' % m]
    return {int(k): (g['m%d_tree' % m][off[i]:off[i + 1]].tolist(), g['m%d_scope' % m][off[i]:off[i + 1]].tolist())
            for i, k in enumerate(keys)}


def _edges(tree):
    return sorted((min(i, p), max(i, p)) for i, p in enumerate(tree) if p >= 0)


def assert_trees(name, m, trees):
    """``trees``: the ``trees_dict`` of member ``m`` of a model of the fixture ``name``.  Its keys, the scopes and the roots
    of the trees it is chained from are the reference's (the roots are drawn, the scopes follow the conjunctions).  A tree
    that is the only maximum spanning tree of the cumulative information (``tree_unique``, tools/gen_golden_xpc.py) has the
    reference's edges; elsewhere it must be one of the maximum spanning trees: its sorted edge weights are the
    reference's within 2^-23, the rule and the tolerance of ``cnet_ref.assert_leaf_trees``."""
    g = golden(name)
    want = golden_trees(g, m)
    if want is None:
        assert trees is None
        return
    assert sorted(trees) == sorted(want)
    trees = {k: ([int(t) for t in v[0]], [int(s) for s in v[1]]) for k, v in trees.items()}
    for k in want:                                   # the chain itself: every entry is a prefix of the next
        assert trees[k][1] == want[k][1] and len(trees[k][0]) == k
    got_s, want_s = segments(trees), segments(want)
    learner, _, kw = CONFIGS[name]
    model = restated(name)
    members = model['members'] if learner == 'expc' and kw['sd_level'] == SD_LEVEL_2 else [model['members'][m]]
    info = cumulative_information(g['x'], [x['cl_parts'] for x in members], kw.get('alpha', 0.01))
    for i, ((scope, tree), (ref_scope, ref_tree)) in enumerate(zip(got_s, want_s)):
        assert scope == ref_scope and tree.index(-1) == ref_tree.index(-1), i
        if g['m%d_tree_unique' % m][i]:
            assert _edges(tree) == _edges(ref_tree), i
        else:
            w = info[scope][:, scope]
            a = np.sort([w[e] for e in _edges(tree)])
            b = np.sort([w[e] for e in _edges(ref_tree)])
            assert a.shape == b.shape and (len(a) == 0 or np.max(np.abs(a - b)) <= 2.0 ** -23), i
    # the chained predecessors of every entry follow from its segments
    for k, (tree, scope) in trees.items():
        lo, roots = 0, []
        for seg_scope, seg_tree in got_s:
            if lo >= k:
                break
            hi = lo + len(seg_scope)
            roots.append(lo + seg_tree.index(-1))
            for j, t in enumerate(seg_tree):
                if t >= 0:
                    assert tree[lo + j] == lo + t
            lo = hi
        for below, above in zip(roots, roots[1:]):
            assert tree[below] == above
        assert tree[roots[-1]] == -1
