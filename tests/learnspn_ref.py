"""A numpy float64 restatement of LearnSPN for discrete data (reference deeprob/spn/learning/learnspn.py:121-222 with
splitting/gvs.py, splitting/random.py, learning/leaf.py and algorithms/structure.py:prune), in the manner of
tests/flat_spn_query_ref.py: plain loops over the reference's FIFO task queue, one task at a time, on data slices.
The HIP path batches a generation of tasks; this file does not, and the two must give the same graph.

The graph is the reference's node-link dict (structure/io.py:133-177) so that it compares with the golden JSON files.

K-means is this project's own definition, restated here operation by operation: float64, features in
column order (a column with K <= 2 is one feature, a column with K > 2 is K one-hot features), squared distances
accumulated feature by feature, ties to the lower cluster, centroids = exact counts / size, an emptied cluster keeps its
centroid, 5 restarts seeded by ``random_state.choice(n_rows, n, replace=False)``, at most 100 assignment steps, the
inertia summed as 256 interleaved partial sums added in order, lowest inertia wins, the first on a tie.
"""
from collections import deque

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
RESTARTS, MAX_ITER = 5, 100


def mixture(ks, n_rows, seed, n_clusters=4, noise=0.2):
    """(rows, cluster of each row) of a mixture of ``n_clusters`` prototypes: a row copies its cluster's prototype and each
    entry is replaced by a uniform value of its domain with probability ``noise`` (tools/gen_golden_learnspn.py)."""
    rs = np.random.RandomState(seed)
    ks = np.asarray(ks)
    protos = np.stack([rs.randint(0, ks) for _ in range(n_clusters)])
    z = rs.randint(0, n_clusters, size=n_rows)
    flip = rs.rand(n_rows, len(ks)) < noise
    x = np.where(flip, rs.randint(0, ks, size=(n_rows, len(ks))), protos[z])
    return x.astype(np.uint8), z


# ---- the G statistic, float64, in the order of operations include/deeprob_learn.h states -----------------------------
def joint_counts(xi, xj, ki, kj):
    return np.bincount(xi.astype(np.int64) * kj + xj.astype(np.int64), minlength=ki * kj).reshape(ki, kj)


def g_value(joint, n):
    h = joint.astype(np.float64) + EPS32
    m1 = np.cumsum(h, axis=1)[:, -1]          # sequential sums
    m2 = np.cumsum(h, axis=0)[-1, :]
    e = (m1[:, None] * m2[None, :]) / float(n)
    t = h * np.log(h / e)
    return 2.0 * float(np.cumsum(t.reshape(-1))[-1])


def gvs_component(data, ks, start, p):
    nf = data.shape[1]
    adjacent = np.zeros((nf, nf), bool)
    for a in range(nf):
        for b in range(a + 1, nf):
            g = g_value(joint_counts(data[:, a], data[:, b], ks[a], ks[b]), len(data))
            adjacent[a, b] = adjacent[b, a] = not (g < 2.0 * (ks[a] - 1) * (ks[b] - 1) * p)
    seen, queue = {start}, deque([start])
    while queue:
        f = queue.popleft()
        for o in np.flatnonzero(adjacent[f]):
            if int(o) not in seen:
                seen.add(int(o))
                queue.append(int(o))
    part = np.zeros(nf, np.int64)
    part[sorted(seen)] = 1
    return part


def gvs_cols(data, ks, rs, p=5.0):
    return gvs_component(data, ks, rs.randint(0, data.shape[1]), p)


def rgvs_cols(data, ks, rs, p=5.0):
    nf = data.shape[1]
    k = int(max(np.sqrt(nf), 2))
    if k == nf:
        return gvs_cols(data, ks, rs, p)
    perm = rs.permutation(np.arange(nf))[:k]
    part = gvs_cols(data[:, perm], [ks[e] for e in perm], rs, p)
    clusters = np.zeros(nf, np.int64) if rs.rand() < 0.5 else np.ones(nf, np.int64)
    clusters[perm] = part
    return clusters


# ---- k-means ---------------------------------------------------------------------------------------------------------
def sq_dist(data, ks, cen):
    """[n] squared distances of the rows to ONE centroid ``cen`` ([ncols, kmax] value frequencies)."""
    d = np.zeros(len(data), np.float64)
    for p in range(data.shape[1]):
        v = data[:, p]
        if ks[p] <= 2:
            u = v.astype(np.float64) - cen[p, 1]
            d = d + u * u
        else:
            for k in range(ks[p]):
                u = (v == k).astype(np.float64) - cen[p, k]
                d = d + u * u
    return d


def inertia_sum(d):
    pad = (-len(d)) % 256
    rows = np.concatenate([d, np.zeros(pad)]).reshape(-1, 256)
    part = rows[0].copy()
    for r in rows[1:]:
        part = part + r
    total = part[0]
    for v in part[1:]:
        total = total + v
    return float(total)


def kmeans_restart(data, ks, seed, n):
    """One restart from the rows ``seed``: (labels, inertia, sizes, smallest relative gap between a row's two nearest
    centroids over all its assignment steps)."""
    data = np.asarray(data).astype(np.int64)
    nrows, ncols = data.shape
    kmax = max(2, max(ks))
    cen = np.zeros((n, ncols, kmax))
    for c in range(n):
        for p in range(ncols):
            cen[c, p, data[seed[c], p]] = 1.0
    labels, gap = None, np.inf
    for it in range(MAX_ITER):
        dist = np.stack([sq_dist(data, ks, cen[c]) for c in range(n)], axis=1)
        new = np.argmin(dist, axis=1)                    # (the first minimum: ties to the lower index)
        if n > 1:
            two = np.sort(dist, axis=1)[:, :2]
            gap = min(gap, float(np.min((two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300))))
        same = labels is not None and np.array_equal(new, labels)
        labels = new
        if same or it == MAX_ITER - 1:
            break
        for c in range(n):
            rows = data[labels == c]
            if len(rows) == 0:
                continue
            for p in range(ncols):
                cen[c, p, :] = np.bincount(rows[:, p], minlength=kmax).astype(np.float64) / float(len(rows))
    own = np.zeros(nrows)
    for c in range(n):
        own[labels == c] = sq_dist(data[labels == c], ks, cen[c])
    return labels, inertia_sum(own), np.bincount(labels, minlength=n), gap


def kmeans(data, ks, rs, n=2, stats=None):
    """Labels of the winning restart.  ``stats['gap']``: the smallest relative gap between a row's two nearest centroids
    over all assignments of winning restarts."""
    seeds = [rs.choice(len(data), n, replace=False) for _ in range(RESTARTS)]
    best = None
    for seed in seeds:
        run = kmeans_restart(data, ks, seed, n)
        if best is None or run[1] < best[1]:
            best = run
    if stats is not None:
        stats['gap'] = min(stats.get('gap', np.inf), best[3])
    return best[0]


# ---- a k-means case without distance ties, for the device test of the k-means entries alone -------------------------------
KMEANS_CASE_KS = [2, 2, 5, 3, 2]
KMEANS_CASE_RESTARTS = 2
#: n_clusters -> (rows, columns) of the three tasks of the generation: two 256-row blocks with a ragged second one,
#: exactly one block, and a few rows; the column subsets differ and each holds a binary and a wider column
KMEANS_CASE_TASKS = {c: [(300, [3, 0, 4, 2, 1]), (256, [2, 3, 1, 0]), (5 if c <= 5 else 8, [4, 2, 3])] for c in (1, 2, 8)}
KMEANS_CASE_SEEDS = list(range(16))      # the table: per task, the first seed whose restated gap is >= 1e-6 is the fixture
_kmeans_cases = {}


def kmeans_case_task(n, cols, n_clusters, seed):
    """(rows [n, 5] uint8, seeds [restarts, n_clusters] row positions) of one task, or None.  Discrete rows tie between
    one-hot seeds, so the rows are picked: the seeds of the two restarts are rows of distinct values none of which is as
    near to two seeds of the other restart, and the other rows are drawn from a mixture and kept if their nearest seed is
    unique in both restarts.  That settles the first assignment step only; the caller checks the restated gap."""
    rs, ks = np.random.RandomState(seed), np.asarray(KMEANS_CASE_KS)[cols]
    pool, _ = mixture(KMEANS_CASE_KS, 4000, seed, n_clusters=max(3, n_clusters), noise=0.3)
    cost = np.where(ks <= 2, 1, 2)

    def tied(rows, seed_rows):
        d = np.sort(((pool[rows][:, None, cols] != pool[seed_rows][None, :, cols]) * cost).sum(2), axis=1)
        return d[:, 0] == d[:, 1] if n_clusters > 1 else np.zeros(len(rows), bool)

    distinct = np.unique(pool[:, cols], axis=0, return_index=True)[1]
    if len(distinct) < 2 * n_clusters:
        return None
    for _ in range(4000):
        first, second = np.split(rs.permutation(distinct)[:2 * n_clusters], 2)
        if n == n_clusters:
            second = rs.permutation(first)
        if not tied(first, second).any() and not tied(second, first).any():
            break
    else:
        return None
    seed_rows = np.unique(np.concatenate([first, second]))
    others = np.setdiff1d(np.arange(len(pool)), seed_rows)
    others = others[~tied(others, first) & ~tied(others, second)][:n - len(seed_rows)]
    picked = rs.permutation(np.concatenate([seed_rows, others]))
    if len(picked) != n:
        return None
    position = {int(r): i for i, r in enumerate(picked)}
    return pool[picked], np.array([[position[int(r)] for r in restart] for restart in (first, second)])


def kmeans_case(n_clusters):
    """The fixture of one ``n_clusters``: ``(x uint8 [rows, 5], segments, tasks, want, gap)`` -- the matrix, the matrix rows
    of each task (disjoint, unsorted, scattered over the matrix), per task ``(n, columns, seeds)``, per task and restart
    ``kmeans_restart``'s result, and the smallest restated gap.  Built once; None if the seed table gives no such case."""
    if n_clusters not in _kmeans_cases:
        blocks, tasks, want = [], [], []
        for n, cols in KMEANS_CASE_TASKS[n_clusters]:
            for seed in KMEANS_CASE_SEEDS:
                made = kmeans_case_task(n, cols, n_clusters, seed)
                if made is None:
                    continue
                runs = [kmeans_restart(made[0][:, cols], [KMEANS_CASE_KS[c] for c in cols], s, n_clusters) for s in made[1]]
                if min(run[3] for run in runs) >= 1e-6:
                    break
            else:
                _kmeans_cases[n_clusters] = None
                return None
            blocks.append(made[0])
            tasks.append((n, cols, made[1]))
            want.append(runs)
        stacked = np.concatenate(blocks)
        where = np.random.RandomState(n_clusters).permutation(len(stacked))       # stacked row i is matrix row where[i]
        x = np.empty_like(stacked)
        x[where] = stacked
        offs = np.concatenate([[0], np.cumsum([len(b) for b in blocks])])
        segments = [where[offs[i]:offs[i + 1]] for i in range(len(blocks))]
        _kmeans_cases[n_clusters] = (x, segments, tasks, want, min(run[3] for runs in want for run in runs))
    return _kmeans_cases[n_clusters]


# ---- leaves and the graph ------------------------------------------------------------------------------------------------
def node(cls, scope, **kw):
    return dict({'class': cls, 'scope': list(scope), 'children': []}, **kw)


def mle_leaf(name, var, col, k, alpha):
    n = len(col)
    if name == 'Bernoulli':
        return node('Bernoulli', [var], params={'p': (float(np.sum(col == 1)) + alpha) / (n + 2 * alpha)})
    probs = [(float(np.sum(col == d)) + alpha) / (n + k * alpha) for d in range(k)]
    return node('Categorical', [var], params={'categories': list(range(k)), 'probabilities': probs})


def naive(names, ks, data, scope, alpha):
    out = node('Product', scope)
    for i, s in enumerate(scope):
        out['children'].append(mle_leaf(names[s], s, data[:, i], ks[s], alpha))
    return out


def learn_spn(data, names, ks, split_rows='kmeans', split_cols='gvs', min_rows_slice=256, min_cols_slice=2, random_state=None,
              alpha=0.1, p=5.0, a=2.0, b=2.0, n=2, stats=None):
    """The task loop; ``names[i]`` in ('Bernoulli', 'Categorical'), ``ks[i]`` the domain size.  Returns the root (dict form)."""
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    data = np.asarray(data).astype(np.int64)
    tmp = node('Product', range(data.shape[1]))
    tasks = deque([dict(parent=tmp, data=data, scope=list(range(data.shape[1])), ncs=False, nrs=False, first=True)])
    while tasks:
        t = tasks.popleft()
        d, scope = t['data'], t['scope']
        ns, nf = d.shape
        zero = np.array([np.all(d[:, i] == d[0, i]) for i in range(nf)])
        lks = [ks[s] for s in scope]
        if zero.all():
            t['parent']['children'].append(naive(names, ks, d, scope, alpha))
        elif zero.any():
            nd = node('Product', scope)
            nd['children'].append(naive(names, ks, d[:, zero], [scope[i] for i in np.flatnonzero(zero)], alpha))
            first = t['first'] and len(tasks) == 0
            tasks.append(dict(parent=nd, data=d[:, ~zero], scope=[scope[i] for i in np.flatnonzero(~zero)], ncs=False, nrs=False,
                              first=first))
            t['parent']['children'].append(nd)
        elif t['nrs'] or nf < min_cols_slice or ns < min_rows_slice:
            if nf == 1:
                t['parent']['children'].append(mle_leaf(names[scope[0]], scope[0], d[:, 0], ks[scope[0]], alpha))
            else:
                t['parent']['children'].append(naive(names, ks, d, scope, alpha))
        elif t['ncs'] or t['first']:
            if split_rows == 'random':
                q = rs.beta(a, b)
                clusters = rs.binomial(1, q, size=ns)
            else:
                clusters = kmeans(d, lks, rs, n, stats)
            present = np.unique(clusters)
            if len(present) == 1:
                tasks.append(dict(parent=t['parent'], data=d, scope=scope, ncs=False, nrs=True, first=False))
                continue
            nd = node('Sum', scope, weights=[float(np.sum(clusters == c)) / ns for c in present])
            for c in present:
                tasks.append(dict(parent=nd, data=d[clusters == c], scope=scope, ncs=False, nrs=False, first=False))
            t['parent']['children'].append(nd)
        else:
            if split_cols == 'random':
                q = rs.beta(a, b)
                clusters = rs.binomial(1, q, size=nf)
            elif split_cols == 'gvs':
                clusters = gvs_cols(d, lks, rs, p)
            else:
                clusters = rgvs_cols(d, lks, rs, p)
            present = np.unique(clusters)
            if len(present) == 1:
                tasks.append(dict(parent=t['parent'], data=d, scope=scope, ncs=True, nrs=False, first=False))
                continue
            nd = node('Product', scope)
            for c in present:
                tasks.append(dict(parent=nd, data=d[:, clusters == c], scope=[scope[i] for i in np.flatnonzero(clusters == c)],
                                  ncs=False, nrs=False, first=False))
            t['parent']['children'].append(nd)
    return tmp['children'][0]


def topological_order(root):
    """Kahn's algorithm as structure/node.py:212-246 runs it."""
    outgoing, seen, queue = {id(root): 0}, {id(root)}, deque([root])
    while queue:
        nd = queue.popleft()
        for c in nd['children']:
            outgoing[id(c)] = outgoing.get(id(c), 0) + 1
            if id(c) not in seen:
                seen.add(id(c))
                queue.append(c)
    order, queue = [], deque([root])
    while queue:
        nd = queue.popleft()
        order.append(nd)
        for c in nd['children']:
            outgoing[id(c)] -= 1
            if outgoing[id(c)] == 0:
                queue.append(c)
    assert sum(outgoing.values()) == 0
    return order


def prune(root):
    """algorithms/structure.py:33-77 on the dict form (modifies the nodes, returns the new root)."""
    nodes = topological_order(root)
    mapped = {id(x): x for x in nodes}
    for nd in reversed(nodes):
        if nd['class'] not in ('Sum', 'Product'):
            continue
        kids = [mapped[id(c)] for c in nd['children']]
        if len(kids) == 1:
            mapped[id(nd)] = kids[0]
        elif nd['class'] == 'Product':
            children = []
            for ch in kids:
                children += [mapped[id(c)] for c in ch['children']] if ch['class'] == 'Product' else [ch]
            nd['children'] = children
        else:
            order, weight = [], {}
            for i, ch in enumerate(kids):
                pairs = [(mapped[id(c)], nd['weights'][i] * ch['weights'][j]) for j, c in enumerate(ch['children'])] \
                    if ch['class'] == 'Sum' else [(ch, nd['weights'][i])]
                for sub, w in pairs:
                    if id(sub) not in weight:
                        order.append(sub)
                        weight[id(sub)] = 0.0
                    weight[id(sub)] += w
            nd['children'] = order
            nd['weights'] = [weight[id(c)] for c in order]
    return mapped[id(root)]


def to_digraph(root):
    """The node-link dict of structure/io.py:133-177 (ids in assign_ids order; floats are NOT rounded here)."""
    order = topological_order(root)
    ids = {id(x): i for i, x in enumerate(order)}
    nodes, links = [], []
    for i, nd in enumerate(order):
        rec = {'class': nd['class'], 'scope': list(nd['scope']), 'id': i}
        if nd['class'] == 'Sum':
            rec['weights'] = [float(w) for w in nd['weights']]
        if 'params' in nd:
            rec['params'] = nd['params']
        nodes.append(rec)
        for k, c in enumerate(nd['children']):
            links.append({'idx': k, 'source': ids[id(c)], 'target': i})
    return {'nodes': nodes, 'links': links}


def from_digraph(g):
    """The dict form of a node-link dict (a golden JSON file); returns the root (id 0)."""
    nodes = {int(r['id']): dict({k: v for k, v in r.items() if k != 'id'}, children=[]) for r in g['nodes']}
    slots = {i: {} for i in nodes}
    for e in g['links'] if 'links' in g else g['edges']:
        slots[int(e['target'])][int(e['idx'])] = nodes[int(e['source'])]
    for i, s in slots.items():
        nodes[i]['children'] = [s[k] for k in range(len(s))]
    return nodes[0]


def graphs_differ(got, want, atol=1e-6):
    """None when two node-link dicts are the same graph -- same nodes, classes, scopes, edges, floats within ``atol`` --
    else a description of the first difference."""
    gn = {int(r['id']): r for r in got['nodes']}
    wn = {int(r['id']): r for r in want['nodes']}
    if sorted(gn) != sorted(wn):
        return 'node count {} != {}'.format(len(gn), len(wn))
    for i in sorted(wn):
        g, w = gn[i], wn[i]
        if g['class'] != w['class'] or [int(s) for s in g['scope']] != [int(s) for s in w['scope']]:
            return 'node {}: {} {} != {} {}'.format(i, g['class'], g['scope'], w['class'], w['scope'])
        if w['class'] == 'Sum':
            if len(g['weights']) != len(w['weights']) or np.max(np.abs(np.subtract(g['weights'], w['weights']))) > atol:
                return 'node {}: weights {} != {}'.format(i, g['weights'], w['weights'])
        for key, val in (w.get('params') or {}).items():
            have = np.asarray(g['params'][key], np.float64)
            if have.shape != np.shape(val) or (have.size and np.max(np.abs(have - np.asarray(val, np.float64))) > atol):
                return 'node {}: {} {} != {}'.format(i, key, g['params'][key], val)

    def edges(d):
        return sorted((int(e['target']), int(e['idx']), int(e['source'])) for e in (d['links'] if 'links' in d else d['edges']))
    if edges(got) != edges(want):
        return 'edges differ'
    return None
