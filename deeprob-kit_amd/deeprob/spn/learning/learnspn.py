"""LearnSPN (reference deeprob/spn/learning/learnspn.py:41-222), with the statistics of every task on the HIP device and
the task queue, every random draw and the graph on the host.  Returns a :class:`deeprob.spn.structure.io.FlatSpn`.

The reference pops one task at a time from a FIFO queue.  The queue is breadth first, so the tasks of one GENERATION
(one depth of the task tree, a retry counting as a child) are consecutive in it and their children follow in the same
order; a generation is processed here as a whole: column statistics of all its tasks in one launch, the operations decided
from them, the draws of the ``RandomState`` made on the host in queue order (they need only sizes known by then), the
statistics of all column-splitting tasks, the co-occurrence counts of all Chow-Liu leaf tasks (``learn_leaf`` the function
``leaf.learn_binary_clt``), the k-means -- or, with ``split_rows`` the function ``splitting.cluster.gmm``, the
Gaussian-mixture EM (``hip.learn.GmmBatch``) -- of all row-splitting tasks together, and one partition
launch that writes the next generation's row-index array.  The loop is written once; what depends on the kind of the columns --
discrete (:class:`DiscreteColumns`, below) or Gaussian (``learnspn_cont.GaussianColumns``) -- is asked of a column-kind
object.  See DESIGN.md, "LearnSPN on the device".
"""
from collections import deque
from typing import List, Optional, Union

import numpy as np
import torch

from deeprob.hip import HipError, learn as L
from deeprob.spn.learning.splitting import rdc as R, hist as H, entropy as SE, gini as SG, gvs as SV, cluster as SC
from deeprob.spn.learning.leaf import learn_binary_clt, BERNOULLI_MESSAGE
from deeprob.spn.structure.leaf import LeafType, Bernoulli, Categorical

#: what ``get_learn_leaf_method`` / ``get_split_rows_method`` / ``get_split_cols_method`` of the reference know
#: (learning/leaf.py:31-37, splitting/rows.py:54-68, splitting/cols.py:58-76) and what is built here
KNOWN_LEAF, BUILT_LEAF = ('mle', 'isotonic', 'binary-clt'), ('mle',)
KNOWN_ROWS, BUILT_ROWS = ('kmeans', 'kmeans_mb', 'dbscan', 'wald', 'gmm', 'rdc', 'random'), ('kmeans', 'random')
KNOWN_COLS = ('gvs', 'rgvs', 'wrgvs', 'ebvs', 'ebvs_ae', 'gbvs', 'gbvs_ag', 'rdc', 'random')
BUILT_COLS = ('gvs', 'rgvs', 'random')
KMEANS_RESTARTS = 5
#: launches + host reads + uploads per generation, outside the Lloyd loop
LAUNCHES_PER_GENERATION = 14
#: what ``learn_leaf=learn_binary_clt`` adds to it: the table upload of ``pair_ones``, its zeroing and its counting kernel
#: and the read of the counts ("Chow-Liu tree leaves in learn_spn")
CLT_LAUNCHES_PER_GENERATION = 4

#: the column-split functions of this package that ``split_cols`` takes, recognised by identity, and the split of each
HIST_FUNCTIONS = ((SE.entropy_cols, H.ENTROPY), (SE.entropy_adaptive_cols, H.ENTROPY_ADAPTIVE), (SG.gini_cols, H.GINI),
                  (SG.gini_adaptive_cols, H.GINI_ADAPTIVE), (SV.gvs_cols, 'gvs'), (SV.rgvs_cols, 'rgvs'))

#: the row-split functions of this package that ``split_rows`` takes, recognised by identity, and the split of each
ROWS_FUNCTIONS = ((SC.gmm, 'gmm'), (SC.kmeans, 'kmeans'))

_last_info = {}


def rows_split(split_rows):
    """The split of one of ``ROWS_FUNCTIONS``, None for anything else (a string included)."""
    return next((split for fn, split in ROWS_FUNCTIONS if fn is split_rows), None)


def hist_split(split_cols):
    """The split of one of ``HIST_FUNCTIONS``, None for anything else (a string included)."""
    return next((split for fn, split in HIST_FUNCTIONS if fn is split_cols), None)


def last_info() -> dict:
    """What the last ``learn_spn`` recorded: ``generations``, ``tasks_per_generation``, ``kernels`` (launches of the learn
    library outside the Lloyd loop; ``torch.sort`` and the gathers in front of it are not counted), ``reads``, ``uploads``,
    ``launches`` (the sum of the three), ``lloyd_launches`` and ``lloyd_iterations``; ``gmm_kernels``, ``gmm_reads``,
    ``gmm_uploads`` and ``gmm_iterations``: the launches, reads, uploads and iterations of the Gaussian-mixture EM, counted
    apart (not part of ``launches``; all zero without ``split_rows=gmm``); on discrete data also
    ``launches_per_generation``, the bound DESIGN.md derives for ``launches`` there (``LAUNCHES_PER_GENERATION``, plus
    ``CLT_LAUNCHES_PER_GENERATION`` with Chow-Liu leaves); and ``clt_leaves``: one record per Chow-Liu leaf in queue order,
    with its ``scope``, ``root`` (a variable), ``tree``, ``params``, ``n`` and ``rows`` -- the leaf's slice of its
    generation's row-index array, a device tensor (a view: nothing is read for it; it lives until the next ``learn_spn``)."""
    return dict(_last_info)


def _method(name, known, built, unknown_msg, what):
    if not isinstance(name, str):
        raise NotImplementedError("a custom {} function is not built on the HIP path (built: {})".format(what, ', '.join(built)))
    if name not in known:
        raise ValueError(unknown_msg.format(name))
    if name not in built:
        raise NotImplementedError("{} '{}' is not built on the HIP path (built: {})".format(what, name, ', '.join(built)))
    return name


def _kwargs(given, allowed, what):
    out = dict(allowed)
    for k, v in (given or {}).items():
        if k not in allowed:
            raise TypeError("{} got an unexpected keyword argument '{}'".format(what, k))
        out[k] = v
    return out


def check_random_state(random_state):
    """reference utils/random.py: None, a seed or a RandomState."""
    if random_state is None:
        return np.random.RandomState()
    if isinstance(random_state, (int, np.integer)):
        return np.random.RandomState(int(random_state))
    if isinstance(random_state, np.random.RandomState):
        return random_state
    raise ValueError("The random state must be either None, a seed integer or a Numpy RandomState")


def check_discrete(distributions, domains, who='learn_spn'):
    """Every distribution is Bernoulli or Categorical and every domain ``list(range(K))`` with ``K <= DPL_MAX_K``."""
    for dist in distributions:
        if getattr(dist, 'LEAF_TYPE', None) != LeafType.DISCRETE or dist not in (Bernoulli, Categorical):
            raise NotImplementedError("{} leaves are not built by {} on the HIP path (built: Bernoulli, Categorical)"
                                      .format(getattr(dist, '__name__', dist), who))
    for i, (dist, dom) in enumerate(zip(distributions, domains)):
        if not isinstance(dom, list) or len(dom) == 0 or [int(v) for v in dom] != list(range(len(dom))) \
                or any(v != int(v) for v in dom):
            raise ValueError("The domain of variable {} must be list(range(K)), got {}".format(i, dom))
        if len(dom) > L.DPL_MAX_K:
            raise ValueError("The domain of variable {} has {} values, at most {} are built".format(i, len(dom), L.DPL_MAX_K))
        if dist is Bernoulli and list(dom) != [0, 1]:
            raise ValueError("The domain of the Bernoulli variable {} must be [0, 1], got {}".format(i, dom))


def check_arguments(kind, data, distributions, domains, learn_leaf, split_rows, split_cols, learn_leaf_kwargs,
                    split_rows_kwargs, split_cols_kwargs, min_rows_slice, min_cols_slice):
    """The argument checks of ``learn_spn`` in the reference's order (learnspn.py:80-96), then what this path does not
    build for columns of ``kind``; returns ``(leaf kwargs, rows kwargs, cols kwargs)`` with the defaults filled in.
    Touches no device."""
    if len(distributions) == 0:
        raise ValueError("The list of distribution classes must be non-empty")
    if len(domains) == 0:
        raise ValueError("The list of domains must be non-empty")
    if min_rows_slice <= 0:
        raise ValueError("The minimum number of samples required to split horizontally must be positive")
    if min_cols_slice <= 0:
        raise ValueError("The minimum number of samples required to split vertically must be positive")
    if len(data.shape) != 2:
        raise ValueError("The data must be a matrix of samples by features")
    n_samples, n_features = data.shape
    if len(distributions) != n_features or len(domains) != n_features:
        raise ValueError("Each data column should correspond to a random variable having a distribution and a domain")
    clt = learn_leaf is learn_binary_clt      # (this package's own function, by identity; the string 'binary-clt' is not built)
    if not clt:
        _method(learn_leaf, KNOWN_LEAF, BUILT_LEAF, "Unknown learn leaf method called {}", 'learn_leaf')
    elif any(d is not Bernoulli for d in distributions):
        raise ValueError(BERNOULLI_MESSAGE)                                               # leaf.py:138-139
    rows_fn = rows_split(split_rows)         # (this package's gmm / kmeans functions, by identity; the string 'gmm' is not built)
    if rows_fn is None:
        _method(split_rows, KNOWN_ROWS, BUILT_ROWS, "Unknown split rows method called {}", 'split_rows')
    rdc = split_cols is R.rdc_cols           # (this package's own function, by identity; the string 'rdc' is not built)
    hist = hist_split(split_cols)            # (likewise the entropy, Gini and G-test functions)
    if not rdc:
        kind.check_split_cols(split_cols)
    if clt:
        leaf_kw = _kwargs(learn_leaf_kwargs, {'to_pc': False, 'alpha': 0.1, 'random_state': None}, 'learn_binary_clt')
        check_random_state(leaf_kw['random_state'])             # (the type; a RandomState is returned as it is, untouched)
    else:
        leaf_kw = _kwargs(learn_leaf_kwargs, {'alpha': 0.1}, 'learn_mle')
    clustered = rows_fn is not None or split_rows == 'kmeans'
    rows_kw = _kwargs(split_rows_kwargs, {'n': 2} if clustered else {'a': 2.0, 'b': 2.0}, rows_fn or split_rows)
    if rdc:
        cols_kw = _kwargs(split_cols_kwargs, {'d': R.D_DEFAULT, 'k': R.K_DEFAULT, 's': R.S_DEFAULT}, 'rdc_cols')
    elif hist is not None:
        cols_kw = _kwargs(split_cols_kwargs, H.DEFAULTS[hist], split_cols.__name__)
        if hist in H.MISSING_SIZE and cols_kw['size'] is None:
            raise ValueError(H.MISSING_SIZE[hist])                                        # entropy.py:73-74, gini.py:75-76
    else:
        cols_kw = _kwargs(split_cols_kwargs, {'a': 2.0, 'b': 2.0} if split_cols == 'random' else {'p': 5.0}, split_cols)
    if kind.smoothed_leaves and leaf_kw['alpha'] < 0.0:
        raise ValueError("The Laplace smoothing factor must be non-negative")
    if clustered and not 1 <= int(rows_kw['n']) <= L.DPL_MAX_CLUSTERS:
        raise ValueError("{} on the HIP path takes 1..{} clusters".format('gmm' if rows_fn == 'gmm' else 'k-means', L.DPL_MAX_CLUSTERS))
    kind.check_columns(cols_kw if rdc else None)
    return leaf_kw, rows_kw, cols_kw


def _to_device(data, ks):
    """The data as uint8 domain positions, column major, on the device (one upload); ValueError on NaN or on a value
    outside its domain; HipError for a CPU tensor."""
    if isinstance(data, torch.Tensor):
        if not data.is_cuda:
            raise HipError("data lives on '{}': the deeprob HIP path only works on tensors on a HIP device (there is no "
                           "CPU fallback); pass a numpy array or a device tensor".format(data.device))
        if data.is_floating_point() and bool(torch.isnan(data).any()):
            raise ValueError("The data contains NaN: learn_spn needs complete data")
        kt = torch.as_tensor(ks, device=data.device).to(data.dtype)
        if bool(((data < 0) | (data >= kt) | (data != data.round() if data.is_floating_point() else False)).any()):
            raise ValueError("The data holds values outside the domains")
        x = data.t().contiguous().to(torch.uint8)
    else:
        data = np.asarray(data)
        if np.issubdtype(data.dtype, np.floating) and np.isnan(data).any():
            raise ValueError("The data contains NaN: learn_spn needs complete data")
        if ((data < 0) | (data >= np.asarray(ks)[None, :]) | (data != np.round(data))).any():
            raise ValueError("The data holds values outside the domains")
        if not torch.cuda.is_available():
            raise HipError("learn_spn needs a HIP device (there is no CPU fallback)")
        x = torch.from_numpy(np.ascontiguousarray(data.T).astype(np.uint8)).cuda()
    return L.DeviceData(x.reshape(-1), data.shape[0], data.shape[1])


class _Task:
    __slots__ = ('parent', 'row_off', 'n', 'scope', 'no_cols_split', 'no_rows_split', 'is_first', 'op', 'counts', 'draw',
                 'child_src')

    def __init__(self, parent, n, scope, no_cols_split=False, no_rows_split=False, is_first=False):
        self.parent, self.n, self.scope = parent, n, scope
        self.no_cols_split, self.no_rows_split, self.is_first = no_cols_split, no_rows_split, is_first
        self.row_off = 0


def item_tables(tasks):
    """(column, row offset, rows) of every column of every task: the items of a launch over columns."""
    return ([s for t in tasks for s in t.scope], [t.row_off for t in tasks for _ in t.scope],
            [t.n for t in tasks for _ in t.scope])


def new_node(cls, scope, **kw):
    return dict({'class': cls, 'scope': list(scope), 'children': []}, **kw)


def naive_factorization(kind, scope, stats, n, alpha):
    node = new_node('Product', scope)
    for i, s in enumerate(scope):
        node['children'].append(kind.leaf(s, stats[i], n, alpha))
    return node


def topological_order(root):
    """Kahn's algorithm as the reference runs it (structure/node.py:212-246): the order ``assign_ids`` numbers in."""
    outgoing, seen, queue = {id(root): 0}, {id(root)}, deque([root])
    while queue:                                   # (bfs, node.py:175-189)
        node = queue.popleft()
        for c in node['children']:
            outgoing[id(c)] = outgoing.get(id(c), 0) + 1
            if id(c) not in seen:
                seen.add(id(c))
                queue.append(c)
    ordering, queue = [], deque([root])
    while queue:
        node = queue.popleft()
        ordering.append(node)
        for c in node['children']:
            outgoing[id(c)] -= 1
            if outgoing[id(c)] == 0:
                queue.append(c)
    if sum(outgoing.values()) != 0:
        raise ValueError("SPN structure is not a directed acyclic graph (DAG)")
    return ordering


def to_flat(root):
    """``assign_ids`` (node.py:156-172), then the flat circuit."""
    from deeprob.spn.structure.io import FlatSpn
    order = topological_order(root)
    ids = {id(n): i for i, n in enumerate(order)}
    nodes, children = {}, {}
    for i, n in enumerate(order):
        rec = {'class': n['class'], 'scope': list(n['scope'])}
        if n['class'] == 'Sum':
            rec['weights'] = [float(w) for w in np.asarray(n['weights'], np.float32)]
        if 'params' in n:
            rec['params'] = n['params']
        nodes[i] = rec
        children[i] = [ids[id(c)] for c in n['children']]
    return FlatSpn(nodes, children)


def component(adjacent, start):
    """The connected component of ``start``: what the greedy loop of gvs.py:31-50 collects, whatever order its sets
    iterate in."""
    seen, queue = {start}, deque([start])
    while queue:
        f = queue.popleft()
        for o in np.flatnonzero(adjacent[f]):
            if int(o) not in seen:
                seen.add(int(o))
                queue.append(int(o))
    return seen


def gvs_draws(random_state, nf, split_cols):
    """The draws of gvs (gvs.py:30) or rgvs (gvs.py:76, then :30 on the subset, then :89) on ``nf`` columns: (columns
    tested, start, coin)."""
    k = int(max(np.sqrt(nf), 2))
    if split_cols == 'gvs' or k == nf:
        return np.arange(nf), random_state.randint(0, nf), None
    perm = random_state.permutation(np.arange(nf))[:k]
    start = random_state.randint(0, k)
    return perm, start, random_state.rand()


def pair_clusters(tasks, split_cols, cols_kw, g_all, dof_all):
    """The clusters of every task from the statistics of the pairs a < b of its tested columns (``g_all``, with the
    degrees of freedom ``dof_all`` of a G-test), in task order."""
    out, g_pos = [], 0
    for t in tasks:
        (sub, start, coin), nf = t.draw, len(t.scope)
        k = len(sub)
        ia, ib = np.triu_indices(k, 1)
        g, dof = g_all[g_pos:g_pos + len(ia)], dof_all[g_pos:g_pos + len(ia)]
        g_pos += len(ia)
        if split_cols == 'rdc':
            dependent = g > cols_kw['d']                                              # rdc.py:43
        else:
            dependent = ~(g < 2.0 * dof * cols_kw['p'])                               # gvs.py:203-205, :42
        adjacent = np.zeros((k, k), bool)
        adjacent[ia, ib] = adjacent[ib, ia] = dependent
        if split_cols == 'rdc':
            clusters = R.components(adjacent)                                         # rdc.py:46-48
        else:
            part = np.zeros(k, np.int64)
            part[list(component(adjacent, int(start)))] = 1
            if coin is None:
                clusters = part
            else:
                clusters = np.zeros(nf, np.int64) if coin < 0.5 else np.ones(nf, np.int64)
                clusters[sub] = part
        out.append(clusters)
    return out


class DiscreteColumns:
    """What ``learn_spn`` asks of the kind of its columns, for ``Bernoulli`` / ``Categorical`` columns: the checks and the
    upload, the statistics of a generation's columns, the leaves, the column-split draws and clusters, the k-means batch."""

    launches_per_generation = LAUNCHES_PER_GENERATION
    smoothed_leaves = True                  # (alpha is used, so it is checked)

    def __init__(self, distributions, domains):
        self.distributions, self.domains = distributions, domains

    # ---- the checks of check_arguments that depend on the kind, in its order
    def check_split_cols(self, name):
        if hist_split(name) is None:
            _method(name, KNOWN_COLS, BUILT_COLS, "Unknown split rows method called {}", 'split_cols')   # (sic: cols.py:76)

    def check_columns(self, rdc_kw):
        check_discrete(self.distributions, self.domains)
        if rdc_kw is not None:
            R.check_parameters([len(dom) for dom in self.domains], **rdc_kw)

    def upload(self, data):
        L.load_library()
        self.ks = [len(d) for d in self.domains]
        self.kmax = max(2, max(self.ks))
        self.data = _to_device(data, self.ks)
        return self.data

    # ---- a generation
    def column_stats(self, row_index, item_col, item_off, item_n):
        """(the ``[kmax]`` counts, whether it is constant) of every item, from one launch and one read."""
        counts = L.read(L.column_counts(self.data, row_index, item_col, item_off, item_n, self.kmax))
        return counts, counts.max(axis=1) == np.asarray(item_n)         # a constant column: np.var == 0

    def leaf(self, var, counts, n, alpha):
        """learning/leaf.py:64-68 with structure/leaf.py:162 (Bernoulli) / :261-264 (Categorical) from the column's counts."""
        if self.distributions[var] is Bernoulli:
            return new_node('Bernoulli', [var], params={'p': (float(counts[1]) + alpha) / (n + 2 * alpha)})
        k = self.ks[var]
        probs = np.empty(k, np.float32)
        for i in range(k):
            probs[i] = (int(counts[i]) + alpha) / (n + k * alpha)
        return new_node('Categorical', [var], params={'categories': list(range(k)), 'probabilities': [float(q) for q in probs]})

    def draw_split_cols(self, random_state, t, split_cols, cols_kw):
        """The draws of a column split that is not 'random' (gvs.py:30, 76, 89; rdc.py:170-176): (columns tested, start,
        coin)."""
        nf = len(t.scope)
        if split_cols in H.STAT_SPLITS:
            return None                                 # (the entropy and Gini splits draw nothing)
        if split_cols == 'rdc':
            R.consume_draws(random_state, [self.ks[s] for s in t.scope], int(cols_kw['k']))
            return np.arange(nf), None, None
        return gvs_draws(random_state, nf, split_cols)

    def gtest_values(self, row_index, tasks):
        """``(g, dof)`` of the column pairs a < b of the tested columns of every task, in task order: one launch, one
        read."""
        return self.pair_values(row_index, tasks, L.pair_g)

    def split_cols_clusters(self, row_index, tasks, split_cols, cols_kw):
        """The column clusters of every gvs / rgvs / rdc task: the G statistics (or maximal correlations) of all their
        column pairs in one launch, then per task the adjacency and its component (gvs.py:31-50) or components.  The
        entropy and Gini splits come from the counts ``column_stats`` has read: no launch, no read, no upload."""
        if split_cols in H.STAT_SPLITS:
            return [H.stat_clusters(split_cols, cols_kw, [t.counts[i][:self.ks[s]] for i, s in enumerate(t.scope)], t.n, False)
                    for t in tasks]
        g_all, dof_all = self.pair_values(row_index, tasks, L.pair_maxcorr if split_cols == 'rdc' else L.pair_g)
        return pair_clusters(tasks, split_cols, cols_kw, g_all, dof_all)

    def pair_values(self, row_index, tasks, pair_stat):
        ks, ci, cj, off, n = np.asarray(self.ks), [], [], [], []
        for t in tasks:
            cols = np.asarray(t.scope)[t.draw[0]]
            ia, ib = np.triu_indices(len(cols), 1)          # the pairs a < b, in the order of two nested loops
            ci, cj = ci + list(cols[ia]), cj + list(cols[ib])
            off, n = off + [t.row_off] * len(ia), n + [t.n] * len(ia)
        ci, cj = np.asarray(ci, np.int64), np.asarray(cj, np.int64)
        g_all = L.read(pair_stat(self.data, row_index, ci, cj, off, n, ks[ci], ks[cj])) if len(ci) else np.zeros(0)
        return g_all, (ks[ci] - 1) * (ks[cj] - 1)

    def kmeans_batch(self, row_index, tasks, n_clusters):
        return L.KMeansBatch(self.data, row_index, [(t.row_off, t.n, t.scope, [self.ks[s] for s in t.scope], t.draw) for t in tasks],
                             KMEANS_RESTARTS, n_clusters, self.kmax)

    def gmm_batch(self, row_index, tasks, n_clusters):
        return L.GmmBatch(self.data, row_index, [(t.row_off, t.n, t.scope, [self.ks[s] for s in t.scope], t.draw) for t in tasks],
                          n_clusters, self.kmax)

    def clt_leaves(self, row_index, tasks, alpha):
        """The Chow-Liu leaf of every task (learning/leaf.py:149-150; ``t.draw`` is the position of its root): the
        co-occurrence counts of all of them from one launch and one read, then per task the host half of
        ``BinaryCLT.fit``.  Returns the fitted trees, in the order of the tasks."""
        from deeprob.spn.structure.cltree import BinaryCLT
        ones, out_off = L.pair_ones(self.data, row_index, [(t.row_off, t.n, t.scope) for t in tasks])
        ones = L.read(ones)
        leaves = []
        for t, off in zip(tasks, out_off):
            m = len(t.scope)
            leaf = BinaryCLT(t.scope, root=t.scope[t.draw])
            leaf.fit_counts(ones[off:off + m * m].reshape(m, m).astype(np.int64), t.n, alpha=alpha)
            leaves.append(leaf)
        return leaves


def learn_spn(
    data,
    distributions: list,
    domains: List[Union[list, tuple]],
    learn_leaf='mle',
    split_rows: str = 'kmeans',
    split_cols: str = 'rdc',
    learn_leaf_kwargs: dict = None,
    split_rows_kwargs: dict = None,
    split_cols_kwargs: dict = None,
    min_rows_slice: int = 256,
    min_cols_slice: int = 2,
    random_state=None,
    verbose: bool = True
):
    """
    Learn the structure and parameters of a SPN given some training data and several hyperparameters
    (reference learnspn.py:41-222), on the HIP device.

    Built: discrete data with ``Bernoulli`` (domain ``[0, 1]``) and ``Categorical`` leaves, every domain
    ``list(range(K))`` with ``K <= 16``; ``learn_leaf='mle'``, or the function
    ``deeprob.spn.learning.leaf.learn_binary_clt`` itself (recognised by identity; all-``Bernoulli`` data): Chow-Liu tree
    leaves, see below; ``split_rows`` in ``'kmeans'``, ``'random'``, or one of the functions ``gmm`` and ``kmeans`` of
    ``deeprob.spn.learning.splitting.cluster`` themselves (recognised by identity; ``split_rows_kwargs`` ``{'n': 2}``,
    1..8): ``gmm`` is the Gaussian-mixture split (full covariances, three initialisations, this project's definition:
    DESIGN.md 14.5), for discrete and for all-``Gaussian`` columns, with every column split and leaf learner that
    ``'kmeans'`` works with, and the function ``kmeans`` is the string ``'kmeans'``; the STRING ``'gmm'`` raises;
    ``split_cols`` in ``'gvs'``, ``'rgvs'``, ``'random'``, or the function
    ``deeprob.spn.learning.splitting.rdc.rdc_cols`` itself (recognised by identity): the RDC split as the exact maximal
    correlation, with ``split_cols_kwargs`` in ``d``, ``k``, ``s``; or one of the functions ``entropy_cols``,
    ``entropy_adaptive_cols``, ``gini_cols``, ``gini_adaptive_cols`` (``e``, ``alpha``; the adaptive two also ``size``,
    which is required), ``gvs_cols``, ``rgvs_cols`` (``p``) of ``deeprob.spn.learning.splitting`` themselves (recognised by
    identity): on discrete data the entropy and Gini splits come from the column counts a generation has read anyway,
    and ``gvs_cols`` / ``rgvs_cols`` are ``'gvs'`` / ``'rgvs'``.  Also built: all-continuous data, every distribution
    ``Gaussian`` and every domain a tuple ``(lo, hi)`` (learnspn_cont.py): ``split_rows`` in ``'kmeans'``, ``'random'``,
    ``split_cols`` ``'random'``, the function ``rdc_cols`` (there a ridge-regularised score of its own, see
    splitting/rdc.py) or one of the six functions above -- there on numpy's histograms of the float columns, ``'scott'``
    bins for the entropy and Gini splits and ``'fd'`` bins for the G-test, binned and counted on the device; a column of
    more than 1024 bins or a column pair of more than 12 288 cells raises ``ValueError`` --, MLE Gaussian leaves; the
    STRINGS ``'gvs'`` / ``'rgvs'`` raise there (a G-test needs a table), and ``'ebvs'``, ``'ebvs_ae'``, ``'gbvs'``,
    ``'gbvs_ag'``, ``'wrgvs'`` raise for both kinds.  Every other
    name the reference knows, every other callable, ``Uniform`` and mixed discrete / continuous data raise
    ``NotImplementedError`` before any device work -- so does the STRING ``'rdc'``, the default: pass
    ``split_cols=rdc_cols`` or ``split_cols='gvs'``.  ``'kmeans'`` is this project's own k-means, not
    scikit-learn's: the same kind of split, not the same labels.

    Chow-Liu tree leaves (``learn_leaf=learn_binary_clt``, ``learn_leaf_kwargs`` in ``to_pc``, ``alpha``, ``random_state``):
    a leaf task with more than one column becomes a ``BinaryCLT`` fitted to the task's rows -- the co-occurrence counts of
    all such tasks of a generation come from one launch (``dpl_pair_ones``) --; one-column leaves and the factorisations of
    constant columns stay MLE leaves, as in the reference.  ``FlatSpn`` has no multivariate leaf, so the circuit always
    holds the tree's ``to_pc`` expansion: ``to_pc`` is accepted and both values give the same ``FlatSpn``, whose likelihood,
    MPE and sampling distribution are those of the leaf; ``expectation_maximization`` on the result updates the expansion's
    sum weights freely, not as the tied CPTs of a tree.  The root of each tree is
    ``check_random_state(learn_leaf_kwargs['random_state']).choice(len(scope))``, evaluated per leaf in queue order among
    the other draws: an int re-seeds for every leaf, a ``RandomState`` is consumed in queue order and may be the very
    object passed as ``random_state`` (which is what the reference does with whatever is passed: its ``learn_spn``
    overwrites the key with its own generator, learnspn.py:112), None is a fresh unseeded generator per leaf.  The STRING
    ``'binary-clt'``, a wrapper around the function and a non-``Bernoulli`` distribution (``ValueError``) raise before any
    device work.

    :param data: The training data: a numpy array or a tensor on a HIP device, complete (no NaN).
    :param distributions: A list of distribution classes of ``deeprob.spn.structure.leaf`` (one for each feature).
    :param domains: A list of domains (one for each feature), each ``list(range(K))`` (``(lo, hi)`` for ``Gaussian``).
    :param learn_leaf: The method to use to learn a distribution leaf node: 'mle' or the function ``learn_binary_clt``.
    :param split_rows: The rows splitting method: 'kmeans', 'random', or the function ``gmm`` or ``kmeans`` of
                       ``deeprob.spn.learning.splitting.cluster``.
    :param split_cols: The columns splitting method: 'gvs', 'rgvs', 'random', the function ``rdc_cols`` or one of the
                       functions ``entropy_cols``, ``entropy_adaptive_cols``, ``gini_cols``, ``gini_adaptive_cols``,
                       ``gvs_cols``, ``rgvs_cols``.
    :param learn_leaf_kwargs: The parameters of the learn leaf method (``alpha`` | ``to_pc``, ``alpha``, ``random_state``).
    :param split_rows_kwargs: The parameters of the rows splitting method (``n`` | ``a``, ``b``).
    :param split_cols_kwargs: The parameters of the cols splitting method (``p`` | ``a``, ``b`` | ``d``, ``k``, ``s`` |
                              ``e``, ``alpha`` | ``e``, ``alpha``, ``size``).
    :param min_rows_slice: The minimum number of samples required to split horizontally.
    :param min_cols_slice: The minimum number of features required to split vertically.
    :param random_state: The random state. It can be either None, a seed integer or a Numpy RandomState.
    :param verbose: Accepted for compatibility (no progress bar is drawn).
    :return: A learned valid SPN, as a FlatSpn.
    :raises ValueError: If a parameter is out of scope, the data holds NaN or a domain is not ``range(K)``.
    :raises NotImplementedError: For what the reference knows and this path does not build.
    :raises HipError: If the data is a CPU tensor or the native library is missing.
    """
    if R.all_gaussian(distributions):
        from deeprob.spn.learning.learnspn_cont import GaussianColumns
        kind = GaussianColumns(distributions, domains)
    else:
        kind = DiscreteColumns(distributions, domains)
    leaf_kw, rows_kw, cols_kw = check_arguments(kind, data, distributions, domains, learn_leaf, split_rows, split_cols,
                                                learn_leaf_kwargs, split_rows_kwargs, split_cols_kwargs, min_rows_slice,
                                                min_cols_slice)
    random_state = check_random_state(random_state)
    if split_cols is R.rdc_cols:
        split_cols = 'rdc'
    elif hist_split(split_cols) is not None:
        split_cols = hist_split(split_cols)
    clt = learn_leaf is learn_binary_clt
    split_rows = rows_split(split_rows) or split_rows      # ('gmm' is reached through the function only: the string has raised)
    dev_data = kind.upload(data)
    device = dev_data.device
    n_total, n_features = dev_data.n_rows, dev_data.n_cols
    alpha = float(leaf_kw['alpha'])
    L.reset_counters()
    row_index = torch.arange(n_total, dtype=torch.int32, device=device)

    tmp_node = new_node('Product', range(n_features))
    generation = [_Task(tmp_node, n_total, list(range(n_features)), is_first=True)]
    tasks_per_generation, lloyd_iterations, gmm_iterations, clt_records = [], 0, 0, []
    while generation:
        tasks_per_generation.append(len(generation))
        # ---- column statistics of every task, the operation of every task (learnspn.py:130-147) ----------------------
        stats, constant = kind.column_stats(row_index, *item_tables(generation))
        first = 0
        for t in generation:
            t.counts, zero_var = stats[first:first + len(t.scope)], constant[first:first + len(t.scope)]
            first += len(t.scope)
            t.draw = zero_var
            if zero_var.all():
                t.op = 'naive'
            elif zero_var.any():
                t.op = 'rem'
            elif t.no_rows_split or len(t.scope) < min_cols_slice or t.n < min_rows_slice:
                t.op = 'leaf'
            elif t.no_cols_split or t.is_first:
                t.op = 'rows'
            else:
                t.op = 'cols'
        # ---- the draws, in queue order (random.py:31-32, 56-57; k-means seeds; the kind's column-split draws) -------
        for t in generation:
            if t.op == 'rows' and split_rows == 'random':
                p = random_state.beta(rows_kw['a'], rows_kw['b'])
                t.draw = random_state.binomial(1, p, size=t.n)
            elif t.op == 'rows':
                c = int(rows_kw['n'])
                if t.n < c:
                    raise ValueError("n_samples={} should be >= n_clusters={}".format(t.n, c))
                t.draw = np.stack([random_state.choice(t.n, c, replace=False)
                                   for _ in range(L.GMM_N_INIT if split_rows == 'gmm' else KMEANS_RESTARTS)])
            elif t.op == 'cols' and split_cols == 'random':
                p = random_state.beta(cols_kw['a'], cols_kw['b'])
                t.draw = random_state.binomial(1, p, size=len(t.scope))
            elif t.op == 'cols':
                t.draw = kind.draw_split_cols(random_state, t, split_cols, cols_kw)
            elif t.op == 'leaf' and clt and len(t.scope) > 1:
                # the root of the tree, drawn where the reference's leaf function draws it (cltree.py:185-189)
                t.draw = int(check_random_state(leaf_kw['random_state']).choice(len(t.scope)))
        # ---- the column clusters of every column-splitting task that is not 'random' ---------------------------------
        tested = [t for t in generation if t.op == 'cols' and split_cols != 'random']
        clusters_of = {id(t): c for t, c in zip(tested, kind.split_cols_clusters(row_index, tested, split_cols, cols_kw))}
        # ---- the Chow-Liu trees of every multivariate leaf task -------------------------------------------------------
        clt_tasks = [t for t in generation if t.op == 'leaf' and clt and len(t.scope) > 1]
        clt_of = {}
        if clt_tasks:
            for t, leaf in zip(clt_tasks, kind.clt_leaves(row_index, clt_tasks, alpha)):
                clt_of[id(t)] = leaf
                clt_records.append({'scope': list(t.scope), 'root': leaf.scope[leaf.root], 'tree': leaf.tree, 'params': leaf.params,
                                    'n': t.n, 'rows': row_index[t.row_off:t.row_off + t.n]})
        # ---- k-means of every row-splitting task ----------------------------------------------------------------------
        km_tasks = [t for t in generation if t.op == 'rows' and split_rows in ('kmeans', 'gmm')]
        km_labels, km_result = None, {}
        if km_tasks and split_rows == 'gmm':
            batch = kind.gmm_batch(row_index, km_tasks, int(rows_kw['n']))
            best, _, sizes, km_labels, iters = batch.run()     # the largest bound, the first one on a tie
            gmm_iterations += iters
            for i, t in enumerate(km_tasks):
                km_result[id(t)] = (int(best[i]) * batch.n_lab + batch.lab_off[i], sizes[i, int(best[i])])
        elif km_tasks:
            batch = kind.kmeans_batch(row_index, km_tasks, int(rows_kw['n']))
            inertia, sizes, km_labels, iters = batch.run()
            lloyd_iterations += iters
            for i, t in enumerate(km_tasks):
                best = int(np.argmin(inertia[i]))              # the lowest inertia, the first one on a tie
                km_result[id(t)] = (best * batch.n_lab + batch.lab_off[i], sizes[i, best])
        # ---- the nodes and the children of every task, in queue order (learnspn.py:149-210) -------------------------
        children, host_labels, n_host_labels = [], [], 0

        def child(task, parent_task, label_off=0, label=-1):
            task.child_src = (parent_task.row_off, parent_task.n, label_off, label)
            children.append(task)

        for t in generation:
            scope, nf = t.scope, len(t.scope)
            if t.op == 'rem':
                zero_var = t.draw
                node = new_node('Product', scope)
                rem = [i for i in range(nf) if zero_var[i]]
                node['children'].append(naive_factorization(kind, [scope[i] for i in rem], [t.counts[i] for i in rem], t.n,
                                                            alpha))
                child(_Task(node, t.n, [scope[i] for i in range(nf) if not zero_var[i]], is_first=t.is_first), t)
                t.parent['children'].append(node)
            elif id(t) in clt_of:
                t.parent['children'].append(clt_of[id(t)].to_pc_nodes())      # (FlatSpn has no multivariate leaf)
            elif t.op == 'leaf' and nf == 1:
                t.parent['children'].append(kind.leaf(scope[0], t.counts[0], t.n, alpha))
            elif t.op in ('leaf', 'naive'):
                t.parent['children'].append(naive_factorization(kind, scope, t.counts, t.n, alpha))
            elif t.op == 'rows':
                if split_rows == 'random':
                    labels = t.draw.astype(np.uint8)
                    sizes_t = np.bincount(labels, minlength=2)
                    label_off = n_host_labels
                    host_labels.append(labels)
                    n_host_labels += t.n
                else:
                    label_off, sizes_t = km_result[id(t)]
                present = [c for c in range(len(sizes_t)) if sizes_t[c] > 0]
                if len(present) == 1:
                    child(_Task(t.parent, t.n, scope, no_cols_split=False, no_rows_split=True), t)
                    continue
                node = new_node('Sum', scope, weights=[int(sizes_t[c]) / t.n for c in present])
                for c in present:
                    child(_Task(node, int(sizes_t[c]), scope), t, label_off, c)
                t.parent['children'].append(node)
            else:
                clusters = np.asarray(t.draw) if split_cols == 'random' else clusters_of[id(t)]
                present = np.unique(clusters)
                if len(present) == 1:
                    child(_Task(t.parent, t.n, scope, no_cols_split=True, no_rows_split=False), t)
                    continue
                node = new_node('Product', scope)
                for c in present:
                    child(_Task(node, t.n, [scope[i] for i in range(nf) if clusters[i] == c]), t)
                t.parent['children'].append(node)
        # ---- the next generation's row index ----------------------------------------------------------------------------
        if children:
            off = 0
            for c in children:
                c.row_off = off
                off += c.n
            if host_labels:
                km_labels = L.upload(device, labels=np.concatenate(host_labels))['labels']
            src = np.array([c.child_src for c in children], np.int64)
            row_index = L.partition_rows(row_index, src[:, 0], src[:, 1], src[:, 2], src[:, 3], [c.row_off for c in children],
                                         [c.n for c in children], None if km_labels is None else km_labels.reshape(-1), off)
        generation = children

    c = L.COUNTERS
    _last_info.clear()
    _last_info.update(generations=len(tasks_per_generation), launches=c['kernels'] + c['reads'] + c['uploads'],
                      kernels=c['kernels'], reads=c['reads'], uploads=c['uploads'],
                      lloyd_launches=c['lloyd_kernels'] + c['lloyd_reads'], lloyd_iterations=lloyd_iterations,
                      tasks_per_generation=tasks_per_generation, clt_leaves=clt_records,
                      gmm_kernels=c['gmm_kernels'], gmm_reads=c['gmm_reads'], gmm_uploads=c['gmm_uploads'],
                      gmm_iterations=gmm_iterations)
    if kind.launches_per_generation is not None:
        _last_info['launches_per_generation'] = kind.launches_per_generation + (CLT_LAUNCHES_PER_GENERATION if clt else 0)
    return to_flat(tmp_node['children'][0])
