"""``learn_cnet_bd`` and ``learn_cnet_bic``: the scored cutset-network learners of the reference
(deeprob/spn/learning/cnet_bayesian.py), on the HIP device through ``libdeeprob_clt.so``.

Both grow an OR tree breadth first.  Per open node they take the ``k`` columns of largest information gain as candidate
cuts, fit a Chow-Liu tree to the rows on each side of every candidate, score "cut here" as the sum of the two trees' scores
and the OR node's own, and split at the best candidate iff that beats the score of the node's single tree -- the BDeu score
(``learn_cnet_bd``) or BIC (``learn_cnet_bic``).

The search is level synchronous like ``BinaryCNet.fit``: a generation is every open node of one depth.  Per generation the
rows are packed into bit planes, the counts and gains of every task are taken (``dpc_cnet_pair_counts``,
``dpc_cnet_scores``), and ONE launch of ``dpc_cut_pair_counts`` counts the rows of every (task, candidate) entry that have
the candidate set -- a three-way AND + popcount.  The other side is the task's counts minus those.  The host reads the
active block of every entry and does what is left: float32 mutual information, Prim's spanning tree and a score of O(d)
``math.lgamma`` / log terms per tree.  A child inherits the counts, the tree and the score of the side that won, so nothing
is counted or fitted twice, and the training rows never come back.

Differences from the reference, all in DESIGN.md §17: candidates are ordered (larger gain first, ties to the lower
column) where the reference takes ``np.argpartition``'s order; a trial tree is rooted at the first position of its scope
and the leaves of the result draw their roots from ``random_state`` afterwards, one per leaf breadth first, keeping the
undirected tree that was scored (the reference draws every trial root from an unseeded generator); the scores are float64
from exact integer counts (the reference mixes float32 in).  There is no CPU fallback.
"""
import math
import time
from typing import Optional

import numpy as np

from deeprob.spn.structure.cltree import BinaryCLT
from deeprob.spn.structure.cnet import BinaryCNet
from deeprob.utils.graph import maximum_spanning_tree
from deeprob.utils.random import RandomState, check_random_state
from deeprob.utils.statistics import compute_mutual_information, device_binary_rows, device_training_rows, pair_counts, \
    priors_joints_from_counts

#: the smoothing of the mutual information behind a BDeu trial tree (the reference's ``fit(..., alpha=0.01)``)
BD_TREE_ALPHA = 0.01
#: kernel launches of libdeeprob_clt.so per generation, whatever its number of tasks, while tasks and entries fit one
#: chunk each: gather-pack, pair counts, scores (two kernels), conditioned counts, partition
LAUNCHES_PER_GENERATION = 6

_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])
_profile = {}


def last_profile() -> dict:
    """Where the last ``learn_cnet_bd`` / ``learn_cnet_bic`` spent its time (also ``fit_profile_`` of its result):
    ``generations``, ``tasks_per_generation``, ``entries`` (trial cuts counted on the device), ``launches`` (kernels of
    ``libdeeprob_clt.so``), ``gathers`` (block reads), ``host_tree_seconds`` (trial trees and their scores) and ``seconds``."""
    return dict(_profile)


# ---- counts to scores ------------------------------------------------------------------------------------------------------
def _cells(ones: np.ndarray, n: int) -> np.ndarray:
    """``[D, D, 2, 2]`` int64, ``[i, j, k, l]`` = rows with ``x_i = k`` and ``x_j = l``."""
    ones = np.asarray(ones, np.int64)
    col = np.diag(ones)
    cells = np.empty(ones.shape + (2, 2), np.int64)
    cells[:, :, 1, 1] = ones
    cells[:, :, 0, 1] = col[None, :] - ones
    cells[:, :, 1, 0] = col[:, None] - ones
    cells[:, :, 0, 0] = n - col[None, :] - col[:, None] + ones
    return cells


def _or_bd_scores(col: np.ndarray, n: int, ess: float) -> np.ndarray:
    """BDeu score of every variable without a parent: ``col[i]`` rows of ``n`` have ``x_i = 1``."""
    col = np.asarray(col, np.float64)
    return (math.lgamma(ess) - math.lgamma(n + ess)) + (_lgamma(n - col + ess / 2) - math.lgamma(ess / 2)) \
        + (_lgamma(col + ess / 2) - math.lgamma(ess / 2))


def _family_bd_scores(cells: np.ndarray, ess: float) -> np.ndarray:
    """BDeu score of a child given one parent from ``cells[..., k, l]`` (child = k, parent = l), over the leading axes."""
    cells = np.asarray(cells, np.float64)
    parent = cells.sum(axis=-2)                                     # [..., l]
    per_value = (math.lgamma(ess / 2) - _lgamma(parent + ess / 2)) \
        + (_lgamma(cells[..., 0, :] + ess / 4) - math.lgamma(ess / 4)) \
        + (_lgamma(cells[..., 1, :] + ess / 4) - math.lgamma(ess / 4))
    return per_value[..., 0] + per_value[..., 1]


def _trial_tree(block: np.ndarray, n: int, alpha: float):
    """``(bfs, tree, priors, joints)``: the Chow-Liu tree of the counts ``block`` of ``n`` rows, rooted at position 0 --
    the host half of ``BinaryCLT.fit_counts`` up to the structure."""
    priors, joints = priors_joints_from_counts(block, n, alpha=alpha)
    bfs, tree = maximum_spanning_tree(0, compute_mutual_information(priors, joints))
    return bfs, tree, priors, joints


def _tree_cells(block: np.ndarray, n: int, tree: np.ndarray):
    """``(root, children [d - 1], cells [d - 1, 2, 2])``: per non-root position its four counts against its parent,
    ``cells[., k, l]`` = rows with child = k and parent = l."""
    block = np.asarray(block, np.int64)
    root = int(np.flatnonzero(tree < 0)[0])
    child = np.flatnonzero(tree >= 0)
    pa = tree[child]
    both, c, p = block[child, pa], block[child, child], block[pa, pa]
    cells = np.empty((len(child), 2, 2), np.int64)
    cells[:, 1, 1], cells[:, 1, 0], cells[:, 0, 1], cells[:, 0, 0] = both, c - both, p - both, n - c - p + both
    return root, child, cells


def _bd_tree_score(block, n, tree, ess) -> float:
    """BDeu score of a tree: the families of the non-root positions plus the root's, O(d) ``lgamma`` terms."""
    root, _, cells = _tree_cells(block, n, tree)
    return math.fsum(_family_bd_scores(cells, ess).tolist()
                     + _or_bd_scores(np.asarray(block)[root:root + 1, root], n, ess).tolist())


def _tree_log_likelihood(block, n, tree, params) -> float:
    """The log likelihood of the counted rows under a tree with the float32 log tables ``params``: per position the four
    counts against its parent times ``params[i, l, k]``; a cell of no rows adds nothing."""
    root, child, cells = _tree_cells(block, n, tree)
    logp = np.asarray(params, np.float64)
    with np.errstate(invalid='ignore'):
        terms = np.where(cells > 0, cells * logp[child].transpose(0, 2, 1), 0.0).reshape(-1).tolist()
    c_root = int(np.asarray(block)[root, root])
    for count, lp in ((n - c_root, logp[root, 0, 0]), (c_root, logp[root, 0, 1])):
        if count > 0:
            terms.append(count * float(lp))
    return math.fsum(terms)


class _Scorer:
    """What differs between the two learners: the smoothing per depth and the score of a tree and of an OR node."""

    def __init__(self, kind: str, par: float, n_total: int):
        self.kind, self.par, self.log_n = kind, float(par), math.log(n_total)

    def ess(self, depth: int) -> float:
        return self.par / 2.0 ** depth

    def gain_alpha(self, depth: int) -> float:
        """The ``alpha`` of ``dpc_cnet_scores`` that gives the smoothing of ``select_cand_cuts``."""
        return self.ess(depth) / 4 if self.kind == 'bd' else self.par

    def leaf_alpha(self, depth: int) -> float:
        """The smoothing of a leaf's tables (``estimate_clt_params_bayesian`` for BDeu)."""
        return self.ess(depth) / 4 if self.kind == 'bd' else self.par

    def tree(self, block, n, depth):
        """``(tree rooted at position 0, its score)`` of the counts ``block`` of ``n`` rows at ``depth``."""
        if self.kind == 'bd':
            _, tree, _, _ = _trial_tree(block, n, BD_TREE_ALPHA)
            return tree, _bd_tree_score(block, n, tree, self.ess(depth))
        bfs, tree, priors, joints = _trial_tree(block, n, self.par)
        with np.errstate(divide='ignore'):      # (alpha = 0 can leave a zero probability)
            params = np.log(BinaryCLT.compute_clt_parameters(bfs, tree, priors, joints))
        # the penalty counts the rows of the WHOLE training set at every depth, as the reference does
        return tree, _tree_log_likelihood(block, n, tree, params) - 0.5 * self.log_n * (2 * len(tree) - 1)

    def left_weight(self, n_left, n, depth) -> float:
        if self.kind == 'bd':
            return (n_left + self.ess(depth) / 2) / (n + self.ess(depth))
        return (n_left + self.par) / (n + 2 * self.par)

    def or_score(self, n_left, n, depth) -> float:
        if self.kind == 'bd':
            return float(_or_bd_scores(np.array([n - n_left]), n, self.ess(depth))[0])
        left = self.left_weight(n_left, n, depth)
        return n_left * math.log(left) + (n - n_left) * math.log(1 - left) - 0.5 * self.log_n


def _reroot(tree: np.ndarray, root: int) -> np.ndarray:
    """The predecessors of the same undirected tree with ``root`` on top."""
    tree = np.array(tree, np.int32)
    path, at = [], int(root)
    while at >= 0:
        path.append(at)
        at = int(tree[at])
    for child, parent in zip(path[:-1], path[1:]):
        tree[parent] = child
    tree[root] = -1
    return tree


# ---- the reference's helpers on one data matrix ----------------------------------------------------------------------------
def _check_ess(ess):
    if not ess > 0.0:
        raise ValueError("The equivalent sample size must be positive")


def compute_or_bd_scores(data, ess: float = 0.1) -> np.ndarray:
    """
    The BDeu score of every variable as an OR node (or as the root of a tree) given the data.

    :param data: The binary data matrix ``[N, D]``: a numpy array or a device tensor.
    :param ess: The equivalent sample size (ESS).
    :return: The scores, ``[D]`` float64.
    """
    _check_ess(ess)
    ones, n = pair_counts(data)
    return _or_bd_scores(np.diag(ones), n, ess)


def compute_clt_bd_scores(data, ess: float = 0.1) -> np.ndarray:
    """
    The pairwise BDeu scores a Chow-Liu tree is scored with.

    :param data: The binary data matrix ``[N, D]``: a numpy array or a device tensor.
    :param ess: The equivalent sample size (ESS).
    :return: ``[D, D]`` float64, ``[i, j]`` = the score of ``i`` with parent ``j``.
    """
    _check_ess(ess)
    ones, n = pair_counts(data)
    return _family_bd_scores(_cells(ones, n), ess)


def eval_tree_score(tree, clt_scores: np.ndarray, or_scores: np.ndarray) -> float:
    """
    The BDeu score of a tree structure.

    :param tree: The predecessors, -1 at the root.
    :param clt_scores: The pairwise scores of :func:`compute_clt_bd_scores`.
    :param or_scores: The scores of :func:`compute_or_bd_scores`.
    """
    tree = np.asarray(tree, np.int64)
    child = np.flatnonzero(tree >= 0)
    root = int(np.flatnonzero(tree < 0)[0])
    return math.fsum(np.asarray(clt_scores, np.float64)[child, tree[child]].tolist() + [float(or_scores[root])])


def _top_candidates(gains: np.ndarray, cols: np.ndarray, k: int) -> np.ndarray:
    """The ``k`` columns of ``cols`` (ascending) with the largest gain, larger gain first, ties to the lower column."""
    return cols[np.argsort(-gains[cols], kind='stable')[:k]]


def select_cand_cuts(data, ess: float = 0.1, n_cand_cuts: int = 10) -> np.ndarray:
    """
    The candidate cut columns of a data matrix: the ``min(n_cand_cuts, D)`` columns of largest information gain, larger
    gain first, ties to the lower column (always an array; the reference's order is ``np.argpartition``'s).

    :param data: The binary data matrix ``[N, D]``: a numpy array or a device tensor.
    :param ess: The equivalent sample size: the counts are smoothed by ``ess / 2`` and ``ess``.
    :param n_cand_cuts: The number of candidates.
    """
    import torch
    from deeprob.hip import cnet
    _check_ess(ess)
    if n_cand_cuts < 1:
        raise ValueError("n_cand_cuts must be at least 1")
    x = device_training_rows(data)
    n, d = x.shape
    gen = cnet.Generation(x, torch.arange(n, dtype=torch.int32, device=x.device), [n])
    gen.pack()
    gains, _, _ = gen.scores(gen.counts(0, 1), 0, np.ones((1, d), np.uint8), ess / 4)
    return _top_candidates(gains.cpu().numpy()[0], np.arange(d), min(int(n_cand_cuts), d))


# ---- the learners ----------------------------------------------------------------------------------------------------------
class _Task:
    """An open node: its rows' number, active columns (ascending), and the counts, tree and score it inherited."""
    __slots__ = ('node', 'n', 'cols', 'block', 'tree', 'score')

    def __init__(self, node, n, cols, block, tree, score):
        self.node, self.n, self.cols, self.block, self.tree, self.score = node, n, cols, block, tree, score


def _learn(data, kind: str, par: float, n_cand_cuts: int, random_state) -> BinaryCNet:
    """The search and the leaves.  Every node of the result also records what the search saw of it: ``n_rows_``, ``score_``
    (the score of its single tree) and ``candidates_`` (``[(variable, score of cutting there)]`` in the order tried)."""
    import torch
    from deeprob.hip import clt, cnet
    if n_cand_cuts < 1:
        raise ValueError("n_cand_cuts must be at least 1")
    random_state = check_random_state(random_state)
    x = device_training_rows(data)
    t_start, t_host = time.perf_counter(), 0.0
    n_rows, d = x.shape
    scorer = _Scorer(kind, par, n_rows)
    root = BinaryCNet(list(range(d)))

    # the root's own tree and score, from the counts of all rows
    block = clt.pair_counts(clt.pack_bits(x)).cpu().numpy().astype(np.int64)
    launches, gathers, n_entries = 2, 1, 0
    t0_host = time.perf_counter()
    tree, score = scorer.tree(block, n_rows, 0)
    t_host += time.perf_counter() - t0_host
    tasks = [_Task(root, n_rows, np.arange(d), block, tree, score)]
    rows = torch.arange(n_rows, dtype=torch.int32, device=x.device)
    leaves, widths, depth = {}, [], 0           # leaves: id(node) -> (task, depth)
    step = None
    while any(len(t.cols) > 1 for t in tasks):
        widths.append(len(tasks))
        gen = cnet.Generation(x, rows, [t.n for t in tasks])
        gen.pack()
        launches += 1
        cut = np.full(len(tasks), -1, np.int64)
        next_tasks = []
        step = cnet.chunk_tasks(d)
        for t0 in range(0, len(tasks), step):
            chunk = tasks[t0:t0 + step]
            active = np.zeros((len(chunk), d), np.uint8)
            for i, task in enumerate(chunk):
                active[i, task.cols] = 1
            gains, _, _ = gen.scores(gen.counts(t0, len(chunk)), t0, active, scorer.gain_alpha(depth))
            launches += 3
            gains = gains.cpu().numpy()
            # the entries: per task its candidates in order, those with an empty side left out
            entries = []                        # (task in the chunk, position of the cut in its columns, rows with it set)
            for i, task in enumerate(chunk):
                task.node.score_, task.node.candidates_, task.node.n_rows_ = task.score, [], task.n
                if len(task.cols) < 2:
                    continue
                for c in _top_candidates(gains[i], task.cols, min(int(n_cand_cuts), len(task.cols))):
                    at = int(np.searchsorted(task.cols, c))
                    n_set = int(task.block[at, at])
                    if 0 < n_set < task.n:
                        entries.append((i, at, n_set))
            n_entries += len(entries)
            trials = {}                         # task in the chunk -> [(total, position, n_set, sides)]
            for e0 in range(0, len(entries), step):
                part = entries[e0:e0 + step]
                ones1 = gen.cut_counts([t0 + i for i, _, _ in part], [chunk[i].cols[at] for i, at, _ in part])
                launches += 1
                # the active blocks without the cut column, gathered on the device, in one read
                index = []
                for e, (i, at, _) in enumerate(part):
                    rest = np.delete(chunk[i].cols, at)
                    index.append(((e * d + rest[:, None]) * d + rest[None, :]).reshape(-1))
                set_blocks = ones1.reshape(-1)[torch.from_numpy(np.concatenate(index)).to(x.device)].cpu().numpy().astype(np.int64)
                gathers += 1
                t0_host, off = time.perf_counter(), 0
                for i, at, n_set in part:
                    task = chunk[i]
                    k = len(task.cols) - 1
                    right = set_blocks[off:off + k * k].reshape(k, k)
                    off += k * k
                    left = np.delete(np.delete(task.block, at, axis=0), at, axis=1) - right
                    sides = []
                    for side_block, side_n in ((left, task.n - n_set), (right, n_set)):
                        side_tree, side_score = scorer.tree(side_block, side_n, depth + 1)
                        sides.append((side_block, side_n, side_tree, side_score))
                    total = math.fsum([sides[0][3], sides[1][3], scorer.or_score(task.n - n_set, task.n, depth)])
                    task.node.candidates_.append((int(task.cols[at]), total))
                    trials.setdefault(i, []).append((total, at, n_set, sides))
                t_host += time.perf_counter() - t0_host
            for i, task in enumerate(chunk):
                best = None
                for trial in trials.get(i, ()):             # the first with the strictly largest score
                    if best is None or trial[0] > best[0]:
                        best = trial
                if best is None or not best[0] > task.score:
                    leaves[id(task.node)] = (task, depth)
                    continue
                _, at, n_set, sides = best
                node, column = task.node, int(task.cols[at])
                left_weight = scorer.left_weight(task.n - n_set, task.n, depth)
                scope = [v for v in node.scope if v != column]
                node.children = [BinaryCNet(scope), BinaryCNet(list(scope))]
                node.weights, node.or_id = [left_weight, 1 - left_weight], column
                cut[t0 + i] = column
                rest = np.delete(task.cols, at)
                next_tasks += [_Task(child, side_n, rest, side_block, side_tree, side_score)
                               for child, (side_block, side_n, side_tree, side_score) in zip(node.children, sides)]
        if not next_tasks:
            tasks = []
            break
        rows, _ = gen.partition(cut)
        launches += 1
        tasks, depth = next_tasks, depth + 1
    for task in tasks:                          # what is left open has one column each (or is a lone root)
        task.node.score_, task.node.candidates_, task.node.n_rows_ = task.score, [], task.n
        leaves[id(task.node)] = (task, depth)

    # the leaves, breadth first, left child before right: a drawn root over the tree that was scored
    t0_host = time.perf_counter()
    order, at = [root], 0
    while at < len(order):
        node = order[at]
        at += 1
        if node.children:
            order += node.children
            continue
        task, leaf_depth = leaves[id(node)]
        drawn = int(random_state.choice(len(node.scope)))
        node.clt = BinaryCLT(node.scope, tree=_reroot(task.tree, drawn))
        node.clt.fit_counts(task.block, task.n, alpha=scorer.leaf_alpha(leaf_depth))
    t_host += time.perf_counter() - t0_host
    torch.cuda.synchronize(x.device)
    total = time.perf_counter() - t_start
    _profile.clear()
    _profile.update(learner=kind, seconds=total, host_tree_seconds=t_host, device_seconds=total - t_host,
                    generations=len(widths), tasks_per_generation=widths, entries=n_entries, launches=launches,
                    gathers=gathers)
    root.fit_profile_ = last_profile()
    return root


def learn_cnet_bd(data, ess: float = 0.1, n_cand_cuts: int = 10, random_state: Optional[RandomState] = None) -> BinaryCNet:
    """
    Learn a binary CNet using the Bayesian-Dirichlet equivalent uniform (BDeu) score.

    :param data: The training data ``[N, D]``, every value 0 or 1: a numpy array or a device tensor.
    :param ess: The equivalent sample size (ESS); a node of depth ``k`` uses ``ess / 2 ** k``.
    :param n_cand_cuts: The number of candidate cut columns per node.
    :param random_state: None, a seed or a Numpy RandomState: draws the root of every leaf's tree.
    :return: A binary CNet.
    :raises ValueError: If a parameter is out of domain or the data are not binary.
    """
    _check_ess(ess)
    return _learn(data, 'bd', ess, n_cand_cuts, random_state)


def learn_cnet_bic(data, alpha: float = 0.01, n_cand_cuts: int = 10, random_state: Optional[RandomState] = None) -> BinaryCNet:
    """
    Learn a binary CNet using the Bayesian Information Criterion (BIC) score.

    :param data: The training data ``[N, D]``, every value 0 or 1: a numpy array or a device tensor.
    :param alpha: The Laplace smoothing factor.
    :param n_cand_cuts: The number of candidate cut columns per node.
    :param random_state: None, a seed or a Numpy RandomState: draws the root of every leaf's tree.
    :return: A binary CNet.
    :raises ValueError: If a parameter is out of domain or the data are not binary.
    """
    if alpha < 0.0:
        raise ValueError("The Laplace smoothing factor must be non-negative")
    return _learn(data, 'bic', alpha, n_cand_cuts, random_state)
