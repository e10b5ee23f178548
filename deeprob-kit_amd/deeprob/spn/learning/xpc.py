"""``learn_xpc`` / ``learn_expc``: extremely randomized probabilistic circuits and their ensembles (reference
spn/learning/xpc.py) on the HIP path.  They return a :class:`deeprob.spn.structure.io.FlatSpn`, so a learned XPC has every
query of the node-graph SPNs: ``log_likelihood`` with NaN, ``mpe``, ``sample``, ``moments``, ``posterior``, EM.

The data are uploaded and packed into bit planes once per call.  The partition tree is drawn on the host
(``deeprob.spn.utils.partitioning``), every horizontal split being one histogram and one stable split on the device.  The
leaves under conjunction variables -- naive factorizations, deterministic disjunctions, conjunctions -- come from those
histograms.  All Chow-Liu leaves of a circuit (of every member of an ensemble) are the tasks of ONE
``deeprob.hip.cnet.Generation``: one gather-pack, the exact co-occurrence counts in chunks of ``chunk_tasks(D)``, and per
leaf its block of the counts, from which ``BinaryCLT.fit_counts`` and the mutual information of ``build_trees_dict`` are
host float32 arithmetic.  A ``BinaryCLT`` leaf is expanded by ``to_pc_nodes()``: ``FlatSpn`` has no multivariate leaf.

Deliberate differences from the reference (README, DESIGN.md "XPCs"): the root of a Chow-Liu leaf without a given tree is
drawn from a second generator ``RandomState(random_seed)`` used for nothing else (the reference draws it from an unseeded
generator); the reference's assertions are ``ValueError`` with its texts; arguments are checked; ``det=True`` with
``use_clt=False`` raises (the reference crashes there); there is no CPU fallback.  ``learn_expc`` shuffles the members'
ordering with the GLOBAL ``np.random.shuffle``, cumulatively, exactly as the reference does: ``np.random.seed(s)`` in front
of the call reproduces the reference's ensemble.
"""
import time
from typing import Optional, Tuple

import numpy as np

from deeprob.spn.learning.learnspn import new_node, to_flat
from deeprob.spn.structure.cltree import BinaryCLT
from deeprob.spn.utils.partitioning import DeviceRows, Partition, generate_random_partitioning
from deeprob.utils.graph import maximum_spanning_tree
from deeprob.utils.statistics import compute_mutual_information, priors_joints_from_counts

# SD stands for Structured Decomposable
SD_LEVEL_0 = 0  # non-SD ensemble of non-SD PCs
SD_LEVEL_1 = 1  # non-SD ensemble of SD PCs
SD_LEVEL_2 = 2  # SD ensemble
SD_LEVELS = [SD_LEVEL_0, SD_LEVEL_1, SD_LEVEL_2]

ROOT = -1

_profile = {}


def last_profile() -> dict:
    """Where the last ``learn_xpc`` / ``learn_expc`` of this process spent its time, in seconds (host clock around steps
    that end in a synchronise): ``pack`` (upload and bit planes), ``partition`` (the partition trees: draws, histograms,
    splits, the read of the row ids), ``leaf_counts`` (gather-pack, co-occurrence counts and their read-back) and ``host``
    (mutual information, trees, leaves and the flat circuit)."""
    return dict(_profile)


class _Clock:
    """Laps of a learner call; every lap ends in a synchronise of ``device`` (set once the data are on it)."""

    def __init__(self):
        import torch
        self.device = None
        self.sync = lambda: torch.cuda.synchronize(self.device)
        self.times, self.t = {}, time.perf_counter()

    def lap(self, name):
        self.sync()
        now = time.perf_counter()
        self.times[name] = self.times.get(name, 0.0) + now - self.t
        self.t = now


def _check(conj_len, arity, min_part_inst, det, use_clt):
    from deeprob.hip.clt import DPC_XPC_MAX_CONJ
    if not 1 <= conj_len <= DPC_XPC_MAX_CONJ:
        raise ValueError("conj_len must be in the interval [1, {}] (DPC_XPC_MAX_CONJ)".format(DPC_XPC_MAX_CONJ))
    if arity < 2:
        raise ValueError("Arity must be in the interval [2, 2 ** conj_len]")
    if min_part_inst < 1:
        raise ValueError("min_part_inst must be at least 1")
    if det and not use_clt:
        raise ValueError("det=True needs use_clt=True: a leaf partition that is not under a conjunction has no "
                         "discarded assignments to build a deterministic disjunction from")


# ---- counts of the Chow-Liu leaf partitions -----------------------------------------------------------------------------
class _LeafCounts:
    """The co-occurrence counts of leaf partitions (disjoint within a circuit, so at most N rows per circuit) as the tasks
    of one ``Generation``; the counts stay on the device, ``blocks`` reads the ``[cols][:, cols]`` block of every task."""

    def __init__(self, dev: DeviceRows, parts):
        import torch
        from deeprob.hip import cnet
        self.parts, self.d = parts, dev.shape[1]
        rows = torch.cat([p.device_rows for p in parts]) if len(parts) > 1 else parts[0].device_rows.contiguous()
        gen = cnet.Generation(dev.x, rows, [p.n_rows for p in parts])
        gen.pack()
        self.step = cnet.chunk_tasks(self.d)
        self.chunks = [gen.counts(t0, min(self.step, len(parts) - t0)) for t0 in range(0, len(parts), self.step)]

    def blocks(self, cols_of, parts=None) -> dict:
        """``{id(part): int64 [k, k] counts over the columns cols_of(part)}`` for ``parts`` (default: all), one read per
        chunk."""
        import torch
        out, d = {}, self.d
        wanted = None if parts is None else {id(p) for p in parts}
        for c, ones in enumerate(self.chunks):
            picked = [(i, p) for i, p in enumerate(self.parts[c * self.step:(c + 1) * self.step])
                      if wanted is None or id(p) in wanted]
            if not picked:
                continue
            cols = [np.asarray(cols_of(p), np.int64) for _, p in picked]
            index = np.concatenate([((i * d + k[:, None]) * d + k[None, :]).reshape(-1) for (i, _), k in zip(picked, cols)])
            flat = ones.reshape(-1)[torch.from_numpy(index).to(ones.device)].cpu().numpy().astype(np.int64)
            at = 0
            for (_, p), k in zip(picked, cols):
                out[id(p)] = flat[at:at + len(k) ** 2].reshape(len(k), len(k))
                at += len(k) ** 2
        return out


# ---- the reference's host steps, from counts ----------------------------------------------------------------------------
def greedy_vars_ordering(data, conj_len: int, alpha: float = 0.01) -> list:
    """The ordering of the variables by the reference's heuristic: the variable with the largest summed mutual information
    first, then the ``conj_len - 1`` free variables it shares the most information with, and so on.  ``data``: binary rows
    (numpy or device tensor) or their :class:`DeviceRows`; the counts come from the device."""
    from deeprob.hip import clt
    dev = data if isinstance(data, DeviceRows) else DeviceRows(data)
    ones = clt.pair_counts(dev.planes).cpu().numpy().astype(np.int64)
    mut_info = compute_mutual_information(*priors_joints_from_counts(ones, dev.shape[0], alpha))
    total = np.sum(mut_info, axis=0)
    order, remaining, take = [], list(range(dev.shape[1])), conj_len - 1
    while remaining:
        head = remaining.pop(int(np.argmax(total[remaining])))
        if len(remaining) > take:
            group = [remaining[i] for i in np.argpartition(-mut_info[head][remaining], take)[:take]]
        else:
            group = list(remaining)
        order += [head] + group
        # (what is left is listed in the order of a Python set of ints, as in the reference: the order decides ties and
        # the order inside the next group)
        remaining = list(set(remaining) - set(group))
    return order


def build_trees_dict(n_vars: int, cl_parts_l: list, counts_l: list, conj_vars_l: list, alpha: float,
                     random_state: np.random.RandomState) -> dict:
    """``{scope length: [predecessors, scope]}``: one maximum spanning tree per conjunction and one over the variables
    in no conjunction, from the mutual information summed over the leaf partitions of ``cl_parts_l`` (lists of
    partitions; ``counts_l``: per list the ``[col_ids][:, col_ids]`` counts of its partitions), chained from the bottom
    of the circuit upwards: the root of a tree becomes a child of the root of the tree below it."""
    cumulative_info = np.zeros((n_vars, n_vars))
    for cl_parts, counts in zip(cl_parts_l, counts_l):
        for part, ones in zip(cl_parts, counts):
            mi = compute_mutual_information(*priors_joints_from_counts(ones, part.n_rows, alpha))
            cumulative_info[part.col_ids[:, None], part.col_ids] += mi
    # (a Python set of ints, as in the reference: its order is the order of the free variables in their tree's scope)
    free_vars = list(set(np.arange(n_vars)) - set([var for conj_vars in conj_vars_l for var in conj_vars]))
    scopes = conj_vars_l + [free_vars] if free_vars else conj_vars_l
    trees = []
    for scope in scopes:
        _, tree = maximum_spanning_tree(root=scope.index(random_state.choice(scope)),
                                        adj_matrix=cumulative_info[scope][:, scope])
        trees.append([int(t) for t in tree])
    # from the bottom of the circuit upwards: before a conjunction's tree is put on top, what is below it is an entry
    chain, below, out = list(trees[-1]), [int(v) for v in scopes[-1]], {}
    for tree, scope in zip(trees[-2::-1], scopes[-2::-1]):
        out[len(below)] = [list(chain), list(below)]
        shift = len(below)
        chain[chain.index(ROOT)] = shift + tree.index(ROOT)
        chain += [ROOT if t == ROOT else t + shift for t in tree]
        below += [int(v) for v in scope]
    return out


def _bernoulli(var, p):
    return new_node('Bernoulli', [int(var)], params={'p': float(p)})


def _product(children):
    return dict(new_node('Product', [v for c in children for v in c['scope']]), children=list(children))


def _naive(scope, ones, n, alpha):
    """``learn_mle`` with Bernoulli leaves: ``p = (ones + alpha) / (n + 2 alpha)`` per variable."""
    leaves = [_bernoulli(v, (int(c) + alpha) / (n + 2 * alpha)) for v, c in zip(scope, ones)]
    return leaves[0] if len(leaves) == 1 else _product(leaves)


def build_leaf(part: Partition, use_clt: bool, trees_dict: Optional[dict], det: bool, alpha: float, counts, leaf_root):
    """The node records of the leaf of ``part``.  A partition over conjunction variables is built from its histogram
    (``part.code_counts``); any other from ``counts``, the co-occurrence counts of its rows over its own columns -- or,
    with ``trees_dict``, over the scope of ``trees_dict[len(part.col_ids)]``.  ``leaf_root()`` draws the root position
    of a Chow-Liu leaf without a given tree."""
    scope = part.col_ids.tolist()
    if part.is_conj:
        code = int(np.flatnonzero(part.code_counts[1])[0])
        return _product([_bernoulli(v, a) for v, a in zip(scope, part.assignment_of(code))])
    if part.is_naive:
        hist = part.code_counts[1]
        if not det or part.disc_assignments.shape[0] == 2 ** part.disc_assignments.shape[1]:
            table = np.array([part.assignment_of(code) for code in range(len(hist))], np.int64)
            return _naive(scope, hist @ table, part.n_rows, alpha)
        # a disjunction of the assignments no sibling took: the weights are their smoothed counts
        code_of = {part.assignment_of(code): code for code in range(len(hist))}
        weights = np.array([hist[code_of[tuple(a)]] for a in part.disc_assignments.tolist()], np.float64)
        weights = (weights + alpha) / (weights + alpha).sum()
        products = [_product([_bernoulli(v, a) for v, a in zip(scope, assignment)])
                    for assignment in part.disc_assignments.tolist()]
        if len(products) == 1:
            return products[0]
        return dict(new_node('Sum', scope, weights=weights), children=products)
    if not use_clt:
        return _naive(scope, np.diag(counts), part.n_rows, alpha)
    if trees_dict is not None:
        tree, scope = trees_dict[len(scope)]
        leaf = BinaryCLT(scope, tree=list(tree))
    else:
        leaf = BinaryCLT(scope, root=scope[leaf_root(len(scope))])
    leaf.fit_counts(counts, part.n_rows, alpha=0.01)
    return leaf.to_pc_nodes()


def build_xpc(part_root: Partition, trees_dict: Optional[dict], det: bool, use_clt: bool, alpha: float, counts_of,
              leaf_root) -> dict:
    """The node records of the circuit of a partition tree, bottom up in the reference's post order: a Sum weighted by
    the row shares for a horizontal split, a Product for a vertical one -- a child that is a Product (or a Sum with one
    child) is replaced by its children, as the reference flattens them; the circuit of a Chow-Liu leaf is rooted at a Sum
    with two children and stays whole, as the reference's leaf does -- and ``build_leaf`` at the leaves.
    ``counts_of(part)``: the counts ``build_leaf`` takes."""
    done, stack = {}, [(part_root, False)]
    while stack:
        part, expanded = stack.pop()
        if not part.is_partitioned():
            done[id(part)] = build_leaf(part, use_clt, trees_dict, det, alpha,
                                        None if part.is_naive else counts_of(part), leaf_root)
        elif not expanded:
            stack.append((part, True))
            stack.extend((sub, False) for sub in part.sub_partitions[::-1])
        else:
            kids = [done.pop(id(sub)) for sub in part.sub_partitions]
            if part.is_horizontally_partitioned():
                weights = [sub.n_rows / part.n_rows for sub in part.sub_partitions]
                done[id(part)] = dict(new_node('Sum', kids[0]['scope'], weights=weights), children=kids)
            else:
                flat = []
                for c in kids:
                    if c['class'] == 'Product' or (c['class'] == 'Sum' and len(c['children']) == 1):
                        flat.extend(c['children'])
                    else:
                        flat.append(c)
                done[id(part)] = _product(flat)
    return done[id(part_root)]


def _counts_for(leaf_counts, parts, trees_dict, use_clt, own) -> dict:
    """``{id(part): counts}`` for ``build_leaf``: over the scope of the given tree, or the partition's own block."""
    if trees_dict is not None and use_clt:
        return leaf_counts.blocks(lambda p: trees_dict[len(p.col_ids)][1], parts)
    return own


def learn_xpc(data, det: bool, sd: bool, min_part_inst: int, conj_len: int, arity: int, n_max_parts: int = 200,
              use_clt: bool = True, use_greedy_ordering: Optional[bool] = False, alpha: float = 0.01,
              random_seed: int = 42) -> Tuple['FlatSpn', dict]:
    """
    Learn an eXtremely randomized Probabilistic Circuit (XPC).

    :param data: The binary training data ``[N, D]``: a numpy array or a device tensor.
    :param det: True to force determinism, False otherwise.
    :param sd: True to force structured decomposability, False otherwise.
    :param min_part_inst: The minimum number of instances allowed per partition.
    :param conj_len: The conjunction length, ``1 .. DPC_XPC_MAX_CONJ``.
    :param arity: The maximum number of children for a sum node.
    :param n_max_parts: The maximum number of partitions for the partitions tree.
    :param use_clt: True to use CLTrees as multivariate leaves, False otherwise.
    :param use_greedy_ordering: True to use a greedy ordering, False otherwise.
    :param alpha: Laplace smoothing factor.
    :param random_seed: The seed of the learner's generator and of the generator of the leaf roots.
    :return: ``(circuit, utils)``: the ``FlatSpn`` and ``part_root``, ``cl_parts_l``, ``conj_vars_l``, ``n_parts``,
             ``trees_dict``.
    :raises ValueError: If an argument is out of domain, the data are not binary or no partitioning is found.
    """
    _check(conj_len, arity, min_part_inst, det, use_clt)
    if not sd and use_greedy_ordering:
        raise ValueError("Using the greedy ordering makes sense only if sd = True.")
    clock = _Clock()
    dev = DeviceRows(data)
    clock.device = dev.x.device
    clock.lap('pack')
    random_state = np.random.RandomState(random_seed)
    leaf_state = np.random.RandomState(random_seed)
    if use_greedy_ordering:
        ordering = greedy_vars_ordering(dev, conj_len)
    else:
        ordering = np.arange(dev.shape[1]).tolist()
        random_state.shuffle(ordering)
    part_root, cl_parts_l, conj_vars_l, n_parts = generate_random_partitioning(
        data=dev, sd=sd, min_part_inst=min_part_inst, conj_len=conj_len, arity=arity, n_max_parts=n_max_parts,
        uncond_vars=ordering, random_state=random_state)
    clock.lap('partition')
    if n_parts <= 1:
        raise ValueError("No partitioning found.")
    leaf_counts = _LeafCounts(dev, cl_parts_l)
    own = leaf_counts.blocks(lambda p: p.col_ids)
    clock.lap('leaf_counts')
    trees_dict = None
    if sd and use_clt:
        trees_dict = build_trees_dict(dev.shape[1], [cl_parts_l], [[own[id(p)] for p in cl_parts_l]], conj_vars_l, alpha,
                                      random_state)
        clock.lap('host')
    counts = _counts_for(leaf_counts, cl_parts_l, trees_dict, use_clt, own)
    clock.lap('leaf_counts')
    utils = {'part_root': part_root, 'cl_parts_l': cl_parts_l, 'conj_vars_l': conj_vars_l, 'n_parts': n_parts,
             'trees_dict': trees_dict}
    xpc = to_flat(build_xpc(part_root, trees_dict, det, use_clt, alpha, lambda p: counts[id(p)],
                            lambda k: int(leaf_state.choice(k))))
    clock.lap('host')
    _profile.clear()
    _profile.update(clock.times)
    return xpc, utils


def learn_expc(data, ensemble_dim: int, det: bool, sd_level: int, min_part_inst: int, conj_len: int, arity: int,
               n_max_parts: int = 200, use_clt: bool = True, alpha: float = 0.01, random_seed: int = 42
               ) -> Tuple['FlatSpn', list]:
    """
    Learn an Ensemble (i.e. a uniform mixture) of eXtremely randomized Probabilistic Circuits (EXPC).

    :param data: The binary training data ``[N, D]``: a numpy array or a device tensor.
    :param ensemble_dim: The number of circuits in the mixture.
    :param det: True to force determinism, False otherwise.
    :param sd_level: 0 a non-SD ensemble of non-SD PCs, 1 a non-SD ensemble of SD PCs, 2 an SD ensemble.
    :param min_part_inst: The minimum number of instances allowed per partition.
    :param conj_len: The conjunction length, ``1 .. DPC_XPC_MAX_CONJ``.
    :param arity: The maximum number of children for a sum node.
    :param n_max_parts: The maximum number of partitions for the partitions tree.
    :param use_clt: True to use CLTrees as multivariate leaves, False otherwise.
    :param alpha: Laplace smoothing factor.
    :param random_seed: The seed of the learner's generator and of the generator of the leaf roots.
    :return: ``(circuit, [utils, ...])``: the ``FlatSpn`` of the mixture and one ``utils`` of ``learn_xpc`` per member.
    :raises ValueError: If an argument is out of domain, the data are not binary or no partitioning is found.
    """
    if sd_level not in SD_LEVELS:
        raise ValueError("Choose a value in {0, 1, 2}.")
    _check(conj_len, arity, min_part_inst, det, use_clt)
    if ensemble_dim < 1:
        raise ValueError("ensemble_dim must be at least 1")
    if sd_level == SD_LEVEL_2 and conj_len == 1:
        raise ValueError("No randomness in this setting. Change hyper parameters.")
    clock = _Clock()
    dev = DeviceRows(data)
    clock.device = dev.x.device
    clock.lap('pack')
    random_state = np.random.RandomState(random_seed)
    leaf_state = np.random.RandomState(random_seed)
    sd = sd_level in (SD_LEVEL_1, SD_LEVEL_2)
    ordering = greedy_vars_ordering(dev, conj_len) if sd_level == SD_LEVEL_2 else np.arange(dev.shape[1]).tolist()
    members = []
    for _ in range(ensemble_dim):
        if sd_level != SD_LEVEL_2:
            np.random.shuffle(ordering)             # the GLOBAL generator, cumulatively and in place, as the reference
        members.append(generate_random_partitioning(
            data=dev, sd=sd, min_part_inst=min_part_inst, conj_len=conj_len, arity=arity, n_max_parts=n_max_parts,
            uncond_vars=ordering, random_state=random_state))
    clock.lap('partition')
    if all(n_parts == 1 for _, _, _, n_parts in members):
        raise ValueError("No Partitioning Found")
    # the leaf partitions of all members: one generation of at most ensemble_dim x N rows
    leaf_counts = _LeafCounts(dev, [p for _, cl_parts, _, _ in members for p in cl_parts])
    own = leaf_counts.blocks(lambda p: p.col_ids)
    own_of = lambda parts: [own[id(p)] for p in parts]
    clock.lap('leaf_counts')
    n_vars = dev.shape[1]
    trees_dict_l = [None] * ensemble_dim
    if sd_level == SD_LEVEL_2 and use_clt:
        trees_dict = build_trees_dict(n_vars, [m[1] for m in members], [own_of(m[1]) for m in members],
                                      max([m[2] for m in members], key=len), alpha, random_state)
        trees_dict_l = [trees_dict] * ensemble_dim
    xpc_l = []
    for i, (part_root, cl_parts, conj_vars_l, _) in enumerate(members):
        if sd_level == SD_LEVEL_1 and use_clt:
            # (the reference draws a member's trees and builds the member before it draws the next member's trees; the
            # build draws nothing from `random_state`, so the draws are the same)
            trees_dict_l[i] = build_trees_dict(n_vars, [cl_parts], [own_of(cl_parts)], conj_vars_l, alpha, random_state)
        clock.lap('host')
        counts = _counts_for(leaf_counts, cl_parts, trees_dict_l[i], use_clt, own)
        clock.lap('leaf_counts')
        xpc_l.append(build_xpc(part_root, trees_dict_l[i], det, use_clt, alpha, lambda p: counts[id(p)],
                               lambda k: int(leaf_state.choice(k))))
        clock.lap('host')
    utils = [{'part_root': m[0], 'cl_parts_l': m[1], 'conj_vars_l': m[2], 'n_parts': m[3], 'trees_dict': trees_dict_l[i]}
             for i, m in enumerate(members)]
    root = dict(new_node('Sum', xpc_l[0]['scope'], weights=np.full(ensemble_dim, 1 / ensemble_dim)), children=xpc_l)
    expc = to_flat(root)
    clock.lap('host')
    _profile.clear()
    _profile.update(clock.times)
    return expc, utils
