"""``BinaryCNet``: the binary cutset network of the reference (deeprob/spn/structure/cnet.py) -- an OR tree that conditions
on one binary variable per node, with a :class:`~deeprob.spn.structure.cltree.BinaryCLT` at every leaf -- learned and
queried on the HIP device through ``libdeeprob_clt.so`` (the ``dpc_cnet_*`` entry points of include/deeprob_clt.h).

``fit`` is level synchronous: every open node of one depth is a task with a segment of a row-index array on the device;
per depth the rows are packed into bit planes through the index, the co-occurrence counts of every task are taken by
AND + popcount over its own words, the information gains are evaluated in float64 from those exact counts, and the
segments of the splitting tasks are partitioned stably by their cut column.  The host reads one small record per task
(:func:`stop_rule` decides on it, in the reference's order) and, for a leaf, the leaf's block of the counts, from which the
leaf's tree and tables come by ``BinaryCLT.fit_counts`` -- the host half of ``BinaryCLT.fit``.  The training rows never
come back.  ``log_likelihood`` is one thread per row: a complete row walks one path, a row with NaN walks the OR tree
depth first.  ``sample`` is the same walk in one launch (``dpc_cnq_sample``): every node returns its value and a leaf drawn
below it, a NaN OR node picks between its two sides with their posterior odds, and the NaN entries are filled along the one
path of the drawn leaf and inside it -- an exact draw from ``p(x_missing | x_observed)``, an all-NaN batch being unconditional
generation.  ``marginals`` is the walk taken twice in one launch (``dpc_mar_cnet``): the first gives ``log P(e)``, the second
weighs every consistent leaf with its posterior probability and adds the leaf's own posterior marginals, so that every
NaN entry comes back as ``p(x_j = 1 | x_observed)``, exact.  Inputs follow ``BinaryCLT``: numpy in, numpy out; a device tensor stays on its device; a CPU tensor or a
missing library raises ``HipError``.

Two deliberate differences from the reference, both in DESIGN.md §16.  ``fit`` takes ``random_state``: the reference lets
every leaf draw its root from an unseeded generator, here the roots are ``random_state.choice(len(leaf.scope))``, one per
leaf in breadth-first order, left child before right.  And in ``log_likelihood`` NaN means marginalised; the reference
silently drops a row from the sum at the first OR node whose variable is NaN (cnet.py:226-229).  The scores are float64
(the reference's are float32), which only matters where two gains tie to float32 precision.

The reference has neither ``sample`` nor ``mpe`` nor ``marginals`` for cutset networks, so there is nothing to reproduce: all
are exact here (the OR nodes are deterministic).  Exact MPE is built at kernel, ABI and binding level --
``deeprob.hip.cnet.mpe(model._on_device(device), x)``, ``dpc_cnq_mpe`` -- and the one-line ``mpe`` method on the class awaits
a follow-up.  The XPC learners are ``deeprob.spn.learning.xpc``.  The scored learners ``learn_cnet_bd`` / ``learn_cnet_bic`` are built in
``deeprob.spn.learning.cnet_bayesian`` and return a ``BinaryCNet``.
"""
import time
from typing import List, Optional, Union

import numpy as np

from deeprob.spn.structure.cltree import BinaryCLT
from deeprob.utils.random import RandomState, check_random_state


def stop_rule(n_samples: int, n_features: int, mean_entropy: Optional[float], max_gain: Optional[float],
              min_n_samples: int, min_n_features: int, min_mean_entropy: float) -> Optional[str]:
    """Why the open node with these numbers becomes a leaf, or None if it splits: the reference's rules in the reference's
    order (cnet.py:109-117).  'samples' / 'features' need no scores (``mean_entropy`` and ``max_gain`` may be None);
    then 'entropy' (``mean_entropy < min_mean_entropy``) and 'gain' (``max_gain <= 0``)."""
    if n_samples <= min_n_samples:
        return 'samples'
    if n_features <= min_n_features:
        return 'features'
    if mean_entropy < min_mean_entropy:
        return 'entropy'
    if max_gain <= 0:
        return 'gain'
    return None


class ORNode:
    def __init__(
        self,
        scope: Optional[List[int]],
        children: Optional[list] = None,
        weights: Optional[Union[List[float], np.ndarray]] = None,
        or_id: Optional[int] = None
    ):
        """
        Initialize an OR node.

        :param scope: The scope of the OR node.
        :param children: The two child nodes, for ``or_id`` = 0 and = 1.
        :param weights: The weights of the OR node.
        :param or_id: The variable the OR node conditions on.
        :raises ValueError: If the weights do not sum to 1.
        """
        if weights is not None:
            if isinstance(weights, list):
                weights = np.array(weights, dtype=np.float32)
            if not np.isclose(np.sum(weights), 1.0):
                raise ValueError("Weights don't sum up to 1")
        self.scope = scope
        self.children = children if children is not None else []
        self.weights = weights
        self.or_id = or_id
        self.clt = None


class BinaryCNet(ORNode):
    def __init__(
        self,
        scope: Optional[List[int]],
        children: Optional[list] = None,
        weights: Optional[Union[List[float], np.ndarray]] = None,
        or_id: Optional[int] = None
    ):
        """
        Initialize a binary cutset network (CNet).

        :param scope: The scope of the binary CNet.
        :param children: The child OR nodes of the binary CNet.
        :param weights: The weights of the current OR node.
        :param or_id: The id of the current OR node.
        """
        super().__init__(scope, children, weights, or_id)

    # ---- learning ----------------------------------------------------------------------------------------------------
    def fit(
        self,
        data,
        alpha: float = 0.01,
        min_n_samples: int = 10,
        min_n_features: int = 1,
        min_mean_entropy: float = 0.01,
        random_state: Optional[RandomState] = None
    ):
        """
        Fit the structure and the parameters to binary training data.

        :param data: The training data ``[N, D]``, every value 0 or 1: a numpy array or a device tensor.
        :param alpha: The Laplace smoothing factor.
        :param min_n_samples: A node with this many rows or fewer is a leaf.
        :param min_n_features: A node with this many variables or fewer is a leaf (at least 1).
        :param min_mean_entropy: A node whose mean entropy is below this is a leaf.
        :param random_state: None, a seed or a Numpy RandomState: draws the root of every leaf's tree.
        :raises ValueError: If a parameter is out of domain or the data are not binary.
        """
        import torch
        from deeprob.hip import cnet
        from deeprob.utils.statistics import device_training_rows
        if alpha < 0.0:
            raise ValueError("The Laplace smoothing factor must be non-negative")
        if min_n_samples < 0 or min_n_features < 1:
            raise ValueError("min_n_samples must be non-negative and min_n_features at least 1")
        random_state = check_random_state(random_state)
        x = device_training_rows(data)
        t_start, t_host = time.perf_counter(), 0.0
        n_rows, d = x.shape
        self.scope, self.children, self.weights, self.or_id, self.clt = list(range(d)), [], None, None, None

        rows = torch.arange(n_rows, dtype=torch.int32, device=x.device)
        tasks = [(self, n_rows, np.arange(d))]          # (node, rows, active columns), in the order of the reference's queue
        n_generations = 0
        while tasks:
            n_generations += 1
            gen = cnet.Generation(x, rows, [n for _, n, _ in tasks])
            gen.pack()
            cut = np.full(len(tasks), -1, np.int64)
            next_tasks = []
            step = cnet.chunk_tasks(d)
            for t0 in range(0, len(tasks), step):
                chunk = tasks[t0:t0 + step]
                active = np.zeros((len(chunk), d), np.uint8)
                for i, (_, _, cols) in enumerate(chunk):
                    active[i, cols] = 1
                ones = gen.counts(t0, len(chunk))
                _, stats, best = gen.scores(ones, t0, active, alpha)
                stats, best = stats.cpu().numpy(), best.cpu().numpy()         # the record: one read per chunk
                leaves = []
                for i, (node, n, cols) in enumerate(chunk):
                    why = stop_rule(n, len(cols), float(stats[i, 0]), float(stats[i, 1]), min_n_samples, min_n_features,
                                    min_mean_entropy)
                    if why is not None:
                        leaves.append((i, node, n, cols))
                        continue
                    column, n_right = int(best[i, 0]), int(best[i, 1])
                    left_weight = (n - n_right + alpha) / (n + 2 * alpha)
                    scope = [v for v in node.scope if v != column]
                    node.children = [BinaryCNet(scope), BinaryCNet(scope)]
                    node.weights, node.or_id = [left_weight, 1 - left_weight], column
                    cut[t0 + i] = column
                    rest = cols[cols != column]
                    next_tasks += [(node.children[0], n - n_right, rest), (node.children[1], n_right, rest)]
                if leaves:
                    # the [d_leaf, d_leaf] blocks of the leaves' counts, gathered on the device, in one read
                    index = np.concatenate([((i * d + cols[:, None]) * d + cols[None, :]).reshape(-1)
                                            for i, _, _, cols in leaves])
                    blocks = ones.reshape(-1)[torch.from_numpy(index).to(x.device)].cpu().numpy().astype(np.int64)
                    t0_host, at = time.perf_counter(), 0
                    for _, node, n, cols in leaves:
                        k = len(cols)
                        node.clt = BinaryCLT(node.scope, root=node.scope[int(random_state.choice(k))])
                        node.clt.fit_counts(blocks[at:at + k * k].reshape(k, k), n, alpha=alpha)
                        at += k * k
                    t_host += time.perf_counter() - t0_host
            if not next_tasks:
                break
            rows, _ = gen.partition(cut)
            tasks = next_tasks
        torch.cuda.synchronize(x.device)
        total = time.perf_counter() - t_start
        #: where the last ``fit`` spent its time: the leaves' host learning, and the rest (device generations and records)
        self.fit_profile_ = {'seconds': total, 'host_leaf_seconds': t_host, 'generations_seconds': total - t_host,
                             'generations': n_generations}
        return self

    # ---- queries -----------------------------------------------------------------------------------------------------
    def _nodes(self):
        """The OR nodes breadth first, left child before right."""
        order, at = [self], 0
        while at < len(order):
            node = order[at]
            at += 1
            if node.clt is None:
                if node.children is None or len(node.children) != 2 or node.weights is None or node.or_id is None:
                    raise ValueError("The CNet's structure and parameters must be already initialized")
                order += node.children
        return order

    def _on_device(self, device):
        """The model as tables on ``device`` (uploaded per call, one copy: the arrays are public)."""
        from deeprob.hip import cnet
        nodes = self._nodes()
        number = {id(node): k for k, node in enumerate(nodes)}
        column = {v: c for c, v in enumerate(self.scope)}
        col, child, logw, leaves = [], [], [], []
        for node in nodes:
            if node.clt is not None:
                if node.clt.tree is None or node.clt.params is None:
                    raise ValueError("The CNet's structure and parameters must be already initialized")
                col.append(-1)
                child.append([len(leaves), -1])
                logw.append([0.0, 0.0])
                leaves.append(([column[v] for v in node.clt.scope], node.clt.bfs, node.clt.tree, node.clt.params))
            else:
                col.append(column[node.or_id])
                child.append([number[id(c)] for c in node.children])
                with np.errstate(divide='ignore'):
                    logw.append(np.log(np.asarray(node.weights, np.float64)))
        return cnet.DeviceCNet(len(self.scope), col, child, logw, leaves, device)

    def _run(self, op, x, *args):
        """``op(tables on the device, x on the device, *args)`` under the input rules of the module docstring."""
        from deeprob.hip import clt
        return clt.run_on_device(self, 'BinaryCNet', op, x, *args)

    def log_likelihood(self, x):
        """``[B]`` float32 log likelihoods; NaN entries are marginalised."""
        from deeprob.hip import cnet
        return self._run(cnet.log_likelihood, x)

    def sample(self, x, seed: Optional[int] = None):
        """A copy of ``x`` ``[B, D]`` with every NaN entry drawn, the row as a whole an exact draw from the posterior given
        its observed entries (which come back bit for bit); an all-NaN batch is unconditional generation.  ``seed``: the
        seed of the counter-based generator (the same seed gives the same bytes, whatever the batch a row comes in at the
        same position); None draws one from numpy's global generator."""
        from deeprob.hip import cnet
        # (what is wrong with the call itself is reported before what is wrong with where the rows live)
        if any(node.clt is not None and (node.clt.tree is None or node.clt.params is None) for node in self._nodes()):
            raise ValueError("The CNet's structure and parameters must be already initialized")
        if len(x.shape) != 2 or x.shape[1] != len(self.scope):
            raise ValueError("expected inputs [B, {}], got {}".format(len(self.scope), tuple(x.shape)))
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        return self._run(cnet.sample, x, int(seed))

    def marginals(self, x):
        """A copy of ``x`` ``[B, D]`` with every NaN entry replaced by ``p(x_j = 1 | the row's observed entries)``, exact.
        Observed entries come back bit for bit; an all-NaN row gives the prior marginals; a row whose evidence has
        probability zero gets NaN in its unobserved entries."""
        from deeprob.hip import cnet
        # (what is wrong with the call itself is reported before what is wrong with where the rows live)
        if any(node.clt is not None and (node.clt.tree is None or node.clt.params is None) for node in self._nodes()):
            raise ValueError("The CNet's structure and parameters must be already initialized")
        if len(x.shape) != 2 or x.shape[1] != len(self.scope):
            raise ValueError("expected inputs [B, {}], got {}".format(len(self.scope), tuple(x.shape)))
        return self._run(cnet.marginals, x)

    def likelihood(self, x):
        ll = self.log_likelihood(x)
        return np.exp(ll) if isinstance(ll, np.ndarray) else ll.exp()

    def params_count(self) -> int:
        """The OR weights plus the parameters of the leaves' trees."""
        return sum(node.clt.params_count() if node.clt is not None else len(node.weights) for node in self._nodes())
