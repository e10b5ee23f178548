"""``BinaryCLT``: the binary Chow-Liu tree of the reference (deeprob/spn/structure/cltree.py) as a stand-alone density
estimator, learned and queried on the HIP device through ``libdeeprob_clt.so`` (include/deeprob_clt.h).

``fit`` counts on the device (``dpc_pack_bits``, ``dpc_pair_counts``) and finishes on the host: float32 priors, joints
and mutual information in the reference's expressions from exact integer counts, Prim's maximum spanning tree, the
conditional tables.  ``log_likelihood``, ``mpe``, ``sample`` and ``marginals`` (the exact posterior marginal of every NaN
entry, which the reference does not have) run one thread per row on the device.  Inputs follow
``deeprob.spn.algorithms.inference.log_likelihood``: a numpy array is evaluated on the current HIP device and numpy comes
back, a device tensor stays on its device, a CPU tensor or a missing library raises ``HipError``.

Two deliberate differences from the reference, both documented in DESIGN.md ("Chow-Liu trees"):
``bfs`` is breadth first with children in increasing index (the reference's comes from scipy's sparse storage order);
it only fixes the order of float32 additions.  ``sample`` draws from a counter-based generator with an explicit ``seed``
(the reference uses scipy's global generator and cannot be replayed).

``FlatSpn`` has no multivariate leaf, so the class is never a node of a node-graph SPN here: ``learn_spn`` with
``learn_leaf=deeprob.spn.learning.leaf.learn_binary_clt`` (the function, by identity; the string ``'binary-clt'`` still
raises) fits one tree per multivariate leaf task from counts taken on the learner's own data layout (``fit_counts``) and
hangs its ``to_pc_nodes()`` expansion into the circuit; EM on such a circuit updates the expansion's sum weights freely.
The reference's ``em_init`` / ``em_step`` keep the CPTs of a tree tied: ``em_step`` takes the weighted counts of its rows
from one ``dpc_mix_em_stats`` launch and applies the reference's float32 update (:func:`em_update`) on the host;
``deeprob.spn.structure.cltmix.BinaryCLTMixture`` trains a mixture of trees with them.
"""
from typing import List, Optional, Union

import numpy as np

from deeprob.spn.structure.leaf import Leaf, LeafType
from deeprob.utils.random import RandomState, check_random_state
from deeprob.utils.graph import build_tree_structure, compute_bfs_ordering, maximum_spanning_tree
from deeprob.utils.statistics import compute_mutual_information, pair_counts, priors_joints_from_counts


def _post_order(root):
    """The ``TreeNode``s under ``root`` as the reference's explicit stack visits them (cltree.py:365-392): a node after
    its children, the children of a node from the last to the first."""
    out, stack = [], [(root, False)]
    while stack:
        node, expanded = stack.pop()
        if expanded or node.is_leaf():
            out.append(node)
        else:
            stack.append((node, True))
            stack.extend((c, False) for c in node.get_children())
    return out


def em_update(params: np.ndarray, tree: np.ndarray, root: int, stats: np.ndarray, step_size: float) -> np.ndarray:
    """The tied-CPT EM update of one tree (cltree.py:131-155) in float32 and in the reference's order, as a pure function:
    the new log CPTs ``[D, 2, 2]`` from the current ``params``, the predecessors ``tree``, the position ``root`` and the
    tree's row ``stats`` ``[1 + 2 D]`` of ``dpc_mix_em_stats`` (the sum of the responsibilities, their sums where
    ``x_j = 1`` and where ``x_j = x_parent(j) = 1``), which stand where the reference sums ``stats * data`` itself."""
    f32 = np.float32
    params, tree, stats = np.asarray(params, f32), np.asarray(tree), np.asarray(stats)
    d = len(tree)
    smooth = f32(np.finfo(np.float16).eps)          # 2^-10: the reference smooths the weighted counts this lightly
    mass = f32(stats[0])                            # the batch's responsibility for this tree
    on = stats[1:1 + d].astype(f32)                 # ... where x_j = 1
    on_both = stats[1 + d:1 + 2 * d].astype(f32)    # ... where x_j = 1 and x_parent(j) = 1

    # P(x_j = 1) and its complement, column 1 first
    p_on = (on + f32(2) * smooth) / (mass + f32(4) * smooth)
    marginal = np.stack([f32(1) - p_on, p_on], axis=1)

    # fresh[j, l, 1] = P(x_j = 1 | x_parent(j) = l): the count of (x_j = 1, x_parent = l) over the parent's smoothed mass;
    # the entry of the root's row is indexed with -1 and overwritten below
    count = np.stack([on - on_both, on_both], axis=1)
    fresh = np.empty((d, 2, 2), f32)
    fresh[:, :, 1] = (count + smooth) / (mass * marginal[tree] + f32(4) * smooth)
    fresh[:, :, 0] = f32(1) - fresh[:, :, 1]
    fresh[root] = marginal[root]                    # both rows of the root hold its marginal

    # a step of step_size from the current tables towards the fresh ones, in probability space, rows summing to 1 again
    blend = f32(1.0 - step_size) * np.exp(params) + f32(step_size) * fresh
    blend /= blend.sum(axis=2, keepdims=True)
    with np.errstate(divide='ignore'):
        return np.log(blend)


class BinaryCLT(Leaf):
    LEAF_TYPE = LeafType.DISCRETE

    def __init__(
        self,
        scope: List[int],
        root: Optional[int] = None,
        tree: Optional[Union[List[int], np.ndarray]] = None,
        params: Optional[Union[List[List[List[float]]], np.ndarray]] = None
    ):
        """
        Initialize a Binary Chow-Liu Tree (CLT).

        :param scope: The scope: the ids of the variables.
        :param root: The root variable (an id of the scope). If None, ``fit`` draws it.
        :param tree: The predecessors, as positions in the scope, -1 at the root.
        :param params: The conditional probability tables as a (N, 2, 2) array in log space,
                       ``params[i, l, k] = log P(X_i=k | Pa(X_i)=l)``.
        :raises ValueError: If the root variable is not in scope.
        :raises ValueError: If the tree is not compatible with the number of variables and the root.
        :raises ValueError: If the CPTs are invalid.
        """
        scope = [scope] if isinstance(scope, int) else list(scope)
        if len(scope) == 0:
            raise ValueError("The scope must not be empty")
        if len(set(scope)) != len(scope):
            raise ValueError("The scope must not contain duplicates")
        self.scope = scope

        if root is not None and tree is None:
            if root not in scope:
                raise ValueError("The root variable must be in scope")
            root = scope.index(root)
        bfs = None
        if tree is not None:
            if isinstance(tree, list):
                tree = np.array(tree, dtype=np.int32)
            if len(tree) != len(scope):
                raise ValueError("Invalid tree structure's number of variables")
            if root is None:
                roots = np.flatnonzero(tree == -1)
                if len(roots) != 1:
                    raise ValueError("Invalid tree structure's root node")
                root = int(roots[0])
            else:
                if root not in scope:
                    raise ValueError("The root variable must be in scope")
                root = scope.index(root)
            if tree[root] != -1:
                raise ValueError("Invalid tree structure's root node")
            bfs = compute_bfs_ordering(tree)
        self.root, self.tree, self.bfs = root, tree, bfs

        if isinstance(params, list):
            params = np.array(params, dtype=np.float32)
            if params.shape != (len(scope), 2, 2):
                raise ValueError("Invalid conditional probability table (CPT) shape")
            if not np.allclose(np.exp(params).sum(axis=2), 1.0):
                raise ValueError("Invalid conditional probability table (CPT) values")
        self.params = params

    # ---- learning ----------------------------------------------------------------------------------------------------
    @staticmethod
    def compute_clt_parameters(bfs: np.ndarray, tree: np.ndarray, priors: np.ndarray, joints: np.ndarray) -> np.ndarray:
        """The CPTs (not in log space) of a tree from priors and joints (cltree.py:105-115):
        ``params[i, l, k] = P(X_i=k | Pa(X_i)=l)``; both rows of the root hold its prior."""
        tree = np.asarray(tree)
        me = np.arange(len(bfs))
        pair = joints[me, tree]                              # [i, k, l] = P(X_i=k, X_pa=l); the root's row is overwritten
        inverse = np.reciprocal(priors[tree])                # [i, l]
        params = pair.transpose(0, 2, 1) * inverse[:, :, None]
        params[bfs[0]] = priors[bfs[0]]
        # float32 rounding leaves the rows a little off 1
        params /= np.sum(params, axis=2, keepdims=True)
        return params

    def fit(self, data, domain: List[list], alpha: float = 0.1, random_state: Optional[RandomState] = None, **kwargs):
        """
        Fit the structure (unless a tree was given) and the parameters to binary training data.

        :param data: The training data ``[N, len(scope)]``, every value 0 or 1: a numpy array or a device tensor.
        :param domain: The domains of the variables, ``[0, 1]`` each.
        :param alpha: The Laplace smoothing factor.
        :param random_state: None, a seed or a Numpy RandomState: draws the root when none was given.
        :raises ValueError: If a parameter is out of domain or the data are not binary.
        """
        if len(data.shape) != 2 or len(domain) != data.shape[1]:
            raise ValueError("Each data column should correspond to a random variable having a domain")
        if not all(d == [0, 1] for d in domain):
            raise ValueError("The domains must be binary for a Binary CLT distribution")
        if alpha < 0.0:
            raise ValueError("The Laplace smoothing factor must be non-negative")
        if data.shape[1] != len(self.scope):
            raise ValueError("expected data [N, {}], got {}".format(len(self.scope), tuple(data.shape)))
        random_state = check_random_state(random_state)
        if self.root is None:
            self.root = int(random_state.choice(len(self.scope)))

        self.fit_counts(*pair_counts(data), alpha=alpha)

    def fit_counts(self, ones: np.ndarray, n_samples: int, alpha: float = 0.1):
        """The host part of ``fit``: structure (unless a tree was given) and parameters from the exact co-occurrence counts
        ``ones`` ``[len(scope), len(scope)]`` of ``n_samples`` rows.  ``root`` must be set."""
        priors, joints = priors_joints_from_counts(ones, n_samples, alpha=alpha)
        if self.tree is None:
            self.bfs, self.tree = maximum_spanning_tree(self.root, compute_mutual_information(priors, joints))
        with np.errstate(divide='ignore'):      # (alpha = 0 can leave a zero probability)
            self.params = np.log(self.compute_clt_parameters(self.bfs, self.tree, priors, joints))

    def em_init(self, random_state: np.random.RandomState):
        """Random CPTs for EM (cltree.py:117-125): ``rand(len(scope), 2)``, the two rows of the root made equal."""
        if self.tree is None:
            raise ValueError("The CLT's structure must be already initialized")
        p_on = random_state.rand(len(self.scope), 2)          # P(x_j = 1 | parent value l), one draw per (j, l)
        p_on[self.root, 0] = p_on[self.root, 1]
        self.params = np.log(np.stack([1.0 - p_on, p_on], axis=2).astype(np.float32))

    def em_step(self, stats, data, step_size: float):
        """One batch EM step with tied CPTs (cltree.py:127-155).  ``stats`` ``[B]``: the responsibility of the tree for
        every row of ``data`` ``[B, len(scope)]`` (complete 0 / 1 rows; both numpy or both tensors on one HIP device).  The
        weighted counts are one ``dpc_mix_em_stats`` launch with one component, the update is :func:`em_update`."""
        if self.tree is None:
            raise ValueError("The CLT's structure must be already initialized")
        if self.params is None:
            raise ValueError("The CLT's structure and parameters must be already initialized")
        import torch
        from deeprob.hip import clt
        if len(data.shape) != 2 or data.shape[1] != len(self.scope) or tuple(stats.shape) not in ((data.shape[0],), (data.shape[0], 1)):
            raise ValueError("expected data [B, {}] and stats [B], got {} and {}".format(len(self.scope), tuple(data.shape),
                                                                                      tuple(stats.shape)))
        x, resp = clt.rows_on_device(data, 'BinaryCLT'), clt.rows_on_device(stats, 'BinaryCLT').reshape(-1, 1)
        if bool(torch.isnan(x).any()):
            raise ValueError("The data contains NaN: EM needs complete rows")
        mix = clt.DeviceMixture([(self.bfs, self.tree, self.params)], [0.0], x.device)
        row = clt.mixture_em_stats(mix, clt.pack_query(x), None, resp).cpu().numpy()[0]
        self.params = em_update(self.params, self.tree, self.root, row, step_size)

    # ---- queries -----------------------------------------------------------------------------------------------------
    def _on_device(self, device):
        from deeprob.hip import clt
        if self.tree is None or self.params is None:
            raise ValueError("The CLT's structure and parameters must be already initialized")
        # (uploaded per call, one small copy: `params` is a public array a caller may write into)
        return clt.DeviceTree(self.bfs, self.tree, self.params, device)

    def _run(self, op, x, *args):
        """``op(tree, x on the device, *args)`` under the input rules of the module docstring."""
        from deeprob.hip import clt
        return clt.run_on_device(self, 'BinaryCLT', op, x, *args)

    def log_likelihood(self, x):
        """``[B, 1]`` float32 log likelihoods; NaN entries are marginalised."""
        from deeprob.hip import clt
        return self._run(clt.log_likelihood, x).reshape(-1, 1)

    def likelihood(self, x):
        ll = self.log_likelihood(x)
        return np.exp(ll) if isinstance(ll, np.ndarray) else ll.exp()

    def mpe(self, x):
        """A copy of ``x`` with every NaN entry filled by the most probable completion given the observed entries."""
        from deeprob.hip import clt
        return self._run(clt.mpe, x)

    def sample(self, x, seed: Optional[int] = None):
        """A copy of ``x`` with every NaN entry drawn given the observed entries.  ``seed``: the seed of the counter-based
        generator (the same seed gives the same bytes); None draws one from numpy's global generator."""
        from deeprob.hip import clt
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        return self._run(clt.sample, x, int(seed))

    def marginals(self, x):
        """A copy of ``x`` ``[B, D]`` with every NaN entry replaced by ``p(x_j = 1 | the row's observed entries)``, exact: one
        upward and one downward pass per row.  Observed entries come back bit for bit; an all-NaN row gives the prior
        marginals; a row whose evidence has probability zero gets NaN in its unobserved entries."""
        from deeprob.hip import clt
        # (what is wrong with the call itself is reported before what is wrong with where the rows live)
        if self.tree is None or self.params is None:
            raise ValueError("The CLT's structure and parameters must be already initialized")
        if len(x.shape) != 2 or x.shape[1] != len(self.scope):
            raise ValueError("expected inputs [B, {}], got {}".format(len(self.scope), tuple(x.shape)))
        return self._run(clt.marginals, x)

    def moment(self, k: int = 1) -> float:
        raise NotImplementedError("Computation of moments on Binary CLTs not yet implemented")

    # ---- parameters and structure ------------------------------------------------------------------------------------
    def params_count(self) -> int:
        return 1 + len(self.tree) + self.params.size

    def params_dict(self) -> dict:
        return {'root': None if self.root is None else self.scope[self.root], 'tree': self.tree, 'params': self.params}

    def to_pc(self):
        """
        The smooth, deterministic and structured-decomposable circuit equivalent to the tree (cltree.py:352-395), as a
        :class:`deeprob.spn.structure.io.FlatSpn` with ids in ``assign_ids`` order.

        Variable v becomes two indicator leaves and, under each value l of its parent, a sum node with the weights
        ``exp(params[v][l])`` over the two (a leaf of the tree) or over two products "indicator x the children's sums for
        this value".  The circuit's root is the sum for l = 1 of the tree's root.
        """
        from deeprob.spn.learning.learnspn import to_flat
        return to_flat(self.to_pc_nodes())

    def to_pc_nodes(self) -> dict:
        """The circuit of :meth:`to_pc` as the node records ``to_flat`` takes (``learnspn.new_node``): its root, a Sum.  A
        learner that builds a larger circuit (``learn_xpc``) hangs it under its own nodes."""
        from deeprob.spn.learning.learnspn import new_node
        weights = {self.scope[i]: np.exp(self.params[i]) for i in range(len(self.tree))}
        sums = ([], [])                 # per parent value l: the sums of the nodes visited and not yet consumed
        for node in _post_order(build_tree_structure(self.tree, scope=self.scope)):
            v, n_kids = node.get_id(), len(node.get_children())
            branches = [new_node('Bernoulli', [v], params={'p': float(k)}) for k in (0, 1)]
            if n_kids:
                for k in (0, 1):
                    kids = [branches[k]] + sums[k][-n_kids:]
                    del sums[k][-n_kids:]
                    branches[k] = dict(new_node('Product', [s for c in kids for s in c['scope']]), children=kids)
            for l in (0, 1):
                sums[l].append(dict(new_node('Sum', branches[0]['scope'], weights=weights[v][l]), children=list(branches)))
        return sums[1][0]

    def get_scopes(self):
        """The scope of every inner node of the tree, as in the circuit of ``to_pc``: each once, children first."""
        scopes, pending = [], []
        for node in _post_order(build_tree_structure(self.tree, scope=self.scope)):
            n_kids = len(node.get_children())
            if n_kids == 0:
                pending.append([node.get_id()])
                continue
            merged = [v for s in pending[-n_kids:] for v in s] + [node.get_id()]
            del pending[-n_kids:]
            pending.append(merged)
            scopes.append(merged)
        return scopes
