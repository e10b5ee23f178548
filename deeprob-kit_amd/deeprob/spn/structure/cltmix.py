"""``BinaryCLTMixture``: a mixture of binary Chow-Liu trees over one scope -- the ``Sum`` over ``BinaryCLT`` leaves of the
reference's examples/spn_clt_em.py -- as one object, evaluated and trained on the HIP device through the ``dpc_mix_*`` entry
points of ``libdeeprob_clt.so`` (include/deeprob_clt.h, last section).  ``FlatSpn`` has no multivariate leaf, so the model
cannot be a node graph here; ``to_pc()`` gives the equivalent ``FlatSpn`` (a Sum over the trees' circuits), through which
the node-graph algorithms of ``deeprob.spn.algorithms`` (the moments, for one) are reached.

The posterior queries are the model's own: ``marginals``, ``sample`` and ``mpe`` are one launch each (``dpc_mixq_*``,
DESIGN.md 15.2) that visits the trees one at a time -- ``2 D`` floats and ``D + K`` doubles of scratch per row, where the
circuit of ``to_pc()`` keeps a value per node and row.  ``mpe`` maximises ``w_k p_k(x)`` over the completions AND the
components (the max-product MPE of the circuit); it is not the MAP of the mixture density ``sum_k w_k p_k(x)``, which is
NP-hard, and ``algorithms.mpe(mix.to_pc(), x)`` follows the reference's rule (the values of the sum pass choose the branch)
and need not agree with it.

``em`` is the reference's batch EM (learning/em.py:18-113) for this shape, with the CPTs of every tree TIED as
``BinaryCLT.em_step`` ties them (cltree.py:127-155) and the mixture weights updated as ``Sum.em_step`` does
(node.py:100-111).  An iteration is two launches over the batch index (``dpc_mix_log_likelihood``: likelihoods and
responsibilities of all components; ``dpc_mix_em_stats``: their weighted counts in a fixed order of float64 additions),
one read of ``K (1 + 2 D)`` doubles, the reference's float32 updates on the host (``cltree.em_update``) and one upload of
the new tables.  Two calls with the same arguments give bitwise identical parameters.  Inputs follow ``BinaryCLT``: numpy in,
numpy out through the current HIP device; a device tensor stays on its device; a CPU tensor or a missing library raises
``HipError``.
"""
from typing import List, Optional

import numpy as np

from deeprob.spn.structure.cltree import BinaryCLT, em_update
from deeprob.utils.random import RandomState, check_random_state

#: restarts of the k-means that splits the rows in ``fit``: those of ``learn_spn``
KMEANS_RESTARTS = 5


class BinaryCLTMixture:
    def __init__(self, scope: List[int], components: Optional[List[BinaryCLT]] = None, weights=None):
        """
        Initialize a mixture of Binary Chow-Liu Trees.

        :param scope: The scope: the ids of the variables.
        :param components: The trees. If None, ``fit`` learns them.
        :param weights: The mixture weights, one per tree. They are kept as float32.
        :raises ValueError: If a component has another scope.
        :raises ValueError: If the length of weights and components are different.
        :raises ValueError: If weights don't sum up to 1.
        """
        scope = [scope] if isinstance(scope, int) else list(scope)
        if len(scope) == 0:
            raise ValueError("The scope must not be empty")
        if len(set(scope)) != len(scope):
            raise ValueError("The scope must not contain duplicates")
        self.scope = scope
        if components is not None:
            components = list(components)
            if len(components) == 0:
                raise ValueError("A mixture needs at least one component")
            if any(not isinstance(c, BinaryCLT) for c in components):
                raise ValueError("The components of a BinaryCLTMixture must be BinaryCLTs")
            if any(list(c.scope) != scope for c in components):
                raise ValueError("Components of the mixture have different scopes")
        if weights is not None:
            weights = np.array(weights, dtype=np.float32)
            if components is None or weights.shape != (len(components),):
                raise ValueError("Weights and components length mismatch")
            if not np.isclose(np.sum(weights), 1.0):
                raise ValueError("Weights don't sum up to 1")
        self.components, self.weights = components, weights
        #: batch mean log-likelihood of every iteration of the last ``em`` (before its update), kept on the device
        self.em_mean_ll = None
        #: the cluster of every training row of the last ``fit`` (component j was fitted to the j-th present label)
        self.labels = None

    # ---- learning ----------------------------------------------------------------------------------------------------
    def fit(self, data, domain: List[list], n_components: int = 2, alpha: float = 0.1,
            random_state: Optional[RandomState] = None, clusters=None):
        """
        Split the rows into clusters and fit one tree per present cluster; the weights are the clusters' shares.

        :param data: The training data ``[N, len(scope)]``, every value 0 or 1: a numpy array or a device tensor.
        :param domain: The domains of the variables, ``[0, 1]`` each.
        :param n_components: The number of clusters of the k-means (without ``clusters``).
        :param alpha: The Laplace smoothing factor of the trees.
        :param random_state: None, a seed or a Numpy RandomState: seeds the k-means, then draws every tree's root.
        :param clusters: Optional int labels ``[N]``: the clusters, instead of the k-means.  The seeding of the reference's
                         ``examples/spn_clt_em.py`` is ``clusters=deeprob.spn.learning.splitting.gmm(data, [Bernoulli] * D,
                         domain, random_state, n=n_components)``: the Gaussian-mixture row split on the device.
        :return: Itself.
        :raises ValueError: If a parameter is out of domain.
        """
        import torch
        from deeprob.hip import clt, cnet, learn
        if len(data.shape) != 2 or len(domain) != data.shape[1]:
            raise ValueError("Each data column should correspond to a random variable having a domain")
        if not all(d == [0, 1] for d in domain):
            raise ValueError("The domains must be binary for a Binary CLT distribution")
        if alpha < 0.0:
            raise ValueError("The Laplace smoothing factor must be non-negative")
        if data.shape[1] != len(self.scope):
            raise ValueError("expected data [N, {}], got {}".format(len(self.scope), tuple(data.shape)))
        if n_components < 1:
            raise ValueError("The number of components must be positive")
        n, d = int(data.shape[0]), len(self.scope)
        if clusters is not None:
            clusters = np.asarray(clusters)
            if clusters.shape != (n,) or not np.issubdtype(clusters.dtype, np.integer):
                raise ValueError("expected clusters as {} int labels".format(n))
        elif n < n_components:
            raise ValueError("n_samples={} should be >= n_clusters={}".format(n, n_components))
        random_state = check_random_state(random_state)
        xd = self._device_rows(data)
        if clusters is None:
            # one k-means task over all rows and columns, seeded as learn_spn seeds its row splits
            seeds = np.stack([random_state.choice(n, n_components, replace=False) for _ in range(KMEANS_RESTARTS)])
            x_cm = xd.t().contiguous().to(torch.uint8)
            everything = torch.arange(n, dtype=torch.int32, device=xd.device)
            batch = learn.KMeansBatch(learn.DeviceData(x_cm, n, d), everything, [(0, n, list(range(d)), [2] * d, seeds)],
                                      KMEANS_RESTARTS, n_components, 2)
            inertia, _, labels, _ = batch.run()
            clusters = labels[int(np.argmin(inertia[0])), :n].cpu().numpy().astype(np.int64)
        present = np.unique(clusters)                       # (only the present clusters, as split_rows_clusters keeps them)
        if len(present) > clt.DPC_MIX_MAX_K:
            raise ValueError("{} clusters are more than the {} components of a mixture".format(len(present), clt.DPC_MIX_MAX_K))
        rows = [np.flatnonzero(clusters == c) for c in present]
        # the co-occurrence counts of every cluster's rows: the tasks of one generation, as learn_xpc counts its leaves
        gen = cnet.Generation(xd, torch.from_numpy(np.concatenate(rows).astype(np.int32)).to(xd.device), [len(r) for r in rows])
        gen.pack()
        step = cnet.chunk_tasks(d)
        ones = np.concatenate([gen.counts(t0, min(step, len(rows) - t0)).cpu().numpy() for t0 in range(0, len(rows), step)])
        components = []
        for t, r in enumerate(rows):
            tree = BinaryCLT(self.scope, root=self.scope[int(random_state.choice(d))])
            tree.fit_counts(ones[t].astype(np.int64), len(r), alpha=alpha)
            components.append(tree)
        self.components = components
        self.weights = (np.asarray([len(r) for r in rows], np.float64) / n).astype(np.float32)
        self.labels = clusters
        return self

    def em(self, data, num_iter: int = 100, batch_perc: float = 0.1, step_size: float = 0.5, random_init: bool = True,
           random_state: Optional[RandomState] = None, verbose: bool = True):
        """
        Learn the weights and the (tied) CPTs of the trees by batch Expectation-Maximization; see the module docstring.

        :param data: The data ``[n_samples, len(scope)]``, complete 0 / 1 rows: numpy or a tensor on a HIP device.
        :param num_iter: The number of iterations.
        :param batch_perc: The percentage of data to use for each step.
        :param step_size: The step size for batch EM.
        :param random_init: Whether to random initialize the weights and the CPTs.
        :param random_state: The random state. It can be either None, a seed integer or a Numpy RandomState.
        :param verbose: Whether to show the batch mean log-likelihood of every iteration.
        :return: Itself.
        :raises ValueError: If a parameter is out of domain, or the data contains NaN.
        """
        if num_iter <= 0:
            raise ValueError("The number of iterations must be positive")
        if batch_perc <= 0.0 or batch_perc >= 1.0:
            raise ValueError("The batch percentage must be in (0, 1)")
        if step_size <= 0.0 or step_size >= 1.0:
            raise ValueError("The step size must be in (0, 1)")
        self._check()
        if len(data.shape) != 2 or data.shape[1] != len(self.scope):
            raise ValueError("expected data [n_samples, {}], got {}".format(len(self.scope), tuple(data.shape)))
        import torch
        from deeprob.hip import clt
        from deeprob.spn.learning.em import draw_batches
        xd = self._device_rows(data)
        if bool(torch.isnan(xd).any()):
            raise ValueError("The data contains NaN: EM needs complete rows")
        n_samples, d = xd.shape
        k = len(self.components)
        batch_size = int(batch_perc * n_samples)
        random_state = check_random_state(random_state)
        self.weights = np.asarray(self.weights, np.float32)
        if random_init:
            self.weights = random_state.dirichlet(np.ones(k)).astype(np.float32)
            for c in self.components:
                c.em_init(random_state)
        dev = xd.device
        index = torch.from_numpy(draw_batches(random_state, n_samples, batch_size, num_iter)).to(dev)
        codes = clt.pack_query(xd)
        mix = self._on_device(dev)
        mean_ll = torch.zeros(num_iter, dtype=torch.float64, device=dev)
        bar = None
        if verbose:
            try:
                from tqdm import tqdm
                bar = tqdm(total=num_iter, leave=None, unit='batch',
                           bar_format='{desc}| {n_fmt}/{total_fmt} [{elapsed}<{remaining}, {rate_fmt}]')
            except ImportError:
                bar = None
        for it in range(num_iter):
            # (the rows are complete: no scratch for the upward pass, which would be K 2 D floats per row)
            ll, _, resp = clt.mixture_codes_log_likelihood(mix, codes, index[it], complete=True)
            stats = clt.mixture_em_stats(mix, codes, index[it], resp)
            mean_ll[it] = ll.double().mean()
            stats = stats.cpu().numpy()                                 # the one read of the iteration
            # the weights: a component's share of the batch's responsibility, stats[k][0] (the reference's w_k * sum_i
            # exp(ll_ik - ll_i), node.py:107), lifted by float32 eps, then a step of step_size towards the shares
            share = stats[:, 0].astype(np.float32) + np.finfo(np.float32).eps
            share /= share.sum()
            self.weights = (np.float32(1.0 - step_size) * self.weights + np.float32(step_size) * share).astype(np.float32)
            for c, row in zip(self.components, stats):
                c.params = em_update(c.params, c.tree, c.root, row, step_size)
            with np.errstate(divide='ignore'):
                mix.update(np.stack([c.params for c in self.components]), np.log(self.weights))
            if verbose:
                text = 'Batch Avg. LL: {:.4f}'.format(float(mean_ll[it]))
                if bar is not None:
                    bar.set_description(text)
                    bar.update(1)
                else:
                    print('[{}/{}] {}'.format(it + 1, num_iter, text))
        if bar is not None:
            bar.close()
        self.em_mean_ll = mean_ll
        return self

    # ---- queries -----------------------------------------------------------------------------------------------------
    def _check(self):
        if not self.components or self.weights is None:
            raise ValueError("The mixture's components and weights must be already initialized")
        if any(c.tree is None or c.params is None for c in self.components):
            raise ValueError("The CLT's structure and parameters must be already initialized")

    @staticmethod
    def _device_rows(data):
        """``data`` as float32 rows on a HIP device, under the input rules of the module docstring."""
        from deeprob.hip import clt
        return clt.rows_on_device(data, 'BinaryCLTMixture')

    def _on_device(self, device):
        from deeprob.hip import clt
        self._check()
        with np.errstate(divide='ignore'):      # (a weight of zero is a component that takes no part)
            logw = np.log(np.asarray(self.weights, np.float32))
        # (uploaded per call, one small copy: the parameters are public arrays a caller may write into)
        return clt.DeviceMixture([(c.bfs, c.tree, c.params) for c in self.components], logw, device)

    def _run(self, op, x, *args):
        from deeprob.hip import clt
        self._check()
        return clt.run_on_device(self, 'BinaryCLTMixture', op, x, *args)

    def log_likelihood(self, x):
        """``[B, 1]`` float32 log likelihoods; NaN entries are marginalised."""
        from deeprob.hip import clt
        return self._run(clt.mixture_log_likelihood, x).reshape(-1, 1)

    def likelihood(self, x):
        ll = self.log_likelihood(x)
        return np.exp(ll) if isinstance(ll, np.ndarray) else ll.exp()

    def responsibilities(self, x):
        """``[B, K]`` float32: the posterior probability of every component given the observed entries of the row (all
        zero for a row that is impossible under every component)."""
        from deeprob.hip import clt
        return self._run(lambda mix, xd: clt.mixture_log_likelihood(mix, xd, want_resp=True)[2], x)

    def marginals(self, x):
        """A copy of ``x`` ``[B, D]`` with every NaN entry replaced by ``p(x_j = 1 | the row's observed entries)`` under the
        mixture, exact: the trees' posterior marginals weighted by the posterior of the components.  Observed entries come
        back bit for bit; an all-NaN row gives the prior marginals; a row whose evidence is impossible under every component
        gets NaN in its unobserved entries."""
        from deeprob.hip import clt
        return self._run(clt.mixture_marginals, x)

    def sample(self, x, seed: Optional[int] = None, return_component: bool = False):
        """A copy of ``x`` with every NaN entry drawn given the observed entries: the component from its posterior, then the
        entries from that tree.  ``seed``: the seed of the counter-based generator (the same seed gives the same bytes); None
        draws one from numpy's global generator.  With ``return_component`` also ``[B]`` int32, the drawn component -- for a
        complete row a posterior draw of its cluster; -1 (and the row's NaN left in place) where the evidence is impossible
        under every component."""
        from deeprob.hip import clt
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        return self._run(clt.mixture_sample, x, int(seed), 0, bool(return_component))

    def mpe(self, x, return_component: bool = False):
        """A copy of ``x`` with every NaN entry filled by the completion of the pair (component, completion) that maximises
        ``w_k p_k(x)`` given the observed entries: the max-product MPE of the mixture's circuit.  It is NOT the MAP of the
        mixture density ``sum_k w_k p_k(x)`` (NP-hard), and ``algorithms.mpe(self.to_pc(), x)``, which follows the
        reference's rule, need not agree with it.  With ``return_component`` also ``[B]`` int32, the winning component (-1,
        and the row's NaN left in place, where the evidence is impossible under every component)."""
        from deeprob.hip import clt
        return self._run(clt.mixture_mpe, x, bool(return_component))

    # ---- parameters and structure ------------------------------------------------------------------------------------
    def params_count(self) -> int:
        self._check()
        return len(self.weights) + sum(c.params_count() for c in self.components)

    def to_pc(self):
        """The equivalent circuit as a :class:`deeprob.spn.structure.io.FlatSpn`: a Sum with the mixture weights over the
        circuits of the trees (``BinaryCLT.to_pc_nodes``)."""
        from deeprob.spn.learning.learnspn import new_node, to_flat
        self._check()
        root = dict(new_node('Sum', self.scope, weights=np.asarray(self.weights, np.float32)),
                    children=[c.to_pc_nodes() for c in self.components])
        return to_flat(root)
