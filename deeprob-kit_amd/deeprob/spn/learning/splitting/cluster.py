"""Row clustering on the HIP device (reference deeprob/spn/learning/splitting/cluster.py): ``gmm`` and ``kmeans`` with the
reference's signatures, usable on their own and -- the functions themselves, recognised by identity -- as ``split_rows``
of ``learn_spn``.  Both are this project's own definitions (DESIGN.md 14.5 and "LearnSPN on the device"): the same kind of
split as scikit-learn's, not the same labels, because scikit-learn's k-means initialisation cannot be reproduced.  ``gmm``
is scikit-learn's ``GaussianMixture(n, covariance_type='full', tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=3)`` EM,
operation by operation, from three Lloyd initialisations seeded by ``random_state.choice``; ``kmeans`` is the k-means of
``learn_spn`` for one task (5 restarts, the lowest inertia wins).

Accepted: all-discrete columns (``Bernoulli`` / ``Categorical``, domains ``list(range(K))``) or all-``Gaussian`` columns;
mixed columns and ``Uniform`` raise ``NotImplementedError``.  There is no CPU fallback: a CPU tensor raises ``HipError``.

Not built: the reference's ``kmeans_mb``, ``dbscan`` and ``wald``.
"""
from typing import List, Union

import numpy as np


def _setup(data, distributions, domains, random_state, n, who):
    """The argument checks (before any device work), then ``(kind, device data, row index, RandomState)``."""
    import torch
    from deeprob.hip import learn as L
    from deeprob.spn.learning import learnspn as LS
    from deeprob.spn.learning.splitting import rdc as R
    if len(data.shape) != 2:
        raise ValueError("The data must be a matrix of samples by features")
    if len(distributions) != data.shape[1] or len(domains) != data.shape[1]:
        raise ValueError("Each data column should correspond to a random variable having a distribution and a domain")
    if not 1 <= int(n) <= L.DPL_MAX_CLUSTERS:
        raise ValueError("{} on the HIP path takes 1..{} clusters".format(who, L.DPL_MAX_CLUSTERS))
    if R.all_gaussian(distributions):
        from deeprob.spn.learning.learnspn_cont import GaussianColumns
        kind = GaussianColumns(distributions, domains)
    else:
        kind = LS.DiscreteColumns(distributions, domains)
    kind.check_columns(None)
    random_state = LS.check_random_state(random_state)
    if data.shape[0] < int(n):
        raise ValueError("n_samples={} should be >= n_clusters={}".format(data.shape[0], int(n)))
    dev = kind.upload(data)
    return kind, dev, torch.arange(dev.n_rows, dtype=torch.int32, device=dev.device), random_state


def _task(dev, random_state, n, draws):
    task = LearnTask(0, dev.n_rows, list(range(dev.n_cols)))
    task.draw = np.stack([random_state.choice(dev.n_rows, int(n), replace=False) for _ in range(draws)])
    return task


class LearnTask:
    """What the column kinds' batch builders read of a ``learn_spn`` task."""

    def __init__(self, row_off, n, scope):
        self.row_off, self.n, self.scope, self.draw = row_off, n, scope, None


def gmm(
    data,
    distributions: list,
    domains: List[Union[list, tuple]],
    random_state: np.random.RandomState,
    n: int = 2
) -> np.ndarray:
    """
    Execute GMM clustering on some data, on the HIP device (the definition: DESIGN.md 14.5).

    :param data: The data: a numpy array or a tensor on a HIP device.
    :param distributions: The data distributions.
    :param domains: The data domains.
    :param random_state: The random state: ``choice`` is called three times, once per initialisation.
    :param n: The number of clusters, 1..8.
    :return: An ``np.int64`` array where each element is the cluster where the corresponding data belong.
    """
    from deeprob.hip import learn as L
    kind, dev, row_index, random_state = _setup(data, distributions, domains, random_state, n, 'gmm')
    batch = kind.gmm_batch(row_index, [_task(dev, random_state, n, L.GMM_N_INIT)], int(n))
    best = batch.run()[0]
    return batch.host_labels[int(best[0])].astype(np.int64)


def kmeans(
    data,
    distributions: list,
    domains: List[Union[list, tuple]],
    random_state: np.random.RandomState,
    n: int = 2
) -> np.ndarray:
    """
    Execute K-Means clustering on some data, on the HIP device: the k-means of ``learn_spn`` for one task (DESIGN.md,
    "LearnSPN on the device").

    :param data: The data: a numpy array or a tensor on a HIP device.
    :param distributions: The data distributions.
    :param domains: The data domains.
    :param random_state: The random state: ``choice`` is called five times, once per restart.
    :param n: The number of clusters, 1..8.
    :return: An ``np.int64`` array where each element is the cluster where the corresponding data belong.
    """
    from deeprob.hip import learn as L
    from deeprob.spn.learning.learnspn import KMEANS_RESTARTS
    kind, dev, row_index, random_state = _setup(data, distributions, domains, random_state, n, 'kmeans')
    batch = kind.kmeans_batch(row_index, [_task(dev, random_state, n, KMEANS_RESTARTS)], int(n))
    inertia, _, labels, _ = batch.run()
    return L.read(labels[int(np.argmin(inertia[0]))]).astype(np.int64)
