"""The RDC column split of the reference (deeprob/spn/learning/splitting/rdc.py) for discrete data, on the HIP device.

The reference one-hot encodes a column, takes the ECDF of each indicator, projects with random Gaussian weights, applies
``sin`` and reports the largest canonical correlation of two such feature blocks (rdc.py:85-177).  For a discrete column
every feature is a function of the row's value alone, so a block spans (at most) the indicator space of its column, and
for ``k >= K - 1`` it spans all of it: the largest canonical correlation is then the MAXIMAL (Hirschfeld-Gebelein-Renyi)
correlation of the two columns, the largest singular value of their normalised, centred contingency table.  The random
weights cancel out.  ``dpl_pair_maxcorr`` (include/deeprob_learn.h) computes that value exactly and deterministically
from the joint counts; see DESIGN.md, "rdc column splits".

Built: ``rdc_scores`` and ``rdc_cols``, with the reference's signatures.  Both consume the ``RandomState`` exactly as
the reference does -- for every column in order ``randn(K_i, k)`` then ``randn(k)`` -- and discard the numbers, so later
draws stay in step with the reference.  ``nl`` is not taken (the value does not depend on it).

Not built: ``rdc_rows``, ``rdc_transform`` and ``rdc_cca``.  ``rdc_rows`` clusters the random features themselves and so
does depend on the draws; continuous distributions have no finite table.

``learn_spn(..., split_cols=rdc_cols)`` takes this module's function, recognised by identity.  The STRING 'rdc' (the
reference's default) still raises ``NotImplementedError`` in ``learn_spn``.
"""
from collections import deque
from typing import List, Union

import numpy as np

D_DEFAULT, K_DEFAULT, S_DEFAULT = 0.3, 20, 1.0 / 6.0


def check_parameters(ks, d=D_DEFAULT, k=K_DEFAULT, s=S_DEFAULT):
    """The checks of ``d``, ``k`` and ``s`` against the domain sizes ``ks``; touches no device."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError("The size of the latent space k must be a positive integer, got {}".format(k))
    if isinstance(s, bool) or not isinstance(s, (int, float, np.integer, np.floating)) or not s > 0 or not np.isfinite(s):
        raise ValueError("The variance s of the gaussian distribution must be positive, got {}".format(s))
    if isinstance(d, bool) or not isinstance(d, (int, float, np.integer, np.floating)) or not np.isfinite(d):
        raise ValueError("The threshold d must be a finite number, got {}".format(d))
    if k < max(ks) - 1:
        raise NotImplementedError(
            "k = {} random features cannot span the {} indicators of the largest domain: the reference's score is then "
            "rank limited and depends on the random draws, which is not built on the HIP path (use k >= {})"
            .format(k, max(ks), max(ks) - 1))


def consume_draws(random_state: np.random.RandomState, ks, k: int):
    """The draws of rdc.py:170-176 for columns of domain sizes ``ks``, discarded."""
    for K in ks:
        random_state.randn(K, k)
        random_state.randn(k)


def components(adjacent: np.ndarray) -> np.ndarray:
    """Labels of the connected components of a symmetric adjacency matrix, numbered by each component's smallest member
    (what ``scipy.sparse.csgraph.connected_components`` returns, rdc.py:47)."""
    nf = len(adjacent)
    labels, nxt = np.full(nf, -1, np.int32), 0
    for start in range(nf):
        if labels[start] >= 0:
            continue
        labels[start] = nxt
        queue = deque([start])
        while queue:
            f = queue.popleft()
            for o in np.flatnonzero(adjacent[f]):
                if labels[o] < 0:
                    labels[o] = nxt
                    queue.append(int(o))
        nxt += 1
    return labels


def _check_data(data, distributions, domains):
    from deeprob.spn.learning.learnspn import check_discrete
    if len(distributions) == 0:
        raise ValueError("The list of distribution classes must be non-empty")
    if len(domains) == 0:
        raise ValueError("The list of domains must be non-empty")
    if len(data.shape) != 2:
        raise ValueError("The data must be a matrix of samples by features")
    if len(distributions) != data.shape[1] or len(domains) != data.shape[1]:
        raise ValueError("Each data column should correspond to a random variable having a distribution and a domain")
    check_discrete(distributions, domains, 'rdc_scores')
    return [len(dom) for dom in domains]


def rdc_scores(
    data,
    distributions: list,
    domains: List[Union[list, tuple]],
    random_state,
    k: int = K_DEFAULT,
    s: float = S_DEFAULT
) -> np.ndarray:
    """
    Compute the RDC score for each pair of features (reference rdc.py:85-119) as the exact maximal correlation.

    :param data: The data: a numpy array or a tensor on a HIP device, discrete and complete.
    :param distributions: The data distributions (``Bernoulli`` / ``Categorical``).
    :param domains: The data domains, each ``list(range(K))`` with ``K <= 16``.
    :param random_state: The random state (consumed as the reference consumes it).
    :param k: The size of the latent space; must be at least ``max(K) - 1``.
    :param s: The variance of the gaussian distribution (checked; the value does not depend on it).
    :return: The ``[D, D]`` float64 score matrix, with a unit diagonal.
    :raises ValueError: For bad shapes, domains, data, ``k < 1`` or ``s <= 0``.
    :raises NotImplementedError: For continuous distributions and for ``k < max(K) - 1``.
    :raises HipError: If the data is a CPU tensor or there is no device.
    """
    from deeprob.spn.learning.learnspn import check_random_state, _to_device
    from deeprob.hip import learn as L
    ks = _check_data(data, distributions, domains)
    check_parameters(ks, k=k, s=s)
    random_state = check_random_state(random_state)
    L.load_library()
    dev = _to_device(data, ks)
    consume_draws(random_state, ks, int(k))
    nf = dev.n_cols
    scores = np.ones((nf, nf), np.float64)
    if nf < 2:
        return scores
    import torch
    ia, ib = np.triu_indices(nf, 1)
    row_index = torch.arange(dev.n_rows, dtype=torch.int32, device=dev.device)
    got = L.read(L.pair_maxcorr(dev, row_index, ia, ib, np.zeros(len(ia), np.int64), np.full(len(ia), dev.n_rows),
                                np.asarray(ks)[ia], np.asarray(ks)[ib]))
    scores[ia, ib] = got
    scores[ib, ia] = got
    return scores


def rdc_cols(
    data,
    distributions: list,
    domains: List[Union[list, tuple]],
    random_state,
    d: float = D_DEFAULT,
    k: int = K_DEFAULT,
    s: float = S_DEFAULT
) -> np.ndarray:
    """
    Split the features using the RDC method (reference rdc.py:16-48): the connected components of ``scores > d``.

    :param d: The threshold value that regulates the independence tests among the features.
    :return: A features partitioning: int32 labels, numbered by each component's smallest column.
    """
    check_parameters(_check_data(data, distributions, domains), d=d, k=k, s=s)
    return components(rdc_scores(data, distributions, domains, random_state, k=k, s=s) > d)
