"""The RDC column split of the reference (deeprob/spn/learning/splitting/rdc.py) on the HIP device, for all-discrete and
for all-continuous (``Gaussian``) columns.

The reference takes the ECDF of a column (of each indicator of a discrete one), projects with random Gaussian weights,
applies ``sin`` and reports the largest canonical correlation of two such feature blocks (rdc.py:85-177).

DISCRETE columns.  Every feature is a function of the row's value alone, so a block spans (at most) the indicator space
of its column, and for ``k >= K - 1`` it spans all of it: the largest canonical correlation is then the MAXIMAL
(Hirschfeld-Gebelein-Renyi) correlation of the two columns, the largest singular value of their normalised, centred
contingency table.  The random weights cancel out.  ``dpl_pair_maxcorr`` (include/deeprob_learn.h) computes that value
exactly and deterministically from the joint counts; see DESIGN.md, "rdc column splits".  The ``RandomState`` is consumed
exactly as the reference does -- for every column in order ``randn(K_i, k)`` then ``randn(k)`` -- and the numbers are
discarded.

CONTINUOUS columns (every distribution ``Gaussian``, every domain a tuple).  The draws are consumed AND used: per column
in order ``w = (sqrt(s) * randn(1, k)).astype(float32)`` and ``b = (sqrt(s) * randn(k)).astype(float32)``.  The device
gives the "max" ranks of every column (``dpl_ecdf_ranks``) and, in float64, the sums ``S`` and the raw Gram ``G`` of the
features ``sin(rank / n * w + b)`` (``dpl_rdc_gram``).  The score is this project's own, a ridge-regularised closed form
(``scores_from_gram``), because the reference's iterative CCA on 20 numerically rank-5 features is not a well-defined
function of the data; see DESIGN.md, "rdc on continuous columns":

    C = G / n - S S^T / n^2;  per column block p: lam_p = 1e-8 * trace(C_pp) / k,
    W_p = (C_pp + lam_p I)^(-1/2) by eigh with the eigenvalues clamped at 0 before lam_p is added;
    score(p, q) = min(1, largest singular value of W_p C_pq W_q); the diagonal is 1; a block whose trace is 0 (not above
    1e-12 * k, the rounding residue of a constant column's bounded features) scores 0.

Mixed discrete / continuous columns and ``Uniform`` raise ``NotImplementedError``.  ``nl`` is not taken (``sin``).

Not built: ``rdc_rows``, ``rdc_transform`` and ``rdc_cca``.

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


def all_gaussian(distributions) -> bool:
    """Whether this is the all-continuous case the HIP path builds: a non-empty list of ``Gaussian`` only."""
    from deeprob.spn.structure.leaf import Gaussian
    return len(distributions) > 0 and all(d is Gaussian for d in distributions)


def check_continuous(domains):
    """Every domain of an all-Gaussian problem is a tuple ``(lo, hi)`` (reference leaf.py:526-527)."""
    for i, dom in enumerate(domains):
        if not isinstance(dom, tuple) or len(dom) != 2:
            raise ValueError("The domain must be continuous for a Gaussian distribution: variable {} needs a tuple (lo, hi), "
                             "got {}".format(i, dom))


def check_parameters_continuous(d=D_DEFAULT, k=K_DEFAULT, s=S_DEFAULT):
    """The checks of ``d``, ``k`` and ``s`` for continuous columns (no domain size bounds ``k``)."""
    check_parameters([1], d=d, k=k, s=s)


def draw_features(random_state: np.random.RandomState, n_cols: int, k: int, s: float):
    """The draws of rdc.py:170-176 for ``n_cols`` continuous columns (one ECDF feature each): ``(w, b)``, both
    ``[n_cols, k]`` float32."""
    stddev = np.sqrt(s)
    w, b = np.empty((n_cols, k), np.float32), np.empty((n_cols, k), np.float32)
    for p in range(n_cols):
        w[p] = (stddev * random_state.randn(1, k)).astype(np.float32)[0]
        b[p] = (stddev * random_state.randn(k)).astype(np.float32)
    return w, b


RIDGE, ZERO_TRACE = 1e-8, 1e-12


def scores_from_gram(G: np.ndarray, S: np.ndarray, n: int, m: int, k: int) -> np.ndarray:
    """The ``[m, m]`` score matrix of ``m`` continuous columns from the raw Gram ``G`` (``[m k, m k]``) and the sums ``S``
    of their random features over ``n`` rows: the definition in the module docstring, float64, numpy only."""
    G, S = np.asarray(G, np.float64).reshape(m * k, m * k), np.asarray(S, np.float64).reshape(m * k)
    C = G / float(n) - np.outer(S, S) / (float(n) * float(n))
    whiten = []
    for p in range(m):
        Cpp = C[p * k:(p + 1) * k, p * k:(p + 1) * k]
        trace = float(np.trace(Cpp))
        if not trace > ZERO_TRACE * k:
            whiten.append(None)
            continue
        ev, V = np.linalg.eigh(Cpp)
        ev = np.maximum(ev, 0.0) + RIDGE * trace / k
        whiten.append((V / np.sqrt(ev)) @ V.T)
    scores = np.ones((m, m), np.float64)
    for p in range(m):
        for q in range(p + 1, m):
            if whiten[p] is None or whiten[q] is None:
                value = 0.0
            else:
                M = whiten[p] @ C[p * k:(p + 1) * k, q * k:(q + 1) * k] @ whiten[q]
                value = min(1.0, float(np.linalg.svd(M, compute_uv=False)[0]))
            scores[p, q] = scores[q, p] = value
    return scores


def _rdc_scores_continuous(data, domains, random_state, k, s):
    from deeprob.spn.learning.learnspn import check_random_state
    from deeprob.spn.learning.learnspn_cont import to_device_f
    from deeprob.hip import learn as L
    check_continuous(domains)
    check_parameters_continuous(k=k, s=s)
    random_state = check_random_state(random_state)
    dev = to_device_f(data, 'rdc_scores')
    L.load_library()
    nf, n, k = dev.n_cols, dev.n_rows, int(k)
    w, b = draw_features(random_state, nf, k, s)
    if nf < 2:
        return np.ones((nf, nf), np.float64)
    import torch
    row_index = torch.arange(n, dtype=torch.int32, device=dev.device)
    ranks, out_off = L.ecdf_ranks(dev, row_index, np.arange(nf), np.zeros(nf, np.int64), np.full(nf, n))
    gram = L.rdc_gram(ranks, [(n, nf, 0)], k, w, b)
    return scores_from_gram(L.read(gram['G']), L.read(gram['S']), n, nf, k)


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
    if all_gaussian(distributions):
        check_continuous(domains)
        return None
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
    Compute the RDC score for each pair of features (reference rdc.py:85-119): the exact maximal correlation for discrete
    columns, the ridge-regularised closed form of the module docstring for all-``Gaussian`` columns.

    :param data: The data: a numpy array or a tensor on a HIP device, complete.
    :param distributions: The data distributions (all ``Bernoulli`` / ``Categorical``, or all ``Gaussian``).
    :param domains: The data domains, each ``list(range(K))`` with ``K <= 16``, or each a tuple ``(lo, hi)``.
    :param random_state: The random state (consumed as the reference consumes it; used for continuous columns).
    :param k: The size of the latent space; for discrete columns at least ``max(K) - 1``.
    :param s: The variance of the gaussian distribution (for discrete columns the value does not depend on it).
    :return: The ``[D, D]`` float64 score matrix, with a unit diagonal.
    :raises ValueError: For bad shapes, domains, data, ``k < 1`` or ``s <= 0``.
    :raises NotImplementedError: For mixed or ``Uniform`` columns and, on discrete columns, for ``k < max(K) - 1``.
    :raises HipError: If the data is a CPU tensor or there is no device.
    """
    from deeprob.spn.learning.learnspn import check_random_state, _to_device
    from deeprob.hip import learn as L
    ks = _check_data(data, distributions, domains)
    if ks is None:
        return _rdc_scores_continuous(data, domains, random_state, k, s)
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
    ks = _check_data(data, distributions, domains)
    if ks is None:
        check_parameters_continuous(d=d, k=k, s=s)
    else:
        check_parameters(ks, d=d, k=k, s=s)
    return components(rdc_scores(data, distributions, domains, random_state, k=k, s=s) > d)
