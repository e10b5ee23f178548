"""The entropy column splits of the reference (deeprob/spn/learning/splitting/entropy.py) on the HIP device: a column goes
to cluster 1 when the entropy of its smoothed histogram is below ``e``.  Discrete columns: the histogram is the counts
over the domain, the entropy ``-sum p log2 p``.  ``Gaussian`` columns: ``np.histogram(col, bins='scott')`` -- the bins of
splitting/hist.py, coded and counted on the device (``dpl_hist_codes``, ``dpl_code_counts``) -- and the entropy divided
by ``log2(bins)`` (nan, hence cluster 0, for one bin).  ``learn_spn(..., split_cols=entropy_cols)`` takes these
functions, recognised by identity; the strings 'ebvs' and 'ebvs_ae' stay unbuilt names.
"""
from typing import List, Union

import numpy as np

from deeprob.spn.learning.splitting import hist as H


def entropy_cols(
    data,
    distributions: list,
    domains: List[Union[list, tuple]],
    random_state,
    e: float = 0.3,
    alpha: float = 0.1
) -> np.ndarray:
    """
    Entropy based column splitting method (reference entropy.py:10-49).

    :param data: The data: a numpy array or a tensor on a HIP device, complete.
    :param distributions: Distributions of the features (all ``Bernoulli`` / ``Categorical``, or all ``Gaussian``).
    :param domains: Range of values of the features.
    :param random_state: The random state (no draw is made).
    :param e: Threshold of the considered entropy to be signficant.
    :param alpha: laplacian alpha to apply at frequence.
    :return: A partitioning of features: int64, 1 where the entropy is below ``e``.
    """
    return H.split_alone(H.ENTROPY, data, distributions, domains, random_state, {'e': e, 'alpha': alpha})


def entropy_adaptive_cols(
    data,
    distributions: list,
    domains: List[Union[list, tuple]],
    random_state,
    e: float = 0.3,
    alpha: float = 0.1,
    size: int = None
) -> np.ndarray:
    """
    Adaptive Entropy based column splitting method (reference entropy.py:52-80): ``entropy_cols`` with the threshold
    ``max(e * len(data) / size, float32 eps)``.

    :param size: Size of whole dataset.
    :raises ValueError: If the size of the data is missing.
    """
    return H.split_alone(H.ENTROPY_ADAPTIVE, data, distributions, domains, random_state, {'e': e, 'alpha': alpha, 'size': size})
