"""The Gini column splits of the reference (deeprob/spn/learning/splitting/gini.py) on the HIP device: a column goes to
cluster 1 when the Gini index ``1 - sum p^2`` of its smoothed histogram is below ``e``.  The histograms are those of
entropy.py of this package: the counts over the domain for discrete columns, ``np.histogram(col, bins='scott')`` on the
device for ``Gaussian`` ones.  ``learn_spn(..., split_cols=gini_cols)`` takes these functions, recognised by identity; the
strings 'gbvs' and 'gbvs_ag' stay unbuilt names.
"""
from typing import List, Union

import numpy as np

from deeprob.spn.learning.splitting import hist as H


def gini_cols(
    data,
    distributions: list,
    domains: List[Union[list, tuple]],
    random_state,
    e: float = 0.3,
    alpha: float = 0.1
) -> np.ndarray:
    """
    Gini index column splitting method (reference gini.py:11-51).

    :param data: The data: a numpy array or a tensor on a HIP device, complete.
    :param distributions: Distributions of the features (all ``Bernoulli`` / ``Categorical``, or all ``Gaussian``).
    :param domains: Range of values of the features.
    :param random_state: The random state (no draw is made).
    :param e: Threshold of the considered Gini index to be signficant.
    :param alpha: laplacian alpha to apply at frequence.
    :return: A partitioning of features: int64, 1 where the Gini index is below ``e``.
    """
    return H.split_alone(H.GINI, data, distributions, domains, random_state, {'e': e, 'alpha': alpha})


def gini_adaptive_cols(
    data,
    distributions: list,
    domains: List[Union[list, tuple]],
    random_state,
    e: float = 0.3,
    alpha: float = 0.1,
    size: int = None
) -> np.ndarray:
    """
    Adaptive Gini index column splitting method (reference gini.py:54-82): ``gini_cols`` with the threshold
    ``max(e * len(data) / size, float32 eps)``.

    :param size: Size of whole dataset.
    :raises ValueError: If the size of the data is missing.
    """
    return H.split_alone(H.GINI_ADAPTIVE, data, distributions, domains, random_state, {'e': e, 'alpha': alpha, 'size': size})
