"""The G-test column splits of the reference (deeprob/spn/learning/splitting/gvs.py) on the HIP device: ``gvs_cols``,
``rgvs_cols`` and ``gtest``.  Discrete columns: the joint counts over the two domains (``dpl_pair_g``); this is the path
of ``learn_spn``'s names 'gvs' / 'rgvs', with the same draws and the same result.  ``Gaussian`` columns: each column is
binned with ``np.histogram_bin_edges(col, 'fd')`` (the bins of splitting/hist.py), coded on the device
(``dpl_hist_codes``), and the G statistic of the joint table of two coded columns comes from ``dpl_pair_g_codes``;
``dof = (bins_i - 1) * (bins_j - 1)`` and the columns count as independent when ``g < 2 * dof * p`` -- with an
interquartile range of zero a column has one bin and ``dof`` is 0, as in the reference.  The statistic is float64 here and
float32 in the reference: a decision can differ only within rounding of its threshold.

``wrgvs_cols`` is not built: its ``random_state.choice`` draws depend on the G-tests of the same task (gvs.py:133-139),
and ``learn_spn`` here makes a generation's draws from sizes alone, before any statistic.
"""
from typing import List, Union

import numpy as np

from deeprob.spn.learning.splitting import hist as H


def gvs_cols(
    data,
    distributions: list,
    domains: List[Union[list, tuple]],
    random_state,
    p: float = 5.0
) -> np.ndarray:
    """
    Greedy Variable Splitting (GVS) independence test (reference gvs.py:11-50).

    :param data: The data: a numpy array or a tensor on a HIP device, complete.
    :param distributions: The distributions (all ``Bernoulli`` / ``Categorical``, or all ``Gaussian``).
    :param domains: The domains.
    :param random_state: The random state (``randint`` picks the first feature).
    :param p: The threshold for the G-Test.
    :return: A partitioning of features: int64, 1 for the features dependent on the first one.
    """
    return H.split_alone('gvs', data, distributions, domains, random_state, {'p': p})


def rgvs_cols(
    data,
    distributions: list,
    domains: List[Union[list, tuple]],
    random_state,
    p: float = 5.0
) -> np.ndarray:
    """
    Random Greedy Variable Splitting (RGVS) independence test (reference gvs.py:53-97): GVS on a random subset of
    ``max(sqrt(features), 2)`` features, the others all in cluster 0 or all in cluster 1 by a coin.
    """
    return H.split_alone('rgvs', data, distributions, domains, random_state, {'p': p})


def gtest(
    data,
    i: int,
    j: int,
    distributions: list,
    domains: List[Union[list, tuple]],
    p: float = 5.0,
    test: bool = True
) -> Union[bool, float]:
    """
    The G-Test independence test between two features (reference gvs.py:156-208).

    :param test: If the method is called as test (true) or as value of statistics (false), default True.
    :return: False if the features are assumed to be dependent, True otherwise; the statistic with ``test=False``.
    """
    g, dof = H.split_alone('gvs', data, distributions, domains, None, {'p': p}, pair=(i, j))
    return bool(g < 2.0 * dof * p) if test else g
