"""Row splits from given clusters (reference deeprob/spn/learning/splitting/rows.py:23-43), on the host."""
from typing import List, Tuple

import numpy as np


def split_rows_clusters(
    data: np.ndarray,
    clusters: np.ndarray
) -> Tuple[List[np.ndarray], List[float]]:
    """
    Split the data horizontally given the clusters.

    :param data: The data.
    :param clusters: The clusters.
    :return: (slices, weights) where slices is a list of partial data and
             weights is a list of proportions of the local data in respect to the original data.
    """
    slices, weights = [], []
    n_samples = len(data)
    for c in np.unique(clusters):
        local_data = data[clusters == c, :]
        slices.append(local_data)
        weights.append(len(local_data) / n_samples)
    return slices, weights
