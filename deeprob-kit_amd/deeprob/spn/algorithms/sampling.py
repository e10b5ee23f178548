"""``sample`` of a vanilla SPN (reference: deeprob/spn/algorithms/sampling.py:13-58) on the HIP evaluator."""
from typing import Optional, Union

import numpy as np
import torch

from deeprob.spn.structure.io import FlatSpn
from deeprob.spn.algorithms.inference import top_down


def sample(root: FlatSpn, x: Union[np.ndarray, torch.Tensor], inplace: bool = False, n_jobs: int = 0,
           seed: Optional[int] = None) -> Union[np.ndarray, torch.Tensor]:
    """
    Sample some features from the distribution represented by the SPN, given the others.

    Unlike the reference, a sum node's branch is drawn from the exact posterior
    ``w_k exp(ll_k) / sum_j w_j exp(ll_j)``: sampling.py:56 adds left-skewed Gumbel noise (``gumbel_l``) before its
    argmax, which gives wrong branch frequencies for three or more children.

    :param root: The SPN (as loaded by ``deeprob.spn.structure.io.load_spn_json``).
    :param x: The inputs ``[B, >= n_features]`` with NaN entries to fill with sampled values; the other entries are
              evidence and come back bit for bit.  numpy in gives numpy out, a device tensor stays on its device.
    :param inplace: Whether to write into ``x`` itself (float32).
    :param n_jobs: Accepted for compatibility (the reference's joblib thread count).
    :param seed: Seed of the counter-based draws; None takes one from torch's generator.  The same seed, circuit
                 and inputs give the same output.
    :return: The inputs that are NaN-filled with samples from appropriate distributions.
    :raises ValueError: If the SPN is not smooth / decomposable, or the inputs do not cover its scope.
    """
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    return top_down(root, x, inplace, 1, int(seed) & (2 ** 64 - 1), 'sample')
