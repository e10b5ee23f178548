"""``estimate_priors_joints`` and ``compute_mutual_information`` of the reference (deeprob/utils/statistics.py:33-109)
for binary data, with the counting on the HIP device.

The one statistic of the data both need is the co-occurrence matrix ``ones[i, j]`` = rows with ``x_i = x_j = 1``.  The
reference takes it from a float32 ``np.dot(data.T, data)``; here ``dpc_pack_bits`` + ``dpc_pair_counts`` count it in exact
integers.  Everything after the counts is float32 arithmetic on the host in the reference's expressions, so for
``N < 2^24`` rows -- where the reference's float32 products and sums of 0/1 values are exact too -- priors, joints and
mutual information are the reference's, operation for operation.  Beyond that the reference's own counts round and
the claim ends; the counts here stay exact up to ``N < 2^31``.
"""
from typing import Tuple

import numpy as np


def device_binary_rows(data):
    """Binary ``data`` ``[N, D]`` as a float32 tensor on a HIP device: a numpy array is uploaded to the current device, a
    device tensor is taken as it is.  ValueError for NaN or values other than 0 / 1; HipError for a CPU tensor or a
    missing library."""
    import torch
    from deeprob.hip import HipError, clt
    if isinstance(data, torch.Tensor):
        if not data.is_cuda:
            raise HipError("data lives on '{}': the deeprob HIP path only works on tensors on a HIP device (there is no "
                           "CPU fallback); pass a numpy array or a device tensor".format(data.device))
        if data.dim() != 2:
            raise ValueError("The data must be a matrix of samples by features")
        if not bool(((data == 0) | (data == 1)).all()):
            raise ValueError("The data must be binary: every value 0 or 1, no NaN")
        x = data
    else:
        data = np.asarray(data)
        if data.ndim != 2:
            raise ValueError("The data must be a matrix of samples by features")
        if not ((data == 0) | (data == 1)).all():
            raise ValueError("The data must be binary: every value 0 or 1, no NaN")
        clt.load_library()
        if not torch.cuda.is_available():
            raise HipError("counting needs a HIP device (there is no CPU fallback)")
        x = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).to(torch.device('cuda', torch.cuda.current_device()))
    if x.shape[0] < 1 or x.shape[0] >= 2 ** 31:
        raise ValueError("expected 1 .. 2^31 - 1 rows, got {}".format(x.shape[0]))
    return x


def device_training_rows(data):
    """The training rows of a cutset-network learner (``BinaryCNet.fit``, ``learn_cnet_bd`` / ``learn_cnet_bic``,
    ``select_cand_cuts``) as a contiguous float32 device tensor: :func:`device_binary_rows` of a matrix of at least one row and
    1 .. ``DPC_MAX_D`` columns.  HipError for a CPU tensor, before anything else; ValueError for the rest."""
    import torch
    from deeprob.hip import HipError
    from deeprob.hip.clt import DPC_MAX_D
    if isinstance(data, torch.Tensor) and not data.is_cuda:
        raise HipError("data lives on '{}': the deeprob HIP path only works on tensors on a HIP device (there is no CPU "
                       "fallback) -- build the libraries with `make -C deeprob-kit_amd/csrc` and pass a numpy array or a "
                       "device tensor".format(data.device))
    if len(data.shape) != 2 or data.shape[0] < 1 or data.shape[1] < 1:
        raise ValueError("The data must be a matrix of samples by features")
    if data.shape[1] > DPC_MAX_D:
        raise ValueError("expected at most {} variables (DPC_MAX_D), got {}".format(DPC_MAX_D, data.shape[1]))
    x = device_binary_rows(data)
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    return x


def pair_counts(data) -> Tuple[np.ndarray, int]:
    """``(ones [D, D] int64, N)`` of binary ``data`` ``[N, D]``: a numpy array (counted on the current HIP device) or a
    device tensor.  ValueError for NaN or values other than 0 / 1; HipError for a CPU tensor or a missing library."""
    from deeprob.hip import clt
    x = device_binary_rows(data)
    ones = clt.pair_counts(clt.pack_bits(x))
    return ones.cpu().numpy().astype(np.int64), int(x.shape[0])


def _cells(ones: np.ndarray, n: int) -> np.ndarray:
    """``[D, D, 2, 2]`` int64: ``cells[i, j, k, l]`` = rows with ``x_i = k`` and ``x_j = l``."""
    d = ones.shape[0]
    col = np.diag(ones)                              # col[i] = rows with x_i = 1
    cells = np.empty((d, d, 2, 2), np.int64)
    cells[:, :, 1, 1] = ones
    cells[:, :, 0, 1] = col[None, :] - ones          # x_i = 0, x_j = 1
    cells[:, :, 1, 0] = col[:, None] - ones
    cells[:, :, 0, 0] = n - col[None, :] - col[:, None] + ones
    return cells


def compute_prior_counts(data) -> np.ndarray:
    """``[D, 2]`` float32, ``[i, k]`` = rows with ``x_i = k`` (the reference's statistics.py:185-201), from the exact
    device counts of :func:`pair_counts`."""
    ones, n = pair_counts(data)
    out = np.empty((ones.shape[0], 2), np.float32)
    out[:, 1] = np.diag(ones)
    out[:, 0] = n - np.diag(ones)
    return out


def compute_joint_counts(data) -> np.ndarray:
    """``[D, D, 2, 2]`` float32, ``[i, j, k, l]`` = rows with ``x_i = k`` and ``x_j = l`` (the reference's
    statistics.py:204-225; the diagonal holds a variable against itself), from :func:`pair_counts`."""
    ones, n = pair_counts(data)
    return _cells(ones, n).astype(np.float32)


def priors_joints_from_counts(ones: np.ndarray, n_samples: int, alpha: float = 0.1) -> Tuple[np.ndarray, np.ndarray]:
    """``(priors [D, 2], joints [D, D, 2, 2])`` float32 from the exact integer counts (statistics.py:83-109):
    ``priors[i, k] = P(X_i = k)``, ``joints[i, j, k, l] = P(X_i = k, X_j = l)``, Laplace smoothing ``alpha``."""
    if alpha < 0.0:
        raise ValueError("The Laplace smoothing factor must be non-negative")
    ones = np.asarray(ones, np.int64)
    d = ones.shape[0]
    col = np.diag(ones)                              # col[i] = rows with x_i = 1
    n = int(n_samples)
    # the four cells of every pair in integers; float32 holds them exactly for n < 2^24, as it holds the reference's
    cells = _cells(ones, n)

    priors = np.empty((d, 2), np.float32)
    priors[:, 1] = (col.astype(np.float32) + 2 * alpha) / (n + 4 * alpha)
    priors[:, 0] = 1.0 - priors[:, 1]
    joints = (cells.astype(np.float32) + alpha) / (n + 4 * alpha)
    # a variable with itself: no smoothing off the diagonal of its own table
    v = np.arange(d)
    joints[v, v, 0, 0] = priors[:, 0]
    joints[v, v, 0, 1] = 0.0
    joints[v, v, 1, 0] = 0.0
    joints[v, v, 1, 1] = priors[:, 1]
    return priors, joints


def estimate_priors_joints(data, alpha: float = 0.1) -> Tuple[np.ndarray, np.ndarray]:
    """
    Estimate both priors and joints probability distributions from binary data; the counts come from the HIP device.

    :param data: The binary data matrix: a numpy array or a device tensor.
    :param alpha: The Laplace smoothing factor.
    :return: ``(priors, joints)`` float32, ``priors[i, k] = P(X_i=k)`` and ``joints[i, j, k, l] = P(X_i=k, X_j=l)``.
    :raises ValueError: If the Laplace smoothing factor is out of domain, or the data are not binary.
    """
    if alpha < 0.0:
        raise ValueError("The Laplace smoothing factor must be non-negative")
    ones, n = pair_counts(data)
    return priors_joints_from_counts(ones, n, alpha)


def compute_mutual_information(priors: np.ndarray, joints: np.ndarray) -> np.ndarray:
    """
    The mutual information between every pair of variables (statistics.py:33-61), a symmetric ``[D, D]`` matrix with
    a zero diagonal.

    :raises ValueError: If the shapes disagree, the joints are not symmetric, or either is not a distribution.
    """
    d, k = priors.shape
    if joints.shape != (d, d, k, k):
        raise ValueError("There are inconsistencies between priors and joints distributions")
    if not np.array_equal(joints, joints.transpose(1, 0, 3, 2)):
        raise ValueError("The joints probability distributions are expected to be symmetric")
    if not np.allclose(priors.sum(axis=1), 1.0):
        raise ValueError("The priors probability distributions are not valid")
    if not np.allclose(joints.sum(axis=(2, 3)), 1.0):
        raise ValueError("The joints probability distributions are not valid ")
    # [i, j, k, l] = P(X_i=k) P(X_j=l), as a transposed view of the outer product: numpy orders the four-term sum below by
    # the memory layout of its operand, and the layout is kept the reference's so that the sum is too
    independent = np.multiply.outer(priors, priors).transpose(0, 2, 1, 3)
    with np.errstate(divide='ignore', invalid='ignore'):   # (log 0 on the diagonal, zeroed below)
        mi = np.sum(joints * (np.log(joints) - np.log(independent)), axis=(2, 3))
    np.fill_diagonal(mi, 0.0)
    return mi
