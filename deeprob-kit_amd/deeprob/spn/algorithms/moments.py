"""Moments of a vanilla SPN (reference: deeprob/spn/algorithms/moments.py) on the HIP path, unconditional as the
reference computes them and, with ``x``, conditional on the observed entries of every row.

In a smooth and decomposable circuit the root polynomial is linear in the leaves of any one variable ``j``, so with
``r_L`` the posterior flow into leaf ``L`` (``dP_root/dP_L * P_L / P_root``), ``E[x_j^k | e] = sum_L r_L m_k(L)`` over the
leaves over ``j``: one bottom-up and one top-down pass per row, in one launch of ``dpq_flat_spn_posterior``
(include/deeprob_spnq.h states the passes and the order of every sum).  Without ``x`` the same launch runs on one all-NaN
row, so there is one implementation.  There is no CPU path.

Every function keeps the reference's signature and gains ``x=None``:

* without ``x``: ``[n_features]`` float32, as the reference returns;
* with ``x [B, >= n_features]`` (NaN = not observed): an array of the shape of ``x``; numpy in, numpy out (computed on the
  current HIP device), a device tensor stays on its device.  Per entry -- NaN and inside the scope: the conditional
  statistic; observed and inside the scope: that of a point mass (``moment``: ``x^k``, order 1 is ``x`` bit for bit;
  ``variance``: 0; ``skewness`` / ``kurtosis``: NaN, the 0 / 0 their formulas give); outside the scope: as given.  A row
  whose evidence has probability zero is NaN in its in-scope NaN entries.
"""
from typing import Optional, Union

import numpy as np
import torch

from deeprob.spn.structure.io import FlatSpn
from deeprob.spn.algorithms.inference import check_inputs, upload_inputs

MAX_ORDER = 4       # DPQ_MAX_ORDERS: the leaves' closed forms are written out up to the fourth moment


def _planes(root: FlatSpn, x, n_orders: int, what: str):
    """``(m [n_orders, ...] float32 device tensor or None for B = 0, xd, as_numpy, squeeze)``: the non-central moments of
    order 1..n_orders from one launch."""
    from deeprob.hip import spnq
    squeeze = x is None
    if squeeze:
        if not isinstance(root, FlatSpn):
            raise TypeError("{} works on the FlatSpn returned by deeprob.spn.structure.io.load_spn_json".format(what))
        x = np.full((1, root.n_features), np.nan, np.float32)
    x, as_numpy = check_inputs(root, x, what)
    xd = upload_inputs(x, as_numpy)
    if xd is None:      # B = 0
        return None, x, as_numpy, False
    m = spnq.flat_spn_posterior(root, xd, spnq.DPQ_MODE_MOMENTS, n_orders=n_orders)
    return m, xd, as_numpy, squeeze


def _finish(root: FlatSpn, stat, point_mass: float, xd, as_numpy: bool, squeeze: bool):
    """A float64 statistic formed from the moment planes -> float32 result: in-scope observed entries take the point
    mass's value, entries outside the scope come back as given."""
    from deeprob.hip import spnq
    off, _ = spnq.leaf_table(root)
    scope = torch.zeros(xd.shape[1], dtype=torch.bool)
    scope[:root.n_features] = torch.from_numpy(np.diff(off) > 0)
    scope = scope.to(xd.device)
    observed = ~torch.isnan(xd)
    out = stat.float()
    out = torch.where(observed & scope, torch.full_like(out, point_mass), out)
    out = torch.where(~scope, xd, out)
    if squeeze:
        out = out[0]
    return out.cpu().numpy() if as_numpy else out


def _empty(x, as_numpy: bool):
    return np.empty(x.shape, np.float32) if as_numpy else x.new_empty(tuple(x.shape), dtype=torch.float32)


def moment(root: FlatSpn, order: int = 1, x: Optional[Union[np.ndarray, torch.Tensor]] = None
           ) -> Union[np.ndarray, torch.Tensor]:
    """
    Compute non-central moments of a given order of a smooth and decomposable SPN (reference moments.py:11-33), given
    the observed entries of ``x`` when it is passed.

    :param root: The SPN (a FlatSpn).
    :param order: The order of the moment, 0 .. 4.
    :param x: Optional inputs ``[B, >= n_features]``, NaN = not observed (see the module docstring).
    :return: ``E[x_j^order]`` per variable ``[n_features]``, or ``E[x_j^order | evidence]`` per entry of ``x``.
    :raises ValueError: If the order of the moment is negative.
    :raises NotImplementedError: If the order is above 4.
    """
    if order < 0:
        raise ValueError("The order of the moment must be non-negative")
    if order > MAX_ORDER:
        raise NotImplementedError("moments of order above {} are not built (got {})".format(MAX_ORDER, order))
    if order == 0:      # (the reference skips the computation as well)
        if x is None:
            if not isinstance(root, FlatSpn):
                raise TypeError("moment works on the FlatSpn returned by deeprob.spn.structure.io.load_spn_json")
            return np.ones(root.n_features, dtype=np.float32)
        x, as_numpy = check_inputs(root, x, 'moment')
        return np.ones(x.shape, np.float32) if as_numpy else torch.ones_like(x, dtype=torch.float32)
    m, xd, as_numpy, squeeze = _planes(root, x, int(order), 'moment')
    if m is None:
        return _empty(xd, as_numpy)
    # (the kernel has already written x^k and the entries outside the scope: plane order - 1 is the result, bit for bit)
    out = m[order - 1]
    if squeeze:
        out = out[0]
    return out.cpu().numpy() if as_numpy else out


def expectation(root: FlatSpn, x: Optional[Union[np.ndarray, torch.Tensor]] = None) -> Union[np.ndarray, torch.Tensor]:
    """
    Compute the expectation values of a SPN w.r.t. each of the random variables (reference moments.py:50-57), given the
    observed entries of ``x`` when it is passed.  For a Bernoulli variable ``expectation(root, x)[b, j]`` is
    ``p(x_j = 1 | the evidence of row b)``: the counterpart of ``BinaryCLT.marginals``.
    """
    return moment(root, 1, x)


def variance(root: FlatSpn, x: Optional[Union[np.ndarray, torch.Tensor]] = None) -> Union[np.ndarray, torch.Tensor]:
    """
    Compute the variance values of a SPN w.r.t. each of the random variables (reference moments.py:60-69: ``m2 - m1^2``,
    formed here in float64 from one launch with two orders), given the observed entries of ``x`` when it is passed.
    """
    m, xd, as_numpy, squeeze = _planes(root, x, 2, 'variance')
    if m is None:
        return _empty(xd, as_numpy)
    m = m.double()
    return _finish(root, m[1] - m[0] ** 2.0, 0.0, xd, as_numpy, squeeze)


def skewness(root: FlatSpn, x: Optional[Union[np.ndarray, torch.Tensor]] = None) -> Union[np.ndarray, torch.Tensor]:
    """
    Compute the skewness values of a SPN w.r.t. each of the random variables, given the observed entries of ``x`` when
    it is passed: ``(m3 - 3 m1 m2 + 2 m1^3) / var^1.5`` in float64 from one launch with three orders.

    Different from the reference on purpose: its moments.py:86 forms ``g3 = 3 m2 + 2 m1^2`` where the expansion of the
    third central moment has ``3 m2 - 2 m1^2`` (it reports -3.28 for a near-symmetric Bernoulli variable of mean 0.47).
    This function returns the standardised third central moment.
    """
    m, xd, as_numpy, squeeze = _planes(root, x, 3, 'skewness')
    if m is None:
        return _empty(xd, as_numpy)
    m = m.double()
    g1 = m[0] ** 2.0
    g2 = m[1] - g1
    g3 = 3.0 * m[1] - 2.0 * g1
    return _finish(root, (m[2] - m[0] * g3) / (g2 ** 1.5), float('nan'), xd, as_numpy, squeeze)


def kurtosis(root: FlatSpn, x: Optional[Union[np.ndarray, torch.Tensor]] = None) -> Union[np.ndarray, torch.Tensor]:
    """
    Compute the kurtosis values of a SPN w.r.t. each of the random variables (reference moments.py:90-110), given the
    observed entries of ``x`` when it is passed.  Fisher's definition: 3.0 is subtracted to give 0.0 for a normal
    distribution.  The reference's formula, in float64 from one launch with four orders.
    """
    m, xd, as_numpy, squeeze = _planes(root, x, 4, 'kurtosis')
    if m is None:
        return _empty(xd, as_numpy)
    m = m.double()
    g1 = m[0] ** 2.0
    g2 = m[1] - g1
    g3 = 4.0 * (g1 ** 2.0 + m[0] * m[2])
    g4 = m[1] * (8.0 * g1 - m[1])
    return _finish(root, -2.0 + (m[3] - g3 + g4) / (g2 ** 2.0), float('nan'), xd, as_numpy, squeeze)
