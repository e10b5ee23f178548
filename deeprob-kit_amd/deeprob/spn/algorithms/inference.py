"""``likelihood``, ``log_likelihood`` and ``mpe`` of a vanilla SPN (reference: deeprob/spn/algorithms/inference.py:13-79)
on the HIP evaluator, and ``posterior``: the exact posterior of one discrete variable, which the reference has no
function for.

There is no CPU path: the inputs are moved to the HIP device (or already live there) and the circuit is walked
by ``dpk_flat_spn_forward`` / ``dpk_flat_spn_topdown`` / ``dpq_flat_spn_posterior``.
"""
import ctypes
from typing import Tuple, Union

import numpy as np
import torch

from deeprob.hip import load_library, call, ptr, stream_ptr, require_device_f32, HipError
from deeprob.spn.structure.io import FlatSpn, KIND


def likelihood(root: FlatSpn, x: Union[np.ndarray, torch.Tensor], return_results: bool = False, n_jobs: int = 0
               ) -> Union[np.ndarray, torch.Tensor, Tuple]:
    """
    Compute the likelihoods of the SPN given some inputs (reference inference.py:13-34): ``exp`` of
    :func:`log_likelihood`, with the same arguments and the same kinds of result.
    """
    res = log_likelihood(root, x, return_results=return_results, n_jobs=n_jobs)
    exp = lambda v: torch.exp(v) if isinstance(v, torch.Tensor) else np.exp(v)
    return (exp(res[0]), exp(res[1])) if return_results else exp(res)


def log_likelihood(root: FlatSpn, x: Union[np.ndarray, torch.Tensor], return_results: bool = False, n_jobs: int = 0
                   ) -> Union[np.ndarray, torch.Tensor, Tuple]:
    """
    Compute the logarithmic likelihoods of the SPN given some inputs.

    :param root: The SPN (as loaded by ``deeprob.spn.structure.io.load_spn_json``).
    :param x: The inputs ``[B, n_features]``; they can be marginalized using NaNs.  A numpy array is evaluated on
              the current HIP device and numpy arrays come back (as the reference returns); a device tensor
              stays on its device.
    :param return_results: Whether to also return the log likelihoods of each node, ``[n_nodes, B]``.
    :param n_jobs: Accepted for compatibility (the reference's joblib thread count).
    :return: The log likelihood values ``[B]`` float32.  Additionally, the values of each node.
    :raises ValueError: If the SPN is not smooth / decomposable, or the inputs do not cover its scope.
    """
    if not isinstance(root, FlatSpn):
        raise TypeError("log_likelihood evaluates the FlatSpn returned by deeprob.spn.structure.io.load_spn_json")
    root.check()
    lib = load_library()
    as_numpy = not isinstance(x, torch.Tensor)
    if as_numpy:
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.device('cuda', torch.cuda.current_device()))
    xd = require_device_f32(x, 'x')
    if xd.dim() != 2 or xd.shape[1] < root.n_features:
        raise ValueError("expected inputs [B, >= {}], got {}".format(root.n_features, tuple(xd.shape)))
    B, D = xd.shape
    dev = xd.device
    a = root.device_arrays(dev)
    out = torch.empty(B, dtype=torch.float32, device=dev)
    table = torch.empty((root.n_nodes, B), dtype=torch.float32, device=dev) if return_results else None
    ws = None
    if table is None:
        n = call(lib.dpk_flat_spn_workspace_bytes, B, root.n_nodes, root.n_slots)
        if n > 0:
            ws = torch.empty(int(n), dtype=torch.uint8, device=dev)
    call(lib.dpk_flat_spn_forward, ptr(xd), B, D, root.n_nodes, root.root, ptr(a['order']), ptr(a['kind']),
                                   ptr(a['arg0']), ptr(a['arg1']), ptr(a['arg2']), ptr(a['par0']), ptr(a['par1']),
                                   ptr(a['child_index']), ptr(a['child_weight']), ptr(a['cat_value']),
                                   ptr(a['cat_logp']), root.n_slots, ptr(a['node_slot']), ptr(a['child_slot']),
                                   ptr(out), ptr(table), ptr(ws),
                                   0 if ws is None else ws.numel(), stream_ptr(dev))
    if as_numpy:
        out = out.cpu().numpy()
        table = None if table is None else table.cpu().numpy()
    return (out, table) if return_results else out


def top_down(root: FlatSpn, x: Union[np.ndarray, torch.Tensor], inplace: bool, mode: int, seed: int, what: str
             ) -> Union[np.ndarray, torch.Tensor]:
    """Bottom-up values, then the walk from the root that fills the NaN entries of ``x`` inside the scope
    (reference evaluation.py:99-177) -- one launch of ``dpk_flat_spn_topdown``; shared by ``mpe`` and ``sample``."""
    if not isinstance(root, FlatSpn):
        raise TypeError("{} works on the FlatSpn returned by deeprob.spn.structure.io.load_spn_json".format(what))
    root.check()
    lib = load_library()
    as_numpy = not isinstance(x, torch.Tensor)
    if as_numpy:
        x = np.asarray(x)
        if inplace and x.dtype != np.float32:
            raise ValueError("inplace=True needs a float32 array")
        host = x if x.dtype == np.float32 and x.flags.c_contiguous else np.ascontiguousarray(x, dtype=np.float32)
        xd = torch.from_numpy(host).to(torch.device('cuda', torch.cuda.current_device()))
    else:
        if not x.is_cuda:
            raise HipError("x lives on '{}': the deeprob HIP path only works on tensors on a HIP device "
                           "(there is no CPU fallback)".format(x.device))
        direct = x.dtype == torch.float32 and x.is_contiguous()
        if inplace and not direct:
            raise ValueError("inplace=True needs a contiguous float32 tensor")
        xd = x if inplace else (x.clone() if direct else require_device_f32(x, 'x').clone())
    if xd.dim() != 2 or xd.shape[1] < root.n_features:
        raise ValueError("expected inputs [B, >= {}], got {}".format(root.n_features, tuple(xd.shape)))
    B, D = xd.shape
    dev = xd.device
    rec = root.circuit(dev)
    n = call(lib.dpk_flat_spn_topdown_workspace_bytes, B, ctypes.addressof(rec))
    ws = torch.empty(int(n), dtype=torch.uint8, device=dev) if n > 0 else None
    call(lib.dpk_flat_spn_topdown, ptr(xd), B, D, ctypes.addressof(rec), mode, seed, ptr(ws),
                                   0 if ws is None else ws.numel(), stream_ptr(dev))
    if not as_numpy:
        return xd
    out = xd.cpu().numpy()
    if inplace:
        x[...] = out
        return x
    return out


def mpe(root: FlatSpn, x: Union[np.ndarray, torch.Tensor], inplace: bool = False, n_jobs: int = 0
        ) -> Union[np.ndarray, torch.Tensor]:
    """
    Compute the Most Probable Explanation of a SPN given some inputs (reference inference.py:61-79).

    :param root: The SPN (as loaded by ``deeprob.spn.structure.io.load_spn_json``).
    :param x: The inputs ``[B, >= n_features]``; the NaN entries inside the SPN's scope are filled, everything else
              comes back bit for bit.  A numpy array gives a numpy array (computed on the current HIP device), a
              device tensor stays on its device.
    :param inplace: Whether to write into ``x`` itself (float32).
    :param n_jobs: Accepted for compatibility (the reference's joblib thread count).
    :return: The NaN-filled inputs.
    :raises ValueError: If the SPN is not smooth / decomposable, or the inputs do not cover its scope.
    """
    return top_down(root, x, inplace, 0, 0, 'mpe')


def check_inputs(root: FlatSpn, x: Union[np.ndarray, torch.Tensor], what: str):
    """The argument checks of the read-only posterior queries (``posterior`` here, ``deeprob.spn.algorithms.moments``),
    those of ``mpe``; nothing touches a device.  Returns ``(x, as_numpy)`` with ``x`` a numpy array (whatever was given
    that is not a tensor) or the device tensor itself.

    :raises TypeError: If ``root`` is not a FlatSpn.
    :raises ValueError: If the SPN is not smooth / decomposable, or the inputs do not cover its scope.
    :raises HipError: If ``x`` is a tensor that does not live on a HIP device.
    """
    if not isinstance(root, FlatSpn):
        raise TypeError("{} works on the FlatSpn returned by deeprob.spn.structure.io.load_spn_json".format(what))
    root.check()
    as_numpy = not isinstance(x, torch.Tensor)
    if as_numpy:
        x = np.asarray(x)
    elif not x.is_cuda:
        raise HipError("x lives on '{}': the deeprob HIP path only works on tensors on a HIP device "
                       "(there is no CPU fallback)".format(x.device))
    if x.ndim != 2 or x.shape[1] < root.n_features:
        raise ValueError("expected inputs [B, >= {}], got {}".format(root.n_features, tuple(x.shape)))
    return x, as_numpy


def upload_inputs(x, as_numpy: bool):
    """What :func:`check_inputs` returned as a contiguous float32 tensor on a HIP device (a numpy array goes to the current
    one); ``None`` for ``B = 0``: nothing is launched then, and a numpy array needs no device."""
    if x.shape[0] == 0:
        return None
    if as_numpy:
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.device('cuda', torch.cuda.current_device()))
    return require_device_f32(x, 'x')


def posterior_values(root: FlatSpn, var: int) -> np.ndarray:
    """The default ``values`` of :func:`posterior`: ``[0, 1]`` for a Bernoulli variable, the sorted union of the
    categories of the variable's leaves for a Categorical one.  (Structure, not parameters: kept per variable.)

    :raises ValueError: If ``var`` is outside the scope or continuous (Uniform / Gaussian leaves).
    """
    var = int(var)
    cache = root.__dict__.setdefault('_posterior_values', {})
    if var in cache:
        return cache[var]
    if not 0 <= var < root.n_features:
        raise ValueError("variable {} is outside the SPN's {} features".format(var, root.n_features))
    leaves = np.flatnonzero((root.kind >= KIND['Bernoulli']) & (root.arg0 == var))
    if not len(leaves):
        raise ValueError("variable {} is outside the SPN's scope".format(var))
    kinds = root.kind[leaves]
    continuous = leaves[(kinds != KIND['Bernoulli']) & (kinds != KIND['Categorical'])]
    if len(continuous):
        i = int(continuous[0])
        raise ValueError("variable {} is continuous ({} leaf #{}): posterior gives the probabilities of the values of "
                         "a discrete variable".format(var, root.classes[i], i))
    support = [np.array([0, 1])] if (kinds == KIND['Bernoulli']).any() else []
    support += [root.cat_value[root.arg1[i]:root.arg1[i] + root.arg2[i]] for i in leaves[kinds == KIND['Categorical']]]
    cache[var] = np.unique(np.concatenate(support)).astype(np.float32)
    return cache[var]


def posterior(root: FlatSpn, x: Union[np.ndarray, torch.Tensor], var: int, values=None
              ) -> Union[np.ndarray, torch.Tensor]:
    """
    The exact posterior ``p(x_var = v | the row's evidence)`` of one discrete variable, for every row: one bottom-up and
    one top-down pass in one launch of ``dpq_flat_spn_posterior`` (include/deeprob_spnq.h).  On the circuit of
    ``learn_classifier`` with ``var`` the class column this is the class posterior, which ``mpe`` (the max-product branch
    at every sum node) neither maximises nor reports.

    :param root: The SPN (a FlatSpn, as ``load_spn_json``, ``learn_spn``, ``learn_classifier`` return).
    :param x: The inputs ``[B, >= n_features]``, NaN = not observed.  A numpy array gives a numpy array (computed on the
              current HIP device), a device tensor stays on its device.
    :param var: The variable: Bernoulli or Categorical leaves.
    :param values: The values ``[V]`` to report, whole numbers (a discrete variable takes no others, and the kernel
                   matches a category by the integer part of the value); default ``[0, 1]`` for a Bernoulli variable, the
                   sorted union of the categories of the variable's leaves for a Categorical one.  A value outside a
                   leaf's support has probability 0 under that leaf.
    :return: ``[B, V]`` float32.  Where ``x[b, var]`` is observed the row is the indicator of ``values == x[b, var]``; a
             row whose evidence has probability zero is NaN.
    :raises ValueError: If ``var`` is continuous or outside the scope, if ``values`` is not ``[V >= 1]`` whole numbers, or
                        on a bad shape of ``x``.
    """
    from deeprob.hip import spnq
    x, as_numpy = check_inputs(root, x, 'posterior')         # (every argument error before anything is uploaded)
    default = posterior_values(root, var)
    values = default if values is None else np.ascontiguousarray(values, dtype=np.float32)
    if values.ndim != 1 or len(values) == 0:
        raise ValueError("expected values [V], V >= 1, got {}".format(tuple(values.shape)))
    if not (np.isfinite(values) & (values == np.trunc(values))).all():
        raise ValueError("the values of a discrete variable are whole numbers, got {}".format(values.tolist()))
    xd = upload_inputs(x, as_numpy)
    if xd is None:
        return np.empty((0, len(values)), np.float32) if as_numpy else x.new_empty((0, len(values)), dtype=torch.float32)
    out = spnq.flat_spn_posterior(root, xd, spnq.DPQ_MODE_VALUES, var=int(var), values=values)
    return out.cpu().numpy() if as_numpy else out
