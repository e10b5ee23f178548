"""``log_likelihood`` and ``mpe`` of a vanilla SPN (reference: deeprob/spn/algorithms/inference.py:37-79) on the HIP
evaluator.

There is no CPU path: the inputs are moved to the HIP device (or already live there) and the circuit is walked
by ``dpk_flat_spn_forward`` / ``dpk_flat_spn_topdown``.
"""
import ctypes
from typing import Tuple, Union

import numpy as np
import torch

from deeprob.hip import load_library, call, ptr, stream_ptr, require_device_f32, HipError
from deeprob.spn.structure.io import FlatSpn


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
