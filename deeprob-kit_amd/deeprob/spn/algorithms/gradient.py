"""``eval_backward`` of a vanilla SPN (reference: deeprob/spn/algorithms/gradient.py:13-63) on the HIP evaluator."""
import ctypes
from typing import Union

import numpy as np
import torch

from deeprob.hip import load_library, call, ptr, stream_ptr, require_device_f32
from deeprob.spn.structure.io import FlatSpn


def eval_backward(root: FlatSpn, lls: Union[np.ndarray, torch.Tensor]) -> Union[np.ndarray, torch.Tensor]:
    """
    Compute the log-gradients at each SPN node.

    :param root: The SPN (as loaded by ``deeprob.spn.structure.io.load_spn_json``).
    :param lls: The log-likelihoods at each node ``[n_nodes, B]``, as ``log_likelihood(..., return_results=True)``
                returns them (numpy, or a tensor on a HIP device).
    :return: The log-gradients w.r.t. the nodes ``[n_nodes, B]`` float32 (numpy in, numpy out).
    :raises ValueError: If the SPN is not smooth / decomposable, or ``lls`` has not one row per node.
    """
    if not isinstance(root, FlatSpn):
        raise TypeError("eval_backward works on the FlatSpn returned by deeprob.spn.structure.io.load_spn_json")
    root.check()
    if len(lls.shape) != 2 or lls.shape[0] != root.n_nodes:
        raise ValueError("Incompatible log-likelihoods broadcasting at each node")
    lib = load_library()
    as_numpy = not isinstance(lls, torch.Tensor)
    if as_numpy:
        lls = torch.from_numpy(np.ascontiguousarray(lls, dtype=np.float32)).to(
            torch.device('cuda', torch.cuda.current_device()))
    ld = require_device_f32(lls, 'lls')
    B, dev = ld.shape[1], ld.device
    grads = torch.empty_like(ld)
    rec = root.circuit(dev)
    call(lib.dpk_flat_spn_backward, ptr(ld), ptr(grads), B, ctypes.addressof(rec), stream_ptr(dev))
    return grads.cpu().numpy() if as_numpy else grads
