"""ctypes binding of ``libdeeprob_spnq.so`` (the C ABI declared in ``include/deeprob_spnq.h``, prefix ``dpq_``): posterior
queries on a node-graph SPN -- conditional moments and the posterior of one discrete variable.  The prototypes, the
``DPQ_*`` constants and the circuit record are read from the header with the parser of ``deeprob.hip``; nothing of them is
written down a second time.  There is no CPU fallback: a missing library or a CPU tensor raises.
"""
import ctypes

import numpy as np
import torch

from deeprob import hip
from deeprob.hip import HipError

BINDING = hip.SPNQ
SIGNATURES, CONSTANTS = BINDING.signatures, BINDING.constants
globals().update(CONSTANTS)
load_library, call, _read_header = BINDING.load, BINDING.call, BINDING.read_header
hip.bound_module(__name__)         # LIB_PATH, HEADER_PATH, ABI_VERSION and _lib are views of BINDING

#: the header's mirror of ``dpk_flat_spn_circuit``; the record ``FlatSpn.circuit(device)`` builds is passed as it is
FlatSpnCircuit = BINDING.struct('dpq_flat_spn_circuit')


def leaf_table(spn):
    """``(var_leaf_off [n_features + 1], var_leaf [n_leaves])`` int32: the node ids of the leaves over each variable, in
    increasing node id (the header's table)."""
    leaves = np.flatnonzero(spn.kind >= 2)
    var = spn.arg0[leaves]
    keep = np.argsort(var, kind='stable')            # (leaves is increasing, so ids stay increasing per variable)
    off = np.zeros(spn.n_features + 1, np.int32)
    off[1:] = np.cumsum(np.bincount(var, minlength=spn.n_features))
    return off, leaves[keep].astype(np.int32)


def _device_leaf_table(spn, device):
    cache = spn.__dict__.setdefault('_leaf_tables', {})      # (structure, not parameters: uploaded once per device)
    key = str(device)
    if key not in cache:
        off, leaf = leaf_table(spn)
        cache[key] = (torch.from_numpy(off).to(device), torch.from_numpy(leaf).to(device))
    return cache[key]


def flat_spn_posterior(spn, xd: torch.Tensor, mode: int, n_orders: int = 0, var: int = 0, values=None,
                       force_workspace: bool = False) -> torch.Tensor:
    """``dpq_flat_spn_posterior`` on the device tensor ``xd [B, D]`` (contiguous float32): ``[n_orders, B, D]`` moments
    (mode ``DPQ_MODE_MOMENTS``) or ``[B, V]`` probabilities of ``values`` for variable ``var`` (``DPQ_MODE_VALUES``).
    ``force_workspace``: take the workspace route whatever the circuit's size (the two routes give the same bits)."""
    if not xd.is_cuda:
        raise HipError("x lives on '{}': the deeprob HIP path only works on tensors on a HIP device (there is no CPU "
                       "fallback)".format(xd.device))
    lib = load_library()
    B, D = xd.shape
    dev = xd.device
    flags = DPQ_FLAG_FORCE_WORKSPACE if force_workspace else 0
    vd = None
    if mode == DPQ_MODE_VALUES:
        vd = torch.as_tensor(np.ascontiguousarray(values, dtype=np.float32)).to(dev)
        out = torch.empty((B, vd.numel()), dtype=torch.float32, device=dev)
    else:
        out = torch.empty((n_orders, B, D), dtype=torch.float32, device=dev)
    if B == 0:
        return out
    rec = spn.circuit(dev)
    off, leaf = _device_leaf_table(spn, dev)
    n = call(lib.dpq_flat_spn_posterior_workspace_bytes, B, ctypes.addressof(rec), flags)
    ws = torch.empty(int(n), dtype=torch.uint8, device=dev) if n > 0 else None
    call(lib.dpq_flat_spn_posterior, hip.ptr(xd), B, D, ctypes.addressof(rec), hip.ptr(off), hip.ptr(leaf), leaf.numel(),
         mode, n_orders, var, hip.ptr(vd), 0 if vd is None else vd.numel(), hip.ptr(out), flags, hip.ptr(ws),
         0 if ws is None else ws.numel(), hip.stream_ptr(dev))
    return out
