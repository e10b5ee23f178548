"""ctypes binding of ``include/deeprob_dgcm.h`` (prefix ``dpm_``) onto ``libdeeprob_dgc.so``: exact posterior moments of the
missing entries of a DGC-SPN.  The prototypes and the ``DPM_*`` constants are read from the header with the parser of
``deeprob.hip``; nothing of them is written down a second time.  There is no CPU fallback: a missing library raises.
"""
import ctypes

import torch

from deeprob import hip
from deeprob.hip import HipError, dgc

BINDING = hip.DGCM
SIGNATURES, CONSTANTS = BINDING.signatures, BINDING.constants
globals().update(CONSTANTS)
load_library, call, _read_header = BINDING.load, BINDING.call, BINDING.read_header
hip.bound_module(__name__)         # LIB_PATH, HEADER_PATH, ABI_VERSION and _lib are views of BINDING

product_geometry = dgc.product_geometry


def _geometry_table(geom):
    return (ctypes.c_int32 * (len(geom) * dgc.DPG_GEOM_INTS))(*[int(v) for row in geom for v in row])


def workspace_bytes(n_rows: int, geom) -> int:
    """``dpm_dgcspn_moments_workspace_bytes``: what a launch over ``n_rows`` images of this geometry needs."""
    lib = load_library()
    return call(lib.dpm_dgcspn_moments_workspace_bytes, int(n_rows), len(geom), ctypes.cast(_geometry_table(geom), ctypes.c_void_p))


def dgcspn_moments(in_features, geom, classes: int, x: torch.Tensor, y, acts, logws, loc: torch.Tensor, scale: torch.Tensor,
                   ws: hip.Workspace, all_classes: bool = False, want_var: bool = True, want_leaf_flow: bool = False):
    """``dpm_dgcspn_moments``: the posterior mean (and variance) of every NaN entry of ``x`` [B, C, H, W] given the image's
    other entries, top-down in one launch.  ``geom``: :func:`product_geometry`; ``acts``: [leaf output, sum layer 1 output,
    ...] NCHW of the bottom-up pass under ``x``; ``logws``: the log-softmax weights of the sum layers 1 .. L-1, then of the
    root; ``ws``: the ``deeprob.hip.Workspace`` the flow maps of the work-groups live in.  ``y``: [B] integer labels (a label
    outside ``[0, classes)`` raises ``ValueError``) or None: class 0, or with ``all_classes`` the mixture over the classes
    under the uniform class prior.  Returns ``(mean, var or None, leaf_flow or None)``; ``leaf_flow`` is ``[B, K, H, W]``."""
    if not loc.is_cuda:
        raise HipError("the model lives on '{}': the deeprob HIP path only computes posterior moments on a HIP device "
                       "(there is no CPU fallback)".format(loc.device))
    lib = load_library()
    C, H, W = (int(v) for v in in_features)
    L, device = len(geom), loc.device
    if x.dim() != 4 or tuple(x.shape[1:]) != (C, H, W):
        raise ValueError("dgcspn_moments: expected x of shape (B, {}, {}, {}), got {}".format(C, H, W, tuple(x.shape)))
    B = int(x.shape[0])
    keep = []

    def dev(t, name, shape):
        return hip.require_model_f32('dgcspn_moments', t, name, shape, device, keep)

    if len(acts) != L:
        raise ValueError('dgcspn_moments: %d activation tensors for %d levels' % (len(acts), L))
    if len(logws) != L:
        raise ValueError('dgcspn_moments: %d weight tensors for %d levels' % (len(logws), L))
    xd = dev(x, 'x', (B, C, H, W))
    act_arr = (ctypes.c_void_p * L)()
    for t, a in enumerate(acts):
        act_arr[t] = hip.ptr(dev(a, 'act[%d]' % t, (B,) + tuple(geom[t][0:3])))
    logw_arr = (ctypes.c_void_p * (L + 1))()
    for t, w in enumerate(logws[:-1], start=1):
        logw_arr[t] = hip.ptr(dev(w, 'logw[%d]' % t, (geom[t][0],) + tuple(geom[t - 1][3:6])))
    logw_arr[L] = hip.ptr(dev(logws[-1], 'root logw', (classes, geom[-1][3] * geom[-1][4] * geom[-1][5])))
    K = geom[0][0]
    locd, scaled = dev(loc, 'loc', (K, C, H, W)), dev(scale, 'scale', (K, C, H, W))
    yd = None if y is None else hip.require_labels('dgcspn_moments', y, B, classes, device)
    garr = _geometry_table(geom)
    mean = torch.empty((B, C, H, W), dtype=torch.float32, device=device)
    var = torch.empty((B, C, H, W), dtype=torch.float32, device=device) if want_var else None
    flow = torch.empty((B, K, H, W), dtype=torch.float32, device=device) if want_leaf_flow else None
    if B > 0:
        n_bytes = call(lib.dpm_dgcspn_moments_workspace_bytes, B, L, ctypes.cast(garr, ctypes.c_void_p))
        buf = ws.get(n_bytes, device)
        call(lib.dpm_dgcspn_moments, B, C, H, W, K, L, ctypes.cast(garr, ctypes.c_void_p), classes, int(bool(all_classes)),
             hip.ptr(xd), hip.ptr(yd), ctypes.cast(act_arr, ctypes.c_void_p), ctypes.cast(logw_arr, ctypes.c_void_p),
             hip.ptr(locd), hip.ptr(scaled), hip.ptr(mean), hip.ptr(var), hip.ptr(flow), hip.ptr(buf), n_bytes,
             hip.stream_ptr(device))
    return mean, var, flow
