"""ctypes binding of ``libdeeprob_dgc.so`` (the C ABI declared in ``include/deeprob_dgc.h``, prefix ``dpg_``): the
top-down pass of a DGC-SPN.  The prototypes and the ``DPG_*`` constants are read from the header with the parser of
``deeprob.hip``; nothing of them is written down a second time.  There is no CPU fallback: a missing library raises.
"""
import ctypes

import torch

from deeprob import hip
from deeprob.hip import HipError

BINDING = hip.DGC
SIGNATURES, CONSTANTS = BINDING.signatures, BINDING.constants
globals().update(CONSTANTS)
load_library, call, _read_header = BINDING.load, BINDING.call, BINDING.read_header
hip.bound_module(__name__)         # LIB_PATH, HEADER_PATH, ABI_VERSION and _lib are views of BINDING


def product_geometry(layers):
    """``[L][DPG_GEOM_INTS]`` rows of the header's geometry table for these SpatialProductLayers, bottom to top."""
    rows = []
    for p in layers:
        if tuple(p.kernel_size) != (2, 2) or p.stride[0] != p.stride[1] or p.dilation[0] != p.dilation[1]:
            raise ValueError("the top-down pass covers 2x2 windows with one stride and one dilation, got kernel {} stride {} "
                             "dilation {}".format(p.kernel_size, p.stride, p.dilation))
        rows.append(list(p.in_features) + list(p.out_features) + list(p.pad) + [p.stride[0], p.dilation[0], int(p.depthwise)])
    assert all(len(r) == DPG_GEOM_INTS for r in rows)
    return rows


def dgcspn_topdown(mode: int, n_samples: int, in_features, geom, classes: int, x, y, acts, logws, loc: torch.Tensor,
                   scale: torch.Tensor, seed: int, want_choice: bool = False, labels_trusted: bool = False):
    """``dpg_dgcspn_topdown``: DgcSpn.sample (mode 1) / DgcSpn.sample_conditional (mode 2) / DgcSpn.mpe_completion (mode 3,
    which ignores ``seed``) top-down in one launch.
    ``geom``: :func:`product_geometry`; ``acts``: [leaf output, sum layer 1 output, ...] NCHW (modes 2 and 3); ``logws``: the
    log-softmax weights of the sum layers 1 .. L-1, then of the root.  Returns ``[B, C, H, W]`` (and the ``[B, 1 + H W]``
    int32 choices when asked).  A label outside ``[0, classes)`` raises ``ValueError`` (``labels_trusted``: the caller drew
    them itself, no check and no read-back)."""
    if not loc.is_cuda:
        raise HipError("the model lives on '{}': the deeprob HIP path only samples on a HIP device (there is no CPU "
                       "fallback)".format(loc.device))
    lib = load_library()
    C, H, W = (int(v) for v in in_features)
    L, B, device = len(geom), int(n_samples), loc.device
    keep = []

    def dev(t, name, shape):
        return hip.require_model_f32('dgcspn_topdown', t, name, shape, device, keep)

    if len(logws) != L:
        raise ValueError('dgcspn_topdown: %d weight tensors for %d levels' % (len(logws), L))
    act_arr = (ctypes.c_void_p * L)()
    xd = None
    if mode in (DPG_MODE_POSTERIOR, DPG_MODE_MPE):
        if acts is None:
            raise ValueError('dgcspn_topdown: mode %d needs the bottom-up activations' % mode)
        if len(acts) != L:
            raise ValueError('dgcspn_topdown: %d activation tensors for %d levels' % (len(acts), L))
        xd = dev(x, 'x', (B, C, H, W))
        for t, a in enumerate(acts):
            act_arr[t] = hip.ptr(dev(a, 'act[%d]' % t, (B,) + tuple(geom[t][0:3])))
    logw_arr = (ctypes.c_void_p * (L + 1))()
    for t, w in enumerate(logws[:-1], start=1):
        logw_arr[t] = hip.ptr(dev(w, 'logw[%d]' % t, (geom[t][0],) + tuple(geom[t - 1][3:6])))
    logw_arr[L] = hip.ptr(dev(logws[-1], 'root logw', (classes, geom[-1][3] * geom[-1][4] * geom[-1][5])))
    K = geom[0][0]
    locd, scaled = dev(loc, 'loc', (K, C, H, W)), dev(scale, 'scale', (K, C, H, W))
    yd = None if y is None else hip.require_labels('dgcspn_topdown', y, B, classes, device, trusted=labels_trusted)
    garr = (ctypes.c_int32 * (L * DPG_GEOM_INTS))(*[int(v) for row in geom for v in row])
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=device)
    choice = torch.empty((B, 1 + H * W), dtype=torch.int32, device=device) if want_choice else None
    call(lib.dpg_dgcspn_topdown, mode, B, C, H, W, K, L, ctypes.cast(garr, ctypes.c_void_p), classes, hip.ptr(xd), hip.ptr(yd),
         ctypes.cast(act_arr, ctypes.c_void_p), ctypes.cast(logw_arr, ctypes.c_void_p), hip.ptr(locd), hip.ptr(scaled),
         int(seed) & 0xFFFFFFFFFFFFFFFF, hip.ptr(out), hip.ptr(choice), hip.stream_ptr(device))
    return (out, choice) if want_choice else out
