"""ctypes binding of ``libdeeprob_rat.so`` (the C ABI declared in ``include/deeprob_rat.h``, prefix ``dpr_``): exact
posterior moments of the unobserved variables of a RAT-SPN.  The prototypes and the ``DPR_*`` constants are read from the
header with the parser of ``deeprob.hip``; nothing of them is written down a second time.  There is no CPU fallback: a
missing library raises.
"""
import ctypes

import torch

from deeprob import hip
from deeprob.hip import HipError

BINDING = hip.RAT
SIGNATURES, CONSTANTS = BINDING.signatures, BINDING.constants
globals().update(CONSTANTS)
load_library, call, _read_header = BINDING.load, BINDING.call, BINDING.read_header
hip.bound_module(__name__)         # LIB_PATH, HEADER_PATH, ABI_VERSION and _lib are views of BINDING


def ratspn_moments(dist: int, lctx, x: torch.Tensor, y, acts, logws, src: torch.Tensor, p0: torch.Tensor, p1,
                   all_classes: bool = False, want_var: bool = True, want_leaf_flow: bool = False):
    """``dpr_ratspn_moments``: the posterior mean (and variance) of every NaN entry of ``x`` [B, D] given the row's other
    entries, top-down in one launch.  ``lctx``: the model's ``deeprob.hip.ops.LeafContext``; ``acts``: [leaf output, sum
    level 1 output, ...] of the bottom-up pass under ``x``; ``logws``: the log-softmax weights of the sum levels
    1 .. depth-1, then of the root; ``src``, ``p0``, ``p1``: the tables of ``deeprob.hip.ops.ratspn_topdown``.  ``y``: [B]
    integer labels (a label outside ``[0, C)`` raises ``ValueError``) or None: class 0, or with ``all_classes`` the mixture
    over the classes under the uniform class prior.  Returns ``(mean, var or None, leaf_flow or None)``; ``leaf_flow`` is
    ``[B, reps 2^depth, I]``.  A shape outside the kernel's envelope raises ``NotImplementedError``."""
    if not p0.is_cuda:
        raise HipError("the model lives on '{}': the deeprob HIP path only computes posterior moments on a HIP device "
                       "(there is no CPU fallback)".format(p0.device))
    lib = load_library()
    depth, reps, D, device = lctx.depth, lctx.reps, lctx.D, p0.device
    G0 = 1 << depth
    if x.dim() != 2 or x.shape[1] != D:
        raise ValueError("ratspn_moments: expected x of shape (B, {}), got {}".format(D, tuple(x.shape)))
    B = int(x.shape[0])
    keep = []

    def dev(t, name, shape):
        return hip.require_model_f32('ratspn_moments', t, name, shape, device, keep)

    xd = dev(x, 'x', (B, D))
    if len(acts) != depth:
        raise ValueError('ratspn_moments: %d activation tensors for depth %d' % (len(acts), depth))
    if len(logws) != depth:
        raise ValueError('ratspn_moments: %d weight tensors for depth %d' % (len(logws), depth))
    act_arr = (ctypes.c_void_p * depth)()
    for t, a in enumerate(acts):
        act_arr[t] = hip.ptr(dev(a, 'act[%d]' % t, (B, reps * (G0 >> t), lctx.I if t == 0 else lctx.S)))
    logw_arr = (ctypes.c_void_p * (depth + 1))()
    for t, w in enumerate(logws[:-1], start=1):
        n = lctx.I if t == 1 else lctx.S
        logw_arr[t] = hip.ptr(dev(w, 'logw[%d]' % t, (reps * (G0 >> t), lctx.S, n * n)))
    n = lctx.I if depth == 1 else lctx.S
    logw_arr[depth] = hip.ptr(dev(logws[-1], 'root logw', (lctx.C, reps * n * n)))
    if src.dtype != torch.int32 or tuple(src.shape) != (reps, D) or not src.is_contiguous() or src.device != device:
        raise ValueError("ratspn_moments: expected src as a contiguous int32 ({}, {}) tensor on '{}'".format(reps, D, device))
    p0d = dev(p0, 'p0', (reps * G0, lctx.I, lctx.d))
    p1d = dev(p1, 'p1', (reps * G0, lctx.I, lctx.d)) if p1 is not None else None
    if dist == DPR_DIST_GAUSSIAN and p1d is None:
        raise ValueError('ratspn_moments: Gaussian leaves need their scales')
    yd = None if y is None else hip.require_labels('ratspn_moments', y, B, lctx.C, device)
    mean = torch.empty((B, D), dtype=torch.float32, device=device)
    var = torch.empty((B, D), dtype=torch.float32, device=device) if want_var else None
    flow = torch.empty((B, reps * G0, lctx.I), dtype=torch.float32, device=device) if want_leaf_flow else None
    if B > 0:
        call(lib.dpr_ratspn_moments, int(dist), B, D, depth, reps, lctx.I, lctx.S, lctx.C, lctx.d, hip.ptr(xd), hip.ptr(yd),
             int(bool(all_classes)), ctypes.cast(act_arr, ctypes.c_void_p), ctypes.cast(logw_arr, ctypes.c_void_p),
             hip.ptr(src), hip.ptr(p0d), hip.ptr(p1d), hip.ptr(mean), hip.ptr(var), hip.ptr(flow), hip.stream_ptr(device))
    return mean, var, flow
