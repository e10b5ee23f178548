"""Operators of the masked autoregressive flow (AutoregressiveLayer, MaskedLinear) on top of the C ABI (csrc/maf.hip).

Routing of one AutoregressiveLayer:

| call                                   | condition                                   | route                                  |
|----------------------------------------|---------------------------------------------|----------------------------------------|
| apply_backward, no graph               | depth 1, units <= 256, D >= 2, packing of   | fused density kernel                   |
|                                        | inputs and outputs in monotone order        |                                        |
| apply_backward, no graph               | otherwise                                   | chained masked GEMMs + epilogue        |
| apply_backward, graph wanted           | any                                         | autograd op on the chained route       |
| apply_forward, no graph                | depth 1, units <= 128                       | sampling kernel, one launch            |
| apply_forward, no graph                | 2-8 hidden layers, <= 512 units in all,     | deep sampling kernel, one launch       |
|                                        | masks autoregressive in the layer's order   |                                        |
| apply_forward, no graph                | otherwise                                   | step loop of the conditioner op        |
| apply_forward, graph wanted (rsample)  | any                                         | step loop of the differentiable op     |

The fused density kernel is chosen by measured cost: with degree-sorted packing that is not a monotone order of the
variables (random degrees) its gathers and scatters made it slower than the chained route.

The step loop is the reference's own algorithm (autoregressive.py:81-121): D evaluations of the conditioner per layer,
each one HIP conditioner op, torch only for the per-column glue.  It is slow by design.
"""
import ctypes
from typing import Tuple

import numpy as np
import torch

from deeprob.hip import load_library, call, ptr, stream_ptr, require_device_f32, HipError

FUSED_MAX_UNITS = 256
SAMPLE_MAX_UNITS = 128
DEEP_MAX_HIDDEN = 8
DEEP_MAX_UNITS = 512
CHAIN_CONDITIONER, CHAIN_DENSITY, CHAIN_BACKWARD = 0, 1, 2     # dpk_maf_chain_workspace_bytes modes
_ACT_CODES = {torch.nn.ReLU: 0, torch.nn.LeakyReLU: 1, torch.nn.Softplus: 2, torch.nn.Tanh: 3, torch.nn.Sigmoid: 4}


def _wants_graph(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _linears(layer):
    return [m for m in layer.network if hasattr(m, 'mask')]


def _activation(layer) -> int:
    """Code of the conditioner's activation (the modules get_activation_class builds, with their default settings)."""
    mods = [m for m in layer.network if not hasattr(m, 'mask')]
    if not mods:
        return 0
    m = mods[0]
    code = _ACT_CODES.get(type(m))
    if code is None or any(type(o) is not type(m) for o in mods):
        raise HipError("AutoregressiveLayer: activation {} has no HIP kernel".format(type(m).__name__))
    if (code == 1 and m.negative_slope != 0.01) or (code == 2 and (m.beta != 1 or m.threshold != 20)):
        raise HipError("AutoregressiveLayer: only the default LeakyReLU / Softplus settings are built")
    return code


def _params(layer):
    lins = _linears(layer)
    W = [require_device_f32(m.weight, 'weight') for m in lins]
    M = [require_device_f32(m.mask, 'mask') for m in lins]
    b = [require_device_f32(m.bias, 'bias') for m in lins]
    return lins, W, M, b


def _chain_arrays(W, M, b):
    n = len(W)
    Wp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in W])
    Mp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in M])
    bp = (ctypes.c_void_p * n)(*[t.data_ptr() for t in b])
    widths = (ctypes.c_int32 * n)(*[t.shape[0] for t in W])
    return Wp, Mp, bp, widths


def _chain_bytes(B: int, D: int, widths, mode: int) -> int:
    return int(call(load_library().dpk_maf_chain_workspace_bytes, B, D, len(widths) - 1, widths, mode))


def _check_input(x: torch.Tensor, layer, name: str) -> torch.Tensor:
    x = require_device_f32(x, name)
    if x.dim() != 2 or x.shape[1] != layer.in_features:
        raise HipError("AutoregressiveLayer: {} of shape {} for {} features".format(name, tuple(x.shape),
                                                                                    layer.in_features))
    return x


def _int_table(layer, key, values: np.ndarray, device) -> torch.Tensor:
    hit = layer.__dict__.setdefault('_int_tables', {})
    t = hit.get(key)
    if t is None or t.device != device:
        t = torch.tensor(np.asarray(values, dtype=np.int32), device=device)
        hit[key] = t
    return t


def packing_orders(m1: np.ndarray, m2: np.ndarray, step_order: np.ndarray):
    """(inputs, hidden units, outputs) packing orders of the fused kernel from boolean masks m1 [U, D], m2 [2D, U]; ties
    are broken by the layer's step order, so that degree-built masks pack the variables in that order."""
    D = m1.shape[1]
    step = np.empty(D, dtype=np.int64)
    step[step_order] = np.arange(D)
    i_ord = np.lexsort((step, -m1.sum(axis=0)))
    h_ord = np.argsort(m1.sum(axis=1), kind='stable')
    o_ord = np.lexsort((step, (m2[:D] | m2[D:]).sum(axis=1)))
    return i_ord, h_ord, o_ord


def _orders(layer, M1: torch.Tensor, M2: torch.Tensor):
    """Packing order of the fused kernel: inputs by decreasing fan-out, hidden units by increasing fan-in, outputs by
    increasing fan-in -- for degree-built masks each 32-row tile then needs a prefix of the packed K range only.  Derived
    from the mask buffers, cached per (address, version); the kernel reads which blocks are zero from the live masks, so
    a stale order costs speed, never correctness."""
    key = (M1.data_ptr(), M1._version, M2.data_ptr(), M2._version, M1.device)
    if layer._orders is None or layer._orders[0] != key:
        i_ord, h_ord, o_ord = packing_orders(M1.detach().cpu().numpy() != 0, M2.detach().cpu().numpy() != 0,
                                             np.asarray(layer.inv_ordering))
        dev = M1.device
        tabs = tuple(torch.tensor(a.astype(np.int32), device=dev) for a in (i_ord, h_ord, o_ord))
        monotone = all(len(a) < 2 or np.all(np.diff(a) == 1) or np.all(np.diff(a) == -1) for a in (i_ord, o_ord))
        layer._orders = (key, tabs, monotone)
    return layer._orders[1]


def _monotone_packing(layer) -> bool:
    lins = _linears(layer)
    _orders(layer, lins[0].mask, lins[1].mask)
    return layer._orders[2]


def deep_schedule(layer):
    """Finalisation schedule of a conditioner with >= 2 hidden layers, or None when its masks are not autoregressive
    in the layer's order.  A first-layer unit is final after the latest step among the variables it reads, a deeper
    unit after the latest of its inputs; the masks are autoregressive when every unit an output reads is final before
    that output's step.  Derived from the mask buffers, cached per (address, version) of every mask, as
    CouplingLayer1d._mask_counts.  Returns (event_ptr [D + 2], events) device tensors."""
    lins = _linears(layer)
    masks = [m.mask for m in lins]
    key = tuple((t.data_ptr(), t._version) for t in masks) + (masks[0].device,)
    hit = layer.__dict__.get('_deep_schedule')
    if hit is not None and hit[0] == key:
        return hit[1]
    D = layer.in_features
    order = np.asarray(layer.inv_ordering)
    step = np.empty(D, dtype=np.int64)
    step[order] = np.arange(D)
    fin = step
    finals = []
    for t in masks[:-1]:
        m = t.detach().cpu().numpy() != 0
        fin = np.where(m.any(axis=1), np.max(np.where(m, fin[None, :], -1), axis=1), -1)
        finals.append(fin)
    mo = masks[-1].detach().cpu().numpy() != 0
    need = np.max(np.where(mo, fin[None, :], -1), axis=1)         # latest final step among the units each output reads
    ok = bool(np.all(need[:D] < step) and np.all(need[D:] < step))
    plan = None
    if ok and all(int(f.max(initial=-1)) < (1 << 31) for f in finals):
        slots = [[] for _ in range(D + 1)]
        for l, f in enumerate(finals):
            for j in range(len(f)):
                slots[int(f[j]) + 1].append((l << 16) | j)
        ptr_ = np.zeros(D + 2, dtype=np.int32)
        ptr_[1:] = np.cumsum([len(sl) for sl in slots])
        ev = np.array([e for sl in slots for e in sl], dtype=np.int32)
        dev = masks[0].device
        plan = (torch.tensor(ptr_, device=dev), torch.tensor(ev, device=dev))
    layer._deep_schedule = (key, plan)
    return plan


def _step_order(layer, device) -> torch.Tensor:
    return _int_table(layer, ('inv_ordering', tuple(np.asarray(layer.inv_ordering).tolist())), layer.inv_ordering,
                      device)


# ---- density direction ------------------------------------------------------------------------------------------------
def density_chain(x: torch.Tensor, layer, ws: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """apply_backward on the chained route (masked GEMM per layer + epilogue)."""
    lib = load_library()
    B, D = x.shape
    lins, W, M, b = _params(layer)
    Wp, Mp, bp, widths = _chain_arrays(W, M, b)
    if ws is None:
        ws = layer._ws.get(_chain_bytes(B, D, widths, CHAIN_DENSITY), x.device)
    u = torch.empty_like(x)
    ildj = torch.empty(B, dtype=torch.float32, device=x.device)
    act_w = require_device_f32(layer.scale_act.weight, 'scale_act.weight')
    call(lib.dpk_maf_density_chain, ptr(x), B, D, len(W) - 1, Wp, Mp, bp, widths, _activation(layer), ptr(act_w),
                                    ptr(u), ptr(ildj), ptr(ws), ws.numel(), stream_ptr(x.device))
    return u, ildj


def fused_envelope(layer, D: int) -> bool:
    lins = _linears(layer)
    return len(lins) == 2 and lins[0].weight.shape[0] <= FUSED_MAX_UNITS and D >= 2


def fused_route(layer, D: int) -> bool:
    """Inside the fused kernel's envelope AND faster there than on the chained route (monotone packing order)."""
    return fused_envelope(layer, D) and _monotone_packing(layer)


def density_fused(x: torch.Tensor, layer, in_affine=None, ildj: torch.Tensor = None):
    """apply_backward on the fused kernel (depth 1).  in_affine: (scale, shift) [D] of an eval-mode batch norm folded in
    front; ildj: an accumulator [B] the layer's log-det is added to."""
    lib = load_library()
    B, D = x.shape
    lins, W, M, b = _params(layer)
    units = W[0].shape[0]
    ws = layer._ws.sized(lib.dpk_maf_density_workspace_bytes, D, units, device=x.device)
    i_ord, h_ord, o_ord = _orders(layer, M[0], M[1])
    u = torch.empty_like(x)
    accumulate = ildj is not None
    if ildj is None:
        ildj = torch.empty(B, dtype=torch.float32, device=x.device)
    sc, sh = in_affine if in_affine is not None else (None, None)
    act_w = require_device_f32(layer.scale_act.weight, 'scale_act.weight')
    call(lib.dpk_maf_density_forward, ptr(x), B, D, ptr(W[0]), ptr(M[0]), ptr(b[0]), ptr(W[1]), ptr(M[1]), ptr(b[1]),
                                      units, _activation(layer), ptr(act_w), ptr(sc), ptr(sh), ptr(i_ord), ptr(h_ord),
                                      ptr(o_ord), ptr(u), ptr(ildj), int(accumulate), ptr(ws), ws.numel(),
                                      stream_ptr(x.device))
    return u, ildj


class MafDensityFn(torch.autograd.Function):
    """apply_backward with autograd: chained route forward (its activations kept in a fresh workspace) and the
    chained backward (gradients w.r.t. x, every weight and bias, and the ScaledTanh weight)."""

    @staticmethod
    def forward(ctx, layer, x, act_w, *params):
        W, M, b = list(params[0::2]), [m.mask for m in _linears(layer)], list(params[1::2])
        Wp, Mp, bp, widths = _chain_arrays(W, M, b)
        ws = torch.empty(_chain_bytes(x.shape[0], x.shape[1], widths, CHAIN_BACKWARD), dtype=torch.uint8, device=x.device)
        u, ildj = density_chain(x, layer, ws)
        ctx.save_for_backward(x, act_w, *params)
        ctx.layer, ctx.ws = layer, ws
        return u, ildj

    @staticmethod
    def backward(ctx, gu, gildj):
        x, act_w, *params = ctx.saved_tensors
        ws, ctx.ws = ctx.ws, None
        gx, gact, grads = _chain_backward(ctx.layer, x, act_w, params, gu, gildj, None, ws, ctx.needs_input_grad[3:])
        return (None, gx, gact if ctx.needs_input_grad[2] else None, *grads)


def _chain_backward(layer, x, act_w, params, gu, gildj, gZ, ws, need):
    lib = load_library()
    B, D = x.shape
    W, b = list(params[0::2]), list(params[1::2])
    M = [require_device_f32(m.mask, 'mask') for m in _linears(layer)]
    Wp, Mp, bp, widths = _chain_arrays(W, M, b)
    holds = ws is not None
    if ws is None:
        ws = torch.empty(_chain_bytes(B, D, widths, CHAIN_BACKWARD), dtype=torch.uint8, device=x.device)
    n = len(W)
    gws = [torch.empty_like(w) if need[2 * i] else None for i, w in enumerate(W)]
    gbs = [torch.empty_like(t) if need[2 * i + 1] else None for i, t in enumerate(b)]
    gWp = (ctypes.c_void_p * n)(*[ptr(g) for g in gws])
    gbp = (ctypes.c_void_p * n)(*[ptr(g) for g in gbs])
    gx = torch.empty_like(x)
    gact = torch.empty(1, dtype=torch.float32, device=x.device) if act_w is not None else None
    gu = require_device_f32(gu, 'grad_u') if gu is not None else None
    gildj = require_device_f32(gildj, 'grad_ildj') if gildj is not None else None
    gZ = require_device_f32(gZ, 'grad_z') if gZ is not None else None
    call(lib.dpk_maf_density_chain_backward, ptr(x), B, D, n - 1, Wp, Mp, bp, widths, _activation(layer), ptr(act_w),
                                             ptr(gu), ptr(gildj), ptr(gZ), ptr(gx), gWp, gbp, ptr(gact), int(holds),
                                             ptr(ws), ws.numel(), stream_ptr(x.device))
    grads = []
    for gw, gb in zip(gws, gbs):
        grads += [gw, gb]
    return gx, (gact.reshape(act_w.shape) if gact is not None else None), grads


def autoregressive_backward(x: torch.Tensor, layer) -> Tuple[torch.Tensor, torch.Tensor]:
    """AutoregressiveLayer.apply_backward (reference: flows/layers/autoregressive.py:72-79)."""
    x = _check_input(x, layer, 'x')
    lins = _linears(layer)
    flat = [t for m in lins for t in (m.weight, m.bias)]
    if _wants_graph(x, layer.scale_act.weight, *flat):
        return MafDensityFn.apply(layer, x, require_device_f32(layer.scale_act.weight, 'scale_act.weight'),
                                  *[require_device_f32(t, 'parameter') for t in flat])
    if fused_route(layer, x.shape[1]):
        return density_fused(x, layer)
    return density_chain(x, layer)


def flow_density(flow, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """MAF.apply_backward without a graph: every eval-mode BatchNormLayer1d is folded (one small kernel) into the
    in_scale / in_shift of the fused kernel of the autoregressive layer behind it, whose log-det is accumulated into
    one [B] vector; layers on other routes apply the pending affine first."""
    from deeprob.flows.utils import BatchNormLayer1d
    from deeprob.hip import ops_flows
    x = require_device_f32(x, 'x')
    B = x.shape[0]
    ildj = torch.zeros(B, dtype=torch.float32, device=x.device)
    affine, consts = None, []
    for layer in flow.layers:
        if isinstance(layer, BatchNormLayer1d):
            affine, _ = ops_flows.bn1d_fold(layer, inverse=False, in_affine=affine, ldj_const=consts)
        elif hasattr(layer, 'network') and affine is not None and fused_route(layer, x.shape[1]):
            x, ildj = density_fused(_check_input(x, layer, 'x'), layer, in_affine=affine, ildj=ildj)
            affine = None
        else:
            if affine is not None:
                x, affine = ops_flows.affine1d(x, affine), None
            x, d = layer.apply_backward(x)
            ildj = ildj + d
    if affine is not None:
        x = ops_flows.affine1d(x, affine)
    for c in consts:
        ildj = ildj + c
    return x, ildj


# ---- the conditioner as a differentiable op (the step loop) -----------------------------------------------------------
class MafConditionerFn(torch.autograd.Function):
    """Z [B, 2D] = network(x) (reference: autoregressive.py:73), with its backward on the chained route."""

    @staticmethod
    def forward(ctx, layer, x, *params):
        lib = load_library()
        B, D = x.shape
        W, b = list(params[0::2]), list(params[1::2])
        M = [require_device_f32(m.mask, 'mask') for m in _linears(layer)]
        Wp, Mp, bp, widths = _chain_arrays(W, M, b)
        ws = torch.empty(_chain_bytes(B, D, widths, CHAIN_BACKWARD), dtype=torch.uint8, device=x.device)
        z = torch.empty(B, 2 * D, dtype=torch.float32, device=x.device)
        call(lib.dpk_maf_conditioner_forward, ptr(x), B, D, len(W) - 1, Wp, Mp, bp, widths, _activation(layer), ptr(z),
                                              ptr(ws), ws.numel(), stream_ptr(x.device))
        ctx.save_for_backward(x, *params)
        ctx.layer, ctx.ws = layer, ws
        return z

    @staticmethod
    def backward(ctx, gz):
        x, *params = ctx.saved_tensors
        ws, ctx.ws = ctx.ws, None
        gx, _, grads = _chain_backward(ctx.layer, x, None, params, None, None, gz, ws, ctx.needs_input_grad[2:])
        return (None, gx, *grads)


def conditioner(x: torch.Tensor, layer) -> torch.Tensor:
    """Z = network(x); an autograd node (its activations kept for the backward) only when a graph is wanted."""
    x = require_device_f32(x, 'x')
    flat = [require_device_f32(t, 'parameter') for m in _linears(layer) for t in (m.weight, m.bias)]
    if _wants_graph(x, *flat):
        return MafConditionerFn.apply(layer, x, *flat)
    lib = load_library()
    B, D = x.shape
    lins, W, M, b = _params(layer)
    Wp, Mp, bp, widths = _chain_arrays(W, M, b)
    ws = layer._ws.get(_chain_bytes(B, D, widths, CHAIN_CONDITIONER), x.device)
    z = torch.empty(B, 2 * D, dtype=torch.float32, device=x.device)
    call(lib.dpk_maf_conditioner_forward, ptr(x), B, D, len(W) - 1, Wp, Mp, bp, widths, _activation(layer), ptr(z),
                                          ptr(ws), ws.numel(), stream_ptr(x.device))
    return z


def step_loop(u: torch.Tensor, layer) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's sampling algorithm (autoregressive.py:81-121): one conditioner evaluation per variable, in the
    order of inv_ordering, on the partially produced x (entries not yet produced are 0).  Differentiable when autograd
    is on (rsample); D conditioner passes per layer -- slow by design."""
    D = layer.in_features
    a = layer.scale_act.weight
    if torch.is_grad_enabled():
        x = list(torch.unbind(torch.zeros_like(u), dim=1))
        ldj = list(torch.unbind(torch.zeros_like(u), dim=1))
        for i in layer.inv_ordering:
            z = conditioner(torch.stack(x, dim=1), layer)
            s = a * torch.tanh(z[:, D + i])
            x[i] = u[:, i] * torch.exp(s) + z[:, i]
            ldj[i] = s
        return torch.stack(x, dim=1), torch.sum(torch.stack(ldj, dim=1), dim=1)
    x = torch.zeros_like(u)
    ldj = torch.zeros_like(u)
    for i in layer.inv_ordering:
        z = conditioner(x, layer)
        s = a * torch.tanh(z[:, D + i])
        x[:, i] = u[:, i] * torch.exp(s) + z[:, i]
        ldj[:, i] = s
    return x, torch.sum(ldj, dim=1)


def sample_envelope(layer) -> bool:
    lins = _linears(layer)
    return len(lins) == 2 and lins[0].weight.shape[0] <= SAMPLE_MAX_UNITS


def deep_sample_envelope(layer) -> bool:
    """2 .. 8 hidden layers of at most 512 units in all, masks autoregressive in the layer's order."""
    lins = _linears(layer)
    if not 3 <= len(lins) <= DEEP_MAX_HIDDEN + 1 or sum(m.weight.shape[0] for m in lins[:-1]) > DEEP_MAX_UNITS:
        return False
    return deep_schedule(layer) is not None


def sample_deep_kernel(u: torch.Tensor, layer) -> Tuple[torch.Tensor, torch.Tensor]:
    """apply_forward without a graph on the one-launch sampling kernel for >= 2 hidden layers."""
    lib = load_library()
    B, D = u.shape
    lins, W, M, b = _params(layer)
    Wp, Mp, bp, widths = _chain_arrays(W, M, b)
    ws = layer._ws_sample.sized(lib.dpk_maf_sample_deep_workspace_bytes, D, len(W) - 1, widths, device=u.device)
    ev_ptr, ev = deep_schedule(layer)
    x = torch.empty_like(u)
    ldj = torch.empty(B, dtype=torch.float32, device=u.device)
    act_w = require_device_f32(layer.scale_act.weight, 'scale_act.weight')
    call(lib.dpk_maf_sample_deep_forward, ptr(u), B, D, len(W) - 1, Wp, Mp, bp, widths, _activation(layer), ptr(act_w),
                                          ptr(_step_order(layer, u.device)), ptr(ev_ptr), ptr(ev), ptr(x), ptr(ldj),
                                          ptr(ws), ws.numel(), stream_ptr(u.device))
    return x, ldj


def sample_kernel(u: torch.Tensor, layer) -> Tuple[torch.Tensor, torch.Tensor]:
    """apply_forward without a graph on the one-launch sampling kernel (depth 1, any mask)."""
    lib = load_library()
    B, D = u.shape
    lins, W, M, b = _params(layer)
    units = W[0].shape[0]
    ws = layer._ws_sample.sized(lib.dpk_maf_sample_workspace_bytes, D, units, device=u.device)
    x = torch.empty_like(u)
    ldj = torch.empty(B, dtype=torch.float32, device=u.device)
    act_w = require_device_f32(layer.scale_act.weight, 'scale_act.weight')
    call(lib.dpk_maf_sample_forward, ptr(u), B, D, ptr(W[0]), ptr(M[0]), ptr(b[0]), ptr(W[1]), ptr(M[1]), ptr(b[1]),
                                     units, _activation(layer), ptr(act_w), ptr(_step_order(layer, u.device)), ptr(x),
                                     ptr(ldj), ptr(ws), ws.numel(), stream_ptr(u.device))
    return x, ldj


def autoregressive_forward(u: torch.Tensor, layer) -> Tuple[torch.Tensor, torch.Tensor]:
    """AutoregressiveLayer.apply_forward (reference: flows/layers/autoregressive.py:81-121)."""
    u = _check_input(u, layer, 'u')
    if torch.is_grad_enabled():
        return step_loop(u, layer)
    if sample_envelope(layer):
        return sample_kernel(u, layer)
    if deep_sample_envelope(layer):
        return sample_deep_kernel(u, layer)
    return step_loop(u, layer)


# ---- MaskedLinear on its own ------------------------------------------------------------------------------------------
class MaskedLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, lin):
        lib = load_library()
        B, fin = x.shape
        fout = W.shape[0]
        ws = torch.empty(call(lib.dpk_masked_linear_workspace_bytes, fin, fout), dtype=torch.uint8, device=x.device)
        y = torch.empty(B, fout, dtype=torch.float32, device=x.device)
        mask = require_device_f32(lin.mask, 'mask')
        call(lib.dpk_masked_linear_forward, ptr(x), B, fin, fout, ptr(W), ptr(mask), ptr(b), ptr(y), ptr(ws), ws.numel(),
                                            stream_ptr(x.device))
        ctx.save_for_backward(x, W, mask)
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = load_library()
        x, W, mask = ctx.saved_tensors
        B, fin = x.shape
        fout = W.shape[0]
        gy = require_device_f32(gy, 'grad_y')
        need = ctx.needs_input_grad
        gx = torch.empty_like(x) if need[0] else None
        gW = torch.empty_like(W) if need[1] else None
        gb = torch.empty(fout, dtype=torch.float32, device=x.device) if (need[2] and ctx.has_b) else None
        ws = torch.empty(lib.dpk_masked_linear_workspace_bytes(fin, fout), dtype=torch.uint8, device=x.device)
        call(lib.dpk_masked_linear_backward, ptr(x), B, fin, fout, ptr(W), ptr(mask), ptr(gy), ptr(gx), ptr(gW), ptr(gb),
                                             ptr(ws), ws.numel(), stream_ptr(x.device))
        return gx, gW, gb, None


def masked_linear(x: torch.Tensor, lin) -> torch.Tensor:
    """MaskedLinear.forward (reference: torch/utils.py:88-96) on any leading shape."""
    x = require_device_f32(x, 'x')
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1]).contiguous()
    W = require_device_f32(lin.weight, 'weight')
    b = require_device_f32(lin.bias, 'bias') if lin.bias is not None else None
    y = MaskedLinearFn.apply(x2, W, b, lin)
    return y.reshape(*lead, W.shape[0])
