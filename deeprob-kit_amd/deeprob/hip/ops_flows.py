"""Flow operators on top of the C ABI: RealNVP-1D coupling, batch norm (folded in eval mode, batch statistics in
training mode), Normal base.

Density direction (`apply_backward`, what `log_prob` / training uses): forward and autograd.  Sampling direction
(`apply_forward`): forward only -- asking autograd for a graph through it raises instead of silently returning a
detached result.
"""
import ctypes
from typing import Optional, Tuple

import torch

from deeprob.hip import (load_library, call, check, ptr, stream_ptr, require_device_f32, HipError, tensors_key,
                         trust_versions, prepare_begin, prepare_commit, prepare_release, prepared, BnFoldArgs as _BnFoldArgs,
                         PairsTablesArgs as _PairsTablesArgs, DPK_FLAG_PARAMS_CACHED, cached_tables_flag)


# ---- one verification pass per flow forward (round 3) -----------------------------------------------------------------
# NormalizingFlow._forward_fused calls flow1d_prepare once: every eval-mode BatchNormLayer1d is folded by ONE launch
# (dpk_bn1d_fold_many, which also leaves the sum of the constant log-determinants) and the packed tables of every
# alternating-mask coupling are fingerprinted / rebuilt by TWO launches (dpk_coupling1d_pairs_tables) -- instead of three
# small launches per layer.  The per-layer operators below recognise the forward's token (hip.prepare_begin) and skip
# their own launches: the couplings through Workspace.tables_flag, a folded batch norm by its ``_fold_token``, the sum of
# the constants by the flow's ``_const_sum_token``.
flow1d_release = prepare_release


def flow1d_prepare(flow, layers, x: torch.Tensor):
    """Fold the batch norms and verify the coupling tables of one density evaluation in three launches (see above).
    Layers outside the batched entries' envelope are left to their own operators.  No-op when the version counters are
    trusted (nothing is launched per call then) or for host tensors (the operators raise)."""
    token = prepare_begin()
    if trust_versions() or not x.is_cuda or x.dim() != 2 or x.dtype != torch.float32 or len(layers) > 32:
        return
    from deeprob.flows.utils import BatchNormLayer1d
    lib = load_library()
    dev = x.device
    # ---- batch norms whose input is not another batch norm's output (the fold chain restarts behind every coupling)
    bn_idx = [i for i, l in enumerate(layers) if isinstance(l, BatchNormLayer1d)]
    simple = [i for i in bn_idx if i == 0 or not isinstance(layers[i - 1], BatchNormLayer1d)]
    entries, folded = [], {}
    for i in simple[:16]:
        bn = layers[i]
        if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                   for t in (bn.weight, bn.bias, bn.running_var, bn.running_mean)):
            continue
        D = bn.in_features
        key = (tensors_key(bn.weight, bn.bias, bn.running_var, bn.running_mean, None, None), False, float(bn.eps))
        hit = getattr(bn, '_fold_cache', None)
        if hit is None or hit[0] != key:
            hit = (key, (torch.empty(D, dtype=torch.float32, device=dev), torch.empty(D, dtype=torch.float32, device=dev)),
                   torch.empty(1, dtype=torch.float32, device=dev), (None, None))
            bn._fold_cache = hit
        (sc, sh), own = hit[1], hit[2]
        entries.append(_BnFoldArgs(ptr(bn.weight), ptr(bn.bias), ptr(bn.running_var), ptr(bn.running_mean), None, None, ptr(sc), ptr(sh), ptr(own), float(bn.eps),
                                   D, 0, 0))
        folded[i] = (bn, hit)
    if entries:
        total = None
        if len(folded) == len(bn_idx):      # every constant comes from this launch: their sum too (sum_constants' tensor)
            consts = [folded[i][1][2] for i in bn_idx]
            ckey = tuple(id(t) for t in consts)
            chit = getattr(flow, '_const_sum_cache', None)
            if chit is None or chit[0] != ckey:
                chit = (ckey, torch.empty(1, dtype=torch.float32, device=dev), list(consts))
                flow._const_sum_cache = chit
            total = chit[1]
        arr = (_BnFoldArgs * len(entries))(*entries)
        call(lib.dpk_bn1d_fold_many, len(entries), ctypes.cast(arr, ctypes.c_void_p), ptr(total), stream_ptr(dev))
        for bn, _ in folded.values():
            bn._fold_token = token
        if total is not None:
            flow._const_sum_token = token
    # ---- couplings inside the column-pair kernel's envelope (the tests of coupling1d / coupling1d_logprob)
    centries, marked = [], []
    for i, layer in enumerate(layers):
        if isinstance(layer, BatchNormLayer1d) or len(centries) == 16:
            continue
        net = getattr(layer, 'network', None)
        if net is None or len(net) != 3:
            continue
        lin1, lin2 = net[0], net[-1]
        units, D = lin1.weight.shape[0], x.shape[1]
        parity = layer._pair_parity()
        if parity is None or units not in (32, 64, 96, 128) or D % 8 != 0 or not lin1.weight.is_cuda:
            continue
        if lin1.weight.dtype != torch.float32 or not all(t.is_contiguous() for t in (lin1.weight, lin1.bias, lin2.weight, lin2.bias)):
            continue
        if i > 0 and isinstance(layers[i - 1], BatchNormLayer1d):
            if (i - 1) not in folded:
                continue            # a chain of batch norms in front: the per-layer route folds and verifies it
            sc, sh = folded[i - 1][1][1]
        else:
            sc, sh = None, None
        pw = layer._ws_pairs
        ws = pw.sized(lib.dpk_coupling1d_pairs_workspace_bytes, D, units, device=dev, or_none=True)
        if ws is None:
            continue
        w1, b1, w2, b2 = lin1.weight, lin1.bias, lin2.weight, lin2.bias
        key = (tensors_key(w1, b1, w2, b2, sc, sh), parity, bool(layer.affine))
        if not _pairs_well_conditioned(pw, key, w1, w2, sc, parity):
            continue                # (the fp32-MFMA kernel takes this layer: no packed tables)
        flags = cached_tables_flag() if pw.holds_tables(key) else 0
        centries.append(_PairsTablesArgs(ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(sc), ptr(sh), ptr(ws), ws.numel(), D, units,
                                         parity, int(layer.affine), flags))
        marked.append((pw, key))
    if centries:
        arr = (_PairsTablesArgs * len(centries))(*centries)
        rc = lib.dpk_coupling1d_pairs_tables(len(centries), ctypes.cast(arr, ctypes.c_void_p), stream_ptr(dev))
        if rc:
            # nothing is known about any of these table sets now: the per-layer operators rebuild (round-3 advice: the keys
            # used to be recorded BEFORE the launch, and a failure left them claiming tables that were never built)
            for pw, _ in marked:
                pw.forget_prepared()
            check(rc, lib.dpk_coupling1d_pairs_tables)
        for pw, key in marked:
            pw.tables_built(key, token)
    prepare_commit(token)


# ---- accuracy guard of the split-f16 coupling kernels (round 4) --------------------------------------------------------
# The column-pair kernels multiply on two-way f16 splits: >= 22 significant bits per product against fp32's 24.  For the
# flows one meets (default initialisation, trained weights of that order) that is invisible: the conditioner's worst-case
# gain  A = max_j sum_i |W1[j,i] a_i| * max_d sum_j |W2[d,j]|  (a = the folded BatchNorm scale on the masked inputs) is
# 50-80, and 2^-22 A |x| stays below 1e-6 of |log p|.  A badly conditioned layer (conditioner weights 10x, BatchNorm
# variances of 1e-4: A = 2e3 .. 4e4) amplifies every product's rounding by A, the reference's fp32 arithmetic included --
# there 22 bits measured 6x the reference's own distance from fp64 (tests/test_flows_gpu.py::
# the stress test of the column-pair kernels).  Such layers keep the fp32-MFMA kernel (dpk_coupling1d_forward: exact fp32
# products, csrc/coupling.hip).  The verdict is taken where the packed tables are keyed -- once per (parameter versions,
# folded affine), one small reduction and one host read -- so a frozen model pays nothing per call.
PAIRS_GAIN_LIMIT = 1024.0


def _pairs_well_conditioned(pw, key, w1: torch.Tensor, w2: torch.Tensor, sc: Optional[torch.Tensor], parity: int) -> bool:
    hit = getattr(pw, '_cond', None)
    if hit is not None and hit[0] == key:
        return hit[1]
    if torch.cuda.is_current_stream_capturing():
        return False        # (no host read inside a capture: an unjudged layer takes the exact kernel)
    with torch.no_grad():
        cols = w1[:, parity::2].abs()          # the conditioner sees the masked (pass-through) columns only
        if sc is not None:
            cols = cols * sc.reshape(-1)[parity::2].abs()
        gain = float((cols.sum(dim=1).max() * w2.abs().sum(dim=1).max()).item())
    ok = gain == gain and gain <= PAIRS_GAIN_LIMIT
    pw._cond = (key, ok, gain)
    return ok


def _no_graph(*tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise HipError(
            "the sampling direction (apply_forward) of the HIP flow kernels has no backward: wrap the call in "
            "torch.no_grad(), or freeze the parameters"
        )


def coupling1d(x: torch.Tensor, layer, inverse: bool, in_affine: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
               ldj: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """CouplingLayer1d.apply_backward / apply_forward (reference: deeprob/flows/layers/coupling.py:72-104)."""
    lib = load_library()
    x = require_device_f32(x, 'x')
    lin1, lin2 = layer.network[0], layer.network[-1]
    if inverse:
        _no_graph(x, lin1.weight, lin2.weight)
    if len(layer.network) != 3 or lin1.weight.shape[0] % 32 != 0 or lin1.weight.shape[0] > 512:
        # deeper conditioners / odd widths: layer-by-layer route on the generic GEMM kernel
        if in_affine is not None:
            x = affine1d(x, in_affine)
        out, d = _coupling1d_mlp(x, layer, inverse)
        if ldj is not None:
            ldj += d
            d = ldj
        return out, d
    B, D = x.shape
    units = lin1.weight.shape[0]
    n_masked, n_trans = layer._mask_counts()
    parity = layer._pair_parity()
    if parity is not None and units in (32, 64, 96, 128) and D % 8 == 0 and x.data_ptr() % 16 == 0:
        # the reference's alternating masks: split-f16 MFMA kernel, packed tables kept while the weights (and the
        # folded input affine) are unchanged.  (Rows that are not 16-byte aligned -- a view at an odd storage offset --
        # keep the generic kernel below; the test comes first so that nothing of this branch leaks into that route.)
        pw = layer._ws_pairs
        ws = pw.sized(lib.dpk_coupling1d_pairs_workspace_bytes, D, units, device=x.device)
        out = torch.empty_like(x)
        if out.data_ptr() % 16 == 0:
            ldj_p = ldj if ldj is not None else torch.empty(B, dtype=torch.float32, device=x.device)
            sc, sh = in_affine if in_affine is not None else (None, None)
            act = layer.scale_act.weight if layer.affine else None
            w1, b1 = require_device_f32(lin1.weight, 'W1'), require_device_f32(lin1.bias, 'b1')
            w2, b2 = require_device_f32(lin2.weight, 'W2'), require_device_f32(lin2.bias, 'b2')
            key = (tensors_key(w1, b1, w2, b2, sc, sh), parity, bool(layer.affine))
            # (accuracy guard: a badly conditioned layer keeps the fp32-MFMA kernel below)
            if _pairs_well_conditioned(pw, key, w1, w2, sc, parity):
                flags = pw.tables_flag(key)
                rc = lib.dpk_coupling1d_pairs_forward(
                    ptr(x), B, D, parity, ptr(w1), ptr(b1), ptr(w2), ptr(b2), units, ptr(act), ptr(sc), ptr(sh),
                    int(layer.affine), int(inverse), ptr(out), ptr(ldj_p), int(ldj is not None), ptr(ws), ws.numel(),
                    flags, stream_ptr(x.device))
                if rc:
                    pw.forget_tables()        # (a failed call built nothing: the next one does not trust the tables)
                    check(rc, lib.dpk_coupling1d_pairs_forward)
                return out, ldj_p
    ws = layer._ws.sized(lib.dpk_coupling1d_workspace_bytes, D, units, n_masked, n_trans, device=x.device)
    out = torch.empty_like(x)
    accumulate = ldj is not None
    if ldj is None:
        ldj = torch.empty(B, dtype=torch.float32, device=x.device)
    sc, sh = in_affine if in_affine is not None else (None, None)
    act = layer.scale_act.weight if layer.affine else None
    call(lib.dpk_coupling1d_forward, 
        ptr(x), B, D, ptr(layer.mask), ptr(layer.inv_mask), n_masked, n_trans,
        ptr(require_device_f32(lin1.weight, 'W1')), ptr(require_device_f32(lin1.bias, 'b1')),
        ptr(require_device_f32(lin2.weight, 'W2')), ptr(require_device_f32(lin2.bias, 'b2')), units,
        ptr(act), ptr(sc), ptr(sh), int(layer.affine), int(inverse), ptr(out), ptr(ldj), int(accumulate),
        ptr(ws), ws.numel(), stream_ptr(x.device))
    return out, ldj


def coupling1d_logprob(x: torch.Tensor, layer, in_affine, ildj: Optional[torch.Tensor], out_affine,
                       base_loc: torch.Tensor, base_scale: torch.Tensor,
                       ildj_const: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """The last CouplingLayer1d of a flow (density direction) + the folded affine behind it + the diagonal Normal base in
    ONE kernel (reference: coupling.py:72-87 followed by flows/utils.py:118-139 and flows/models/base.py:139-143):
    ``ll = sum_d log N(out_affine(u)_d; loc_d, scale_d) + ildj - sum s + ildj_const``.  None when the layer is outside
    the column-pair MFMA kernel's envelope (the caller then chains coupling1d and normal_base_logprob)."""
    lib = load_library()
    x = require_device_f32(x, 'x')
    lin1, lin2 = layer.network[0], layer.network[-1]
    if len(layer.network) != 3 or x.dim() != 2:
        return None
    B, D = x.shape
    units = lin1.weight.shape[0]
    parity = layer._pair_parity()
    if parity is None or units not in (32, 64, 96, 128) or D % 8 != 0 or x.data_ptr() % 16 != 0 or base_loc.numel() != D:
        return None
    pw = layer._ws_pairs
    ws = pw.sized(lib.dpk_coupling1d_pairs_workspace_bytes, D, units, device=x.device, or_none=True)
    if ws is None:
        return None
    sc, sh = in_affine if in_affine is not None else (None, None)
    osc, osh = out_affine if out_affine is not None else (None, None)
    act = layer.scale_act.weight if layer.affine else None
    w1, b1 = require_device_f32(lin1.weight, 'W1'), require_device_f32(lin1.bias, 'b1')
    w2, b2 = require_device_f32(lin2.weight, 'W2'), require_device_f32(lin2.bias, 'b2')
    key = (tensors_key(w1, b1, w2, b2, sc, sh), parity, bool(layer.affine))
    if not _pairs_well_conditioned(pw, key, w1, w2, sc, parity):
        return None             # (accuracy guard: the caller chains the fp32-MFMA coupling and the base density)
    flags = pw.tables_flag(key)
    ll = torch.empty(B, dtype=torch.float32, device=x.device)
    rc = lib.dpk_coupling1d_pairs_logprob(
        ptr(x), B, D, parity, ptr(w1), ptr(b1), ptr(w2), ptr(b2), units, ptr(act), ptr(sc), ptr(sh), int(layer.affine),
        ptr(osc), ptr(osh), ptr(require_device_f32(base_loc.reshape(-1), 'loc')),
        ptr(require_device_f32(base_scale.reshape(-1), 'scale')), ptr(ildj), ptr(ildj_const), ptr(ll), ptr(ws),
        ws.numel(), flags, stream_ptr(x.device))
    return pw.outcome(rc, lib.dpk_coupling1d_pairs_logprob, ll)


def _mlp_args(layer):
    """(n_hidden, W pointer array, b pointer array, widths array, tensors kept alive) of the conditioner."""
    import ctypes
    lins = [m for m in layer.network if isinstance(m, torch.nn.Linear)]
    ws = [require_device_f32(m.weight, 'weight') for m in lins]
    bs = [require_device_f32(m.bias, 'bias') for m in lins]
    n = len(lins)
    Wp = (ctypes.c_void_p * n)(*[w.data_ptr() for w in ws])
    bp = (ctypes.c_void_p * n)(*[b.data_ptr() for b in bs])
    widths = (ctypes.c_int32 * n)(*[w.shape[0] for w in ws])
    return n - 1, Wp, bp, widths, (ws, bs)


# a training forward keeps the conditioner activations for its backward while they fit this many bytes per layer call
# (beyond it the backward evaluates the conditioner again)
KEEP_ACTIVATIONS_BYTES = 1 << 30


def _mlp_backward_bytes(B: int, n_hidden: int, widths) -> int:
    return int(call(load_library().dpk_coupling1d_mlp_workspace_bytes, B, n_hidden, widths, 1))


def _coupling1d_mlp(x: torch.Tensor, layer, inverse: bool, keep: bool = False):
    """CouplingLayer1d with any conditioner depth (reference: coupling.py:45-56, :72-104).  keep: the workspace
    is a fresh buffer laid out for the backward, returned as third value (it holds the conditioner activations)."""
    lib = load_library()
    layer._mask_counts()
    B, D = x.shape
    n_hidden, Wp, bp, widths, alive = _mlp_args(layer)
    if keep:
        ws = torch.empty(_mlp_backward_bytes(B, n_hidden, widths), dtype=torch.uint8, device=x.device)
    else:
        ws = layer._ws.sized(lib.dpk_coupling1d_mlp_workspace_bytes, B, n_hidden, widths, 0, device=x.device)
    out = torch.empty_like(x)
    ldj = torch.empty(B, dtype=torch.float32, device=x.device)
    act = layer.scale_act.weight if layer.affine else None
    call(lib.dpk_coupling1d_mlp_forward, ptr(x), B, D, ptr(layer.mask), ptr(layer.inv_mask), n_hidden, Wp, bp, widths,
                                         ptr(act), int(layer.affine), int(inverse), ptr(out), ptr(ldj), ptr(ws),
                                         ws.numel(), stream_ptr(x.device))
    del alive
    return (out, ldj, ws) if keep else (out, ldj)


def bn1d_fold(bn, inverse: bool, in_affine=None, ldj_const: Optional[torch.Tensor] = None):
    """Eval-mode BatchNormLayer1d as a per-variable affine (reference: deeprob/flows/utils.py:118-153), composed with
    an incoming affine.  Returns ((scale, shift), ldj_const[1]); a given ``ldj_const`` is accumulated into.

    The fold depends only on the layer's parameters / running statistics and on the incoming affine: its result is
    kept (the SAME tensors, so that the coupling behind it recognises its packed tables) while their addresses and
    version counters are unchanged."""
    lib = load_library()
    D = bn.in_features
    dev = bn.weight.device
    s_in, h_in = in_affine if in_affine is not None else (None, None)
    key = (tensors_key(bn.weight, bn.bias, bn.running_var, bn.running_mean, s_in, h_in), bool(inverse), float(bn.eps))
    hit = getattr(bn, '_fold_cache', None)
    fresh = hit is None or hit[0] != key
    if fresh:
        sc = torch.empty(D, dtype=torch.float32, device=dev)
        sh = torch.empty(D, dtype=torch.float32, device=dev)
        own = torch.empty(1, dtype=torch.float32, device=dev)     # this layer's constant log-det
        # (s_in / h_in are kept alive with the entry: their addresses are part of the key)
        hit = (key, (sc, sh), own, (s_in, h_in))
        bn._fold_cache = hit
    if (fresh or not trust_versions()) and not (not fresh and not inverse and in_affine is None
                                                and prepared(getattr(bn, '_fold_token', None))):
        # The fold is one D-element kernel: it runs on every call (into the SAME tensors), so that a write through
        # `.data` of a statistic or parameter -- which moves no version counter -- is folded in; the coupling behind it
        # fingerprints these tensors on the device.  With hip.trust_version_counters(True) it runs on a key change only.
        (sc, sh), own = hit[1], hit[2]
        call(lib.dpk_bn1d_fold, ptr(require_device_f32(bn.weight, 'weight')), ptr(require_device_f32(bn.bias, 'bias')),
                                ptr(require_device_f32(bn.running_var, 'running_var')),
                                ptr(require_device_f32(bn.running_mean, 'running_mean')), float(bn.eps), D,
                                int(inverse), ptr(s_in), ptr(h_in), ptr(sc), ptr(sh), ptr(own), 0, stream_ptr(dev))
    if isinstance(ldj_const, list):      # the caller sums the layers' constants itself (sum_constants below)
        ldj_const.append(hit[2])
        return hit[1], ldj_const
    if ldj_const is None:
        return hit[1], hit[2].clone()
    ldj_const += hit[2]
    return hit[1], ldj_const


def sum_constants(owner, consts) -> Optional[torch.Tensor]:
    """Total of the eval-mode BatchNorm layers' constant log-determinants (one-element tensors kept by bn1d_fold): summed
    once and reused while every layer returns the very tensors it returned before -- four one-element additions per
    call otherwise."""
    if not consts:
        return None
    key = tuple(id(t) for t in consts)
    hit = getattr(owner, '_const_sum_cache', None)
    if hit is None or hit[0] != key:
        hit = (key, torch.stack([t.reshape(()) for t in consts]).sum().reshape(1), list(consts))   # (keeps them alive)
        owner._const_sum_cache = hit
    elif not trust_versions() and not prepared(getattr(owner, '_const_sum_token', None)):
        # (bn1d_fold rewrites the constants in place on every call: the total follows them, into the same tensor)
        torch.sum(torch.stack([t.reshape(()) for t in consts]), dim=0, keepdim=True, out=hit[1])
    return hit[1]


def affine1d(x: torch.Tensor, affine) -> torch.Tensor:
    lib = load_library()
    x = require_device_f32(x, 'x')
    out = torch.empty_like(x)
    B, D = x.shape
    call(lib.dpk_affine1d_forward, ptr(x), ptr(affine[0]), ptr(affine[1]), B, D, ptr(out), stream_ptr(x.device))
    return out


def normal_base_logprob(u: torch.Tensor, affine, loc, scale, ildj, ildj_const) -> torch.Tensor:
    """sum_d log N(affine(u); loc, scale) + ildj + ildj_const (reference: flows/models/base.py:139-143)."""
    lib = load_library()
    u = require_device_f32(u, 'u')
    B, D = u.shape
    out = torch.empty(B, dtype=torch.float32, device=u.device)
    sc, sh = affine if affine is not None else (None, None)
    call(lib.dpk_normal_base_logprob, ptr(u), ptr(sc), ptr(sh), ptr(require_device_f32(loc, 'loc')),
                                      ptr(require_device_f32(scale, 'scale')), ptr(ildj), ptr(ildj_const), B, D,
                                      ptr(out), stream_ptr(u.device))
    return out


def _wants_graph(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class CouplingFn(torch.autograd.Function):
    """CouplingLayer1d.apply_backward with autograd (reference: flows/layers/coupling.py:72-87; backward
    formulas SURVEY 8a).  The conditioner activations are recomputed in the backward."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, act, layer):
        with torch.no_grad():
            u, ildj = coupling1d(x, layer, inverse=False)
        ctx.save_for_backward(x, W1, b1, W2, b2, act)
        ctx.layer = layer
        return u, ildj

    @staticmethod
    def backward(ctx, gu, gildj):
        lib = load_library()
        x, W1, b1, W2, b2, act = ctx.saved_tensors
        layer = ctx.layer
        B, D = x.shape
        units = W1.shape[0]
        gu = require_device_f32(gu, 'grad_u')
        gildj = require_device_f32(gildj, 'grad_ildj')
        need = ctx.needs_input_grad
        gx = torch.empty_like(x)
        gW1 = torch.empty_like(W1) if need[1] else None
        gb1 = torch.empty_like(b1) if need[2] else None
        gW2 = torch.empty_like(W2) if need[3] else None
        gb2 = torch.empty_like(b2) if need[4] else None
        gact = torch.empty_like(act) if (act is not None and need[5]) else None
        ws = layer._ws_bwd.sized(lib.dpk_coupling1d_backward_workspace_bytes, B, D, units, int(layer.affine), device=x.device)
        call(lib.dpk_coupling1d_backward, 
            ptr(x), B, D, ptr(layer.mask), ptr(layer.inv_mask), ptr(W1), ptr(b1), ptr(W2), ptr(b2), units, ptr(act),
            int(layer.affine), ptr(gu), ptr(gildj), ptr(gx), ptr(gW1), ptr(gb1), ptr(gW2), ptr(gb2), ptr(gact),
            ptr(ws), ws.numel(), stream_ptr(x.device))
        return gx, gW1, gb1, gW2, gb2, gact, None


class CouplingMlpFn(torch.autograd.Function):
    """CouplingLayer1d.apply_backward with autograd for any conditioner depth: inputs are x, the ScaledTanh weight
    (or None) and then weight, bias of every Linear in order."""

    @staticmethod
    def forward(ctx, layer, inverse, x, act, *params):
        widths = [w.shape[0] for w in params[0::2]]
        import ctypes
        need = _mlp_backward_bytes(x.shape[0], len(widths) - 1, (ctypes.c_int32 * len(widths))(*widths))
        if need <= KEEP_ACTIVATIONS_BYTES:
            u, ildj, ctx.kept = _coupling1d_mlp(x, layer, inverse=inverse, keep=True)
        else:
            (u, ildj), ctx.kept = _coupling1d_mlp(x, layer, inverse=inverse), None
        ctx.save_for_backward(x, act, *params)
        ctx.layer, ctx.inverse = layer, bool(inverse)
        return u, ildj

    @staticmethod
    def backward(ctx, gu, gildj):
        import ctypes
        lib = load_library()
        x, act, *params = ctx.saved_tensors
        layer = ctx.layer
        B, D = x.shape
        gu = require_device_f32(gu, 'grad_u')
        gildj = require_device_f32(gildj, 'grad_ildj')
        ws_t, bs_t = params[0::2], params[1::2]
        n = len(ws_t)
        need = ctx.needs_input_grad
        gws = [torch.empty_like(w) if need[4 + 2 * i] else None for i, w in enumerate(ws_t)]
        gbs = [torch.empty_like(b) if need[5 + 2 * i] else None for i, b in enumerate(bs_t)]
        Wp = (ctypes.c_void_p * n)(*[w.data_ptr() for w in ws_t])
        bp = (ctypes.c_void_p * n)(*[b.data_ptr() for b in bs_t])
        gWp = (ctypes.c_void_p * n)(*[g.data_ptr() if g is not None else None for g in gws])
        gbp = (ctypes.c_void_p * n)(*[g.data_ptr() if g is not None else None for g in gbs])
        widths = (ctypes.c_int32 * n)(*[w.shape[0] for w in ws_t])
        gx = torch.empty_like(x)
        gact = torch.empty_like(act) if (act is not None and need[3]) else None
        kept = ctx.kept
        ctx.kept = None   # a second backward through the same node evaluates the conditioner again
        ws = kept if kept is not None else layer._ws_bwd.get(_mlp_backward_bytes(B, n - 1, widths), x.device)
        fn = lib.dpk_coupling1d_mlp_backward_inverse if ctx.inverse else lib.dpk_coupling1d_mlp_backward
        call(fn, ptr(x), B, D, ptr(layer.mask), ptr(layer.inv_mask), n - 1, Wp, bp, widths, ptr(act),
             int(layer.affine), ptr(gu), ptr(gildj), ptr(gx), gWp, gbp, ptr(gact), int(kept is not None), ptr(ws),
             ws.numel(), stream_ptr(x.device))
        grads = []
        for gw, gb in zip(gws, gbs):
            grads += [gw, gb]
        return (None, None, gx, gact, *grads)


def coupling1d_autograd(x: torch.Tensor, layer, inverse: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """A coupling layer in either direction (density: apply_backward; sampling: apply_forward, what rsample
    differentiates), recording an autograd node when a graph is needed."""
    lin1, lin2 = layer.network[0], layer.network[-1]
    act = layer.scale_act.weight if layer.affine else None
    lins = [m for m in layer.network if isinstance(m, torch.nn.Linear)]
    if not _wants_graph(x, act, *[t for m in lins for t in (m.weight, m.bias)]):
        return coupling1d(x, layer, inverse=inverse)
    layer._mask_counts()   # binary-mask check
    x = require_device_f32(x, 'x')
    import ctypes
    widths = (ctypes.c_int32 * len(lins))(*[m.weight.shape[0] for m in lins])
    if inverse or len(lins) != 2 or \
            _mlp_backward_bytes(x.shape[0], len(lins) - 1, widths) <= KEEP_ACTIVATIONS_BYTES:
        # GEMM-chained conditioner whose activations stay resident for the backward (always for the sampling direction)
        flat = [require_device_f32(t, 'parameter') for m in lins for t in (m.weight, m.bias)]
        return CouplingMlpFn.apply(layer, inverse, x, act, *flat)
    # too large to keep: fused forward, conditioner evaluated again in the backward
    return CouplingFn.apply(x, require_device_f32(lin1.weight, 'W1'),
                            require_device_f32(lin1.bias, 'b1'), require_device_f32(lin2.weight, 'W2'),
                            require_device_f32(lin2.bias, 'b2'), act, layer)


class BatchNormFn(torch.autograd.Function):
    """BatchNormLayer1d.apply_backward (reference: flows/utils.py:118-139): batch statistics + running-statistics
    update when the layer is training, running statistics otherwise; autograd through either."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn):
        lib = load_library()
        x = require_device_f32(x, 'x')
        B, D = x.shape
        dev = x.device
        train = bool(bn.training)
        group = getattr(bn, 'sync_group', None) if train else None
        if group is not None and torch.distributed.is_initialized() and torch.distributed.get_world_size(group) > 1:
            # batch-sharded training: statistics of the whole batch (deeprob.parallel.synchronize_batchnorm)
            from deeprob import parallel
            world = torch.distributed.get_world_size(group)
            mom = torch.empty(2 * D + 1, dtype=torch.float32, device=dev)
            call(lib.dpk_bn1d_local_moments, ptr(x) if B else None, B, D, ptr(mom), stream_ptr(dev))
            table = parallel.bn_gather_moments(mom, group)
            n_total = int(round(float(table[:, 0].sum().item())))
            u = torch.empty_like(x)
            ldj = torch.empty(1, dtype=torch.float32, device=dev)
            mean = torch.empty(D, dtype=torch.float32, device=dev)
            var = torch.empty(D, dtype=torch.float32, device=dev)
            ws = bn._ws.get(8 * D + 256, dev)
            call(lib.dpk_bn1d_sync_forward, ptr(x) if B else None, B, D, ptr(require_device_f32(weight, 'weight')),
                                            ptr(require_device_f32(bias, 'bias')), ptr(table), world,
                                            ptr(bn.running_var), ptr(bn.running_mean), float(bn.momentum),
                                            float(bn.eps), ptr(u) if B else None, ptr(ldj), ptr(mean), ptr(var), ptr(ws),
                                            ws.numel(), stream_ptr(dev))
            ctx.save_for_backward(x, weight, mean, var)
            ctx.bn, ctx.train, ctx.sync = bn, True, (group, n_total)
            return u, ldj.repeat(B)
        ctx.sync = None
        if train:
            u = torch.empty_like(x)
            ldj = torch.empty(1, dtype=torch.float32, device=dev)
            mean = torch.empty(D, dtype=torch.float32, device=dev)
            var = torch.empty(D, dtype=torch.float32, device=dev)
            ws = bn._ws.get(8 * D + 256, dev)
            call(lib.dpk_bn1d_train_forward, ptr(x), B, D, ptr(require_device_f32(weight, 'weight')),
                                             ptr(require_device_f32(bias, 'bias')), ptr(bn.running_var),
                                             ptr(bn.running_mean), float(bn.momentum), float(bn.eps), ptr(u), ptr(ldj),
                                             ptr(mean), ptr(var), ptr(ws), ws.numel(), stream_ptr(dev))
        else:
            affine, ldj = bn1d_fold(bn, inverse=False)
            u = affine1d(x, affine)
            mean, var = bn.running_mean.detach().reshape(-1).clone(), bn.running_var.detach().reshape(-1).clone()
        ctx.save_for_backward(x, weight, mean, var)
        ctx.bn, ctx.train = bn, train
        return u, ldj.repeat(B)

    @staticmethod
    def backward(ctx, gu, gildj):
        lib = load_library()
        x, weight, mean, var = ctx.saved_tensors
        bn = ctx.bn
        B, D = x.shape
        gu = require_device_f32(gu, 'grad_u')
        gildj = require_device_f32(gildj, 'grad_ildj')
        gx = torch.empty_like(x)
        gw = torch.empty_like(weight) if ctx.needs_input_grad[1] else None
        gb = torch.empty_like(weight) if ctx.needs_input_grad[2] else None
        if ctx.sync is not None:
            from deeprob import parallel
            group, n_total = ctx.sync
            sums = torch.empty(2 * D + 1, dtype=torch.float32, device=x.device)
            call(lib.dpk_bn1d_backward_sums, ptr(x) if B else None, ptr(gu) if B else None, ptr(gildj) if B else None,
                                             B, D, ptr(mean), ptr(var), float(bn.eps), ptr(sums),
                                             stream_ptr(x.device))
            sums_x = parallel.bn_reduce_sums(sums, B, n_total, group)
            call(lib.dpk_bn1d_sync_backward, ptr(x) if B else None, ptr(gu) if B else None, B, n_total, D, ptr(weight),
                                             ptr(mean), ptr(var), float(bn.eps), ptr(sums_x), ptr(sums),
                                             ptr(gx) if B else None, ptr(gw), ptr(gb), stream_ptr(x.device))
            return gx, gw, gb, None
        ws = bn._ws.get(4 * (2 * D + 64) + 256, x.device)
        call(lib.dpk_bn1d_backward, ptr(x), ptr(gu), ptr(gildj), B, D, ptr(weight), ptr(mean), ptr(var),
                                    float(bn.eps), int(ctx.train), ptr(gx), ptr(gw), ptr(gb), ptr(ws), ws.numel(),
                                    stream_ptr(x.device))
        return gx, gw, gb, None


class BatchNormInverseFn(torch.autograd.Function):
    """BatchNormLayer1d.apply_forward with autograd (reference: flows/utils.py:141-153): the inverse transformation
    with the running statistics, x = (u - bias) exp(-weight) sqrt(var + eps) + mean."""

    @staticmethod
    def forward(ctx, u, weight, bias, bn):
        u = require_device_f32(u, 'u')
        with torch.no_grad():
            affine, ldj = bn1d_fold(bn, inverse=True)
            x = affine1d(u, affine)
        ctx.save_for_backward(u, weight, bias)
        ctx.bn = bn
        return x, ldj.expand(u.shape[0]).clone()

    @staticmethod
    def backward(ctx, gx, gldj):
        lib = load_library()
        u, weight, bias = ctx.saved_tensors
        bn = ctx.bn
        B, D = u.shape
        gx = require_device_f32(gx, 'grad_x')
        gldj = require_device_f32(gldj, 'grad_ldj')
        gu = torch.empty_like(u)
        gw = torch.empty_like(weight) if ctx.needs_input_grad[1] else None
        gb = torch.empty_like(bias) if ctx.needs_input_grad[2] else None
        ws = bn._ws.get(4 * (5 * D + 64) + 256, u.device)
        call(lib.dpk_bn1d_inverse_backward, ptr(u), ptr(gx), ptr(gldj), B, D, ptr(weight), ptr(bias),
                                            ptr(bn.running_var), float(bn.eps), ptr(gu), ptr(gw), ptr(gb), ptr(ws),
                                            ws.numel(), stream_ptr(u.device))
        return gu, gw, gb, None


class NormalBaseFn(torch.autograd.Function):
    """sum_d log N(u_d; loc_d, scale_d) for the default (frozen) Normal base (reference: flows/models/base.py:139-140)."""

    @staticmethod
    def forward(ctx, u, loc, scale):
        out = normal_base_logprob(u, None, loc, scale, None, None)
        ctx.save_for_backward(u, loc, scale)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = load_library()
        u, loc, scale = ctx.saved_tensors
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise HipError("the Normal base of the HIP flow path is frozen (in_base_loc / in_base_scale do not "
                           "require grad in the reference either)")
        g = require_device_f32(g, 'grad')
        B, D = u.shape
        gu = torch.empty_like(u)
        call(lib.dpk_normal_base_backward, ptr(u), ptr(loc), ptr(scale), ptr(g), B, D, ptr(gu), stream_ptr(u.device))
        return gu, None, None
