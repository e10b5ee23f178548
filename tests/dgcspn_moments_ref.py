"""Restatement of the DGC-SPN posterior-moments pass (dpm_dgcspn_moments, DgcSpn.posterior_moments) in plain numpy on the
host.

The definition is the one at the top of csrc/dgc/dgcspn_moments.hip, statement for statement:
  - product values are never the model's maps: a product is the sum of its four taps in row-major tap order,
    ((v0 + v1) + v2) + v3, in the precision of the activations the caller hands in (numpy float32 arithmetic on the DEVICE's
    fp32 activations, float64 on the oracle's); a tap outside the input map is 0 and receives nothing; tap coordinates and
    the channel decode are those of tests/dgcspn_topdown_ref.py;
  - root: s(i) = prod_value(i) + logw_root[cls, i], m = max s, e = exp(s - m), G(i) = e(i) / sum e; without labels and with
    all_classes, s ranges over all classes x N entries at once and G(i) is the sum over the classes; m = -inf or NaN: the
    image's NaN entries are NaN in mean and var, its leaf_flow is NaN;
  - product level j, top to bottom: F_j[c_t, ih, iw] += G_j[oc, oh, ow] for every tap inside the map;
  - sum layer t = j >= 1: for every (h, w) and output o with F_t[o, h, w] > 0, s(c) = prod_value_below(c, h, w) +
    logw[o, c, h, w], r = softmax_c s, G_{t-1}[c, h, w] = sum_o F_t[o, h, w] r(o, c);
  - leaves: w = sum_k F_0; a NaN entry with w > 0 gets mean = sum_k F_0 loc_k / w and var = sum_k F_0 (scale_k^2 +
    (loc_k - mean)^2) / w, formed from the distances to the first component's loc; w = 0: the pixel is in nobody's scope and
    stays NaN; an observed entry keeps its value, with variance 0;
  - the maxima, the exponentials and every sum are float64 here, where the kernel has fp32.

A helper module (no tests in it)."""
import numpy as np
import torch

from tests import dgcspn_topdown_ref as ref


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def product_map(row, a):
    """[R, Cout, Hout, Wout] in the dtype of ``a``: every product of the level over the maps a [R, Cin, Hin, Win]."""
    cin, hin, win, cout, hout, wout = row[:6]
    stride = row[10]
    oc = np.arange(cout)
    oh, ow = np.arange(hout) * stride, np.arange(wout) * stride
    acc = None
    for t, dh, dw in ref._taps(row):
        ih, iw = oh + dh, ow + dw
        inside = ((ih >= 0) & (ih < hin))[:, None] & ((iw >= 0) & (iw < win))[None, :]
        v = a[:, ref._digit(row, oc, t)][:, :, np.clip(ih, 0, hin - 1)][:, :, :, np.clip(iw, 0, win - 1)]
        v = np.where(inside[None, None], v, a.dtype.type(0.0)).astype(a.dtype)
        acc = v if acc is None else (acc + v).astype(a.dtype)
    return acc


def scatter(row, g):
    """F_j [R, Cin, Hin, Win] float64 from G_j [R, Cout, Hout, Wout]: every product's flow to each of its taps inside."""
    cin, hin, win, cout, hout, wout = row[:6]
    stride, depthwise = row[10], row[12]
    f = np.zeros((g.shape[0], cin, hin, win))
    oh, ow = np.meshgrid(np.arange(hout), np.arange(wout), indexing='ij')
    for t, dh, dw in ref._taps(row):
        ih, iw = oh * stride + dh, ow * stride + dw
        ok = (ih >= 0) & (ih < hin) & (iw >= 0) & (iw < win)
        if depthwise:
            gc = g
        else:   # the output channels whose digit t is c, summed: oc = (hi Cin + c) Cin^(3 - t) + lo
            gc = g.reshape(g.shape[0], cin ** t, cin, cin ** (3 - t), hout, wout).sum(axis=(1, 3))
        # (one tap sends distinct outputs to distinct inputs: the indexed += meets every target once)
        f[:, :, ih[ok], iw[ok]] += gc[:, :, oh[ok], ow[ok]]
    return f


def posterior_moments(geom, acts, logws, loc, scale, x, y=None, all_classes=False):
    """geom: ref.geometry(...); acts: [leaf output [B, K, H, W], sum layer 1 output, ...], all float32 or all float64; logws:
    log-softmax weights of the sum layers 1 .. L-1, then of the root; loc, scale [K, C, H, W]; x [B, C, H, W], NaN = missing;
    y [B] integer labels or None (class 0, or with all_classes the mixture of the classes).  Host tensors / arrays.
    Returns float64 arrays (mean [B, C, H, W], var [B, C, H, W], leaf_flow [B, K, H, W])."""
    acts = [np.ascontiguousarray(_np(a)) for a in acts]
    dt = acts[0].dtype
    assert dt in (np.float32, np.float64) and all(a.dtype == dt for a in acts)
    logws = [np.ascontiguousarray(_np(w)).astype(dt) for w in logws]
    loc, scale, x = _np(loc).astype(np.float64), _np(scale).astype(np.float64), _np(x).astype(np.float64)
    L, B = len(geom), x.shape[0]
    assert len(acts) == L and len(logws) == L
    # ---- root
    row = geom[L - 1]
    p = product_map(row, acts[L - 1]).reshape(B, 1, -1)
    lw = logws[L - 1]
    if y is not None:
        lw = lw[_np(y).astype(np.int64)][:, None]
    elif all_classes:
        lw = lw[None]
    else:
        lw = lw[None, :1]
    s = (p + lw).astype(dt).astype(np.float64)                       # [B, classes taken, N]
    with np.errstate(invalid='ignore', over='ignore'):
        m = s.reshape(B, -1).max(axis=1)                             # (np.max propagates NaN)
        bad = ~(m > -np.inf)
        e = np.exp(s - np.where(bad, 0.0, m)[:, None, None])
        g = (e / e.sum(axis=(1, 2), keepdims=True)).sum(axis=1).reshape((B,) + tuple(row[3:6]))
        g[bad] = 0.0
        # ---- levels, top to bottom
        for j in range(L - 1, -1, -1):
            f = scatter(geom[j], g)
            if j == 0:
                break
            below = geom[j - 1]
            p = product_map(below, acts[j - 1])                      # [B, count, h, w]
            s = (p[:, None] + logws[j - 1][None]).astype(dt).astype(np.float64)   # [B, S, count, h, w]
            ms = s.max(axis=2, keepdims=True)
            e = np.exp(s - ms)
            r = e / e.sum(axis=2, keepdims=True)
            g = np.where((f > 0)[:, :, None], f[:, :, None] * r, 0.0).sum(axis=1)
        # ---- leaves
        w = f.sum(axis=1)[:, None]                                   # [B, 1, H, W]
        d = loc - loc[:1]                                            # [K, C, H, W]: distances from the first component
        mr = (f[:, :, None] * d[None]).sum(axis=1) / w
        mean = loc[0][None] + mr
        var = (f[:, :, None] * ((scale ** 2)[None] + (d[None] - mr[:, None]) ** 2)).sum(axis=1) / w
    reached = (w > 0) & ~bad[:, None, None, None]
    hid = np.isnan(x)
    mean = np.where(hid, np.where(reached, mean, np.nan), x)
    var = np.where(hid, np.where(reached, var, np.nan), 0.0)
    f[bad] = np.nan
    return mean, var, f


def restate_model(model, case, acts, x, y=None, all_classes=None):
    """The restatement on the device's own fp32 activations, with the tables the kernel reads."""
    if all_classes is None:
        all_classes = y is None
    return posterior_moments(ref.case_geometry(case), acts, model._topdown_logw(), model.base_layer.loc, model.base_layer.scale,
                             x, y, all_classes)


def restate_float64(model, case, x, y=None, all_classes=None):
    """The oracle's float64 forward under ``x`` (host), then the restatement on its activations: float64 end to end."""
    sd64, plan = ref.state(model, torch.float64), ref.case_plan(case)
    x = x.detach().cpu().double()
    if all_classes is None:
        all_classes = y is None
    return posterior_moments(ref.case_geometry(case), ref.host_activations(sd64, x, plan), ref.host_logws(sd64, plan),
                             sd64['base_layer.loc'], sd64['base_layer.scale'], x, None if y is None else y.cpu(), all_classes)
