"""Restatement of mode 3 of the DGC-SPN top-down pass (dpg_dgcspn_topdown with DPG_MODE_MPE, DgcSpn.mpe_completion) in
plain numpy float32 on the host.

The definition is the one at the top of csrc/dgc/dgcspn_topdown.hip.  The scores are mode 2's, with the kernel's operand
order: prod_value = ((v0 + v1) + v2) + v3 over the four taps (tests/dgcspn_topdown_ref.py: product_map), then
s(n) = prod_value(n) + logw(n), every operation rounded to float32.  At the root and at every active position of every sum
layer, with m the NaN-propagating maximum of the scores:
  - m > -inf: the first n in index order with s(n) == m;
  - otherwise (m is -inf or NaN): the first n in index order that maximises logw(n), a NaN weight never over a number.
A reached pixel's NaN entries are loc[k, c, h, w] of its component k, its observed entries are kept; a pixel that no path
reaches is returned as given and has component -1.

Nothing here is transcendental and nothing is accumulated in another order than the kernel's, so a device result is
replayed bit for bit from the device's own activations: no tolerance and no exempt rows.

A helper module (no tests in it)."""
import numpy as np
import torch

from tests.dgcspn_topdown_ref import (geometry, product_map, host_activations, host_logws, state, CASES, make_model,  # noqa: F401
                                      make_evidence)


def taps(row):
    """[(tap index, dh, dw)]: the input coordinate of tap t = 2 th + tw is out * stride + (dh, dw)."""
    pl, pt, dil = row[6], row[8], row[11]
    return [(t, (t >> 1) * dil - pt, (t & 1) * dil - pl) for t in range(4)]


def tap_channel(row, oc, t):
    """depthwise: the output channel itself; otherwise digit t of oc in base Cin, the most significant first"""
    cin = row[0]
    return oc if row[12] else (oc // cin ** (3 - t)) % cin


def first_max(s32, lw32):
    """s32, lw32 [M, count] float32 -> pick [M]: the node rule above, row by row."""
    with np.errstate(invalid='ignore'):
        m = np.max(s32, axis=1)                                          # (np.max propagates NaN)
        live = m > -np.inf                                               # False for -inf and for NaN
        by_score = np.argmax(s32 == m[:, None], axis=1)                  # the first True
    by_weight = np.argmax(np.where(np.isnan(lw32), -np.inf, lw32), axis=1)   # (np.argmax: the first maximum)
    return np.where(live, by_score, by_weight)


def topdown_mpe(geom, in_features, acts, logws, loc, x, y):
    """geom: geometry(...); acts: [leaf output [B, K, H, W], sum layer 1 output, ...]; logws: log-softmax weights of the sum
    layers 1 .. L-1, then of the root; loc [K, C, H, W]; x [B, C, H, W] with NaN = to be filled; y [B] integer labels or None
    (class 0).  Host tensors / arrays, read as float32.
    Returns (out [B, C, H, W] float32, choice [B, 1 + H W] int32: the root's input index, then the component per pixel)."""
    f32 = lambda t: np.ascontiguousarray((t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)), dtype=np.float32)
    C, H, W = in_features
    L = len(geom)
    x = f32(x)
    n_rows = x.shape[0]
    acts, logws, loc = [f32(a) for a in acts], [f32(w) for w in logws], f32(loc)
    assert len(acts) == L and len(logws) == L
    ycls = np.zeros(n_rows, np.int64) if y is None else (y.cpu().numpy() if torch.is_tensor(y) else np.asarray(y)).astype(np.int64)
    rows_all = np.arange(n_rows)

    def activate(level, chosen_below, rows, oc, oh, ow):
        row = geom[level]
        for t, dh, dw in taps(row):
            ih, iw = oh * row[10] + dh, ow * row[10] + dw
            ok = (ih >= 0) & (ih < row[1]) & (iw >= 0) & (iw < row[2])
            r = rows[ok]
            if len(r) == 0:
                continue
            assert (chosen_below[r, ih[ok], iw[ok]] == -1).all(), 'a position is reached twice: the circuit is not decomposable'
            chosen_below[r, ih[ok], iw[ok]] = tap_channel(row, oc[ok], t)

    # ---- root: one of the Cr Hr Wr products of the last level
    g = geom[L - 1]
    hw = g[4] * g[5]
    lw = logws[L - 1][ycls]
    s = (product_map(g, acts[L - 1]).reshape(n_rows, -1) + lw).astype(np.float32)
    root = first_max(s, lw)
    chosen = np.full((n_rows, g[1], g[2]), -1, np.int64)             # the map of sum layer L - 1 (the leaf map when L = 1)
    oc, p = root // hw, root % hw
    activate(L - 1, chosen, rows_all, oc, p // g[5], p % g[5])

    # ---- sum layers, top to bottom: layer t sits on product level t - 1
    for t in range(L - 1, 0, -1):
        g = geom[t - 1]
        below = np.full((n_rows, g[1], g[2]), -1, np.int64)
        lwt = logws[t - 1]                                           # [S, Cout, Hout, Wout]
        pm = product_map(g, acts[t - 1])
        for h in range(g[4]):
            for w in range(g[5]):
                rows = np.nonzero(chosen[:, h, w] >= 0)[0]
                if len(rows) == 0:
                    continue
                lw = lwt[chosen[rows, h, w], :, h, w]                # [R, count]
                s = (pm[rows, :, h, w] + lw).astype(np.float32)
                activate(t - 1, below, rows, first_max(s, lw), np.full(len(rows), h), np.full(len(rows), w))
        chosen = below

    # ---- leaves: the location of the chosen component, bit for bit
    k = np.maximum(chosen, 0)                                        # [B, H, W]
    cc, hh, ww = np.meshgrid(np.arange(C), np.arange(H), np.arange(W), indexing='ij')
    mode = loc[k[:, None].repeat(C, axis=1), cc[None], hh[None], ww[None]]
    fill = np.isnan(x) & (chosen >= 0)[:, None]
    out = np.where(fill, mode, x)
    choice = np.concatenate([root[:, None], chosen.reshape(n_rows, H * W)], axis=1).astype(np.int32)
    return torch.from_numpy(out), torch.from_numpy(choice)


# ---- the row of the sanity check against the sampler ----------------------------------------------------------------------------
SANITY_ROW_SEED = 38        # half_observed_row(model, 'dw4', seed): the root posterior's two largest entries lie >= 0.1 apart


def root_posterior64(model, case, row, cls=0):
    """The exact posterior over the root's inputs given the row's observed entries, float64: softmax over
    last product map + root log-weights of the oracle's forward ([Cr Hr Wr], index order of `choice[:, 0]`)."""
    from oracle import dgcspn_oracle as dorc
    from tests.dgcspn_topdown_ref import case_plan
    plan = case_plan(case)
    sd64 = state(model, torch.float64)
    _, acts = dorc.dgcspn_forward(sd64, row.double(), plan, return_activations=True)
    s = acts[-1][0].reshape(-1) + torch.log_softmax(sd64['root_layer.weight'], dim=1)[cls]
    return torch.softmax(s, dim=0).numpy()
