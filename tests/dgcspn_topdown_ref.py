"""Restatement of the DGC-SPN top-down pass (dpg_dgcspn_topdown, DgcSpn.sample / sample_conditional) in plain numpy on the
host.

The definition is the one at the top of csrc/dgc/dgcspn_topdown.hip, statement for statement:
  - product values are never kept as the model's maps: a product is the fp32 sum of its four taps in row-major tap order,
    ((v0 + v1) + v2) + v3, a tap outside the input map is 0 and has no child, the input coordinate of a tap is
    out * stride + t * dilation - pad_before, and a level that is not depthwise decodes its output channel in
    itertools.product order (tap t = 2 th + tw gets digit (oc // Cin^(3 - t)) % Cin);
  - root: s(i) = prod_value(i) + logw_root[y, i] in fp32 (here: numpy float32 arithmetic on the fp32 activations the caller
    hands in -- the DEVICE's, when a device result is replayed), one i by inverse CDF over exp(s - max s) in index order;
  - every sum layer from the top down: an active position (o, h, w) draws its input channel c by inverse CDF over
    exp(s - max), s(c) = prod_value_below(c, h, w) + logw[o, c, h, w]; a maximum of -inf or NaN: by the bare weights,
    exp(logw); the chosen product activates its taps with the decoded channels;
  - the max, the exp and the CDF are float64 here, where the kernel has fp32; the pick is the first n with
    u * total < c(n), the last input when there is none;
  - leaves: an observed entry is kept bit for bit, a NaN entry is loc + scale * z, z = sqrt(-2 log(1 - u1)) cos(2 pi u2);
  - a pixel that no path reaches is returned as given and has component -1;
  - u = oracle.ratspn_oracle.hash_uniform(seed, row * slots_per_row + slot): slot 0 the root, base_t + h * Wout + w the
    position (h, w) of sum layer t (base_1 = 1, then one block per sum layer, bottom to top), base_L + 2 ((c H + h) W + w),
    + 1 the two uniforms of leaf entry (c, h, w);
  - without activations (DgcSpn.sample) every draw is by the bare weights.

Besides the samples it returns per row the MARGIN: the smallest distance, over the row's categorical draws, between u and a
step of the normalised float64 CDF.  A row whose margin is below what fp32 rounding of the kernel's CDF can move may
legitimately choose another input there; tests compare on the rows above a threshold.

It also asserts what makes the pass well defined: no position of any map is activated twice.

A helper module (no tests in it)."""
import numpy as np
import torch

from oracle import dgcspn_oracle as dorc
from oracle import ratspn_oracle as orc

counter_uniform = orc.hash_uniform


def geometry(in_features, n_batch, sum_channels, depthwise, n_pooling):
    """One row per product level, bottom to top, from the oracle's schedule: (Cin, Hin, Win, Cout, Hout, Wout, pad_left,
    pad_right, pad_top, pad_bottom, stride, dilation, depthwise) -- the table of include/deeprob_dgc.h."""
    plan = dorc.schedule(in_features, n_batch, sum_channels, depthwise, n_pooling)
    rows, shape = [], (n_batch, in_features[1], in_features[2])
    for step in plan:
        if step[0] == 'prod':
            _, pad, stride, dilation, dw = step
            # (the geometry of a level from its pads: 'valid' has none, 'final' pads one side only, 'full' all four)
            ke = dilation + 1
            oh = int(np.ceil((pad[2] + pad[3] + shape[1] - ke + 1) / stride))
            ow = int(np.ceil((pad[0] + pad[1] + shape[2] - ke + 1) / stride))
            out = (shape[0] if dw else shape[0] ** 4, oh, ow)
            rows.append(list(shape) + list(out) + list(pad) + [stride, dilation, int(dw)])
            shape = out
        else:
            shape = (sum_channels,) + shape[1:]
    return rows


def slot_layout(geom, c, h, w):
    base, nxt = [0], 1
    for row in geom[:-1]:
        base.append(nxt)
        nxt += row[4] * row[5]
    base.append(nxt)
    return base, nxt + 2 * c * h * w


def _taps(row):
    """[(tap index, dh, dw)] with the input offset of a tap relative to out * stride."""
    pl, pt, dil = row[6], row[8], row[11]
    return [(t, (t >> 1) * dil - pt, (t & 1) * dil - pl) for t in range(4)]


def _digit(row, oc, t):
    cin = row[0]
    return oc if row[12] else (oc // cin ** (3 - t)) % cin


def product_map(row, a32):
    """[R, Cout, Hout, Wout] float32: every product of the level over the maps a32 [R, Cin, Hin, Win], ((v0+v1)+v2)+v3."""
    cin, hin, win, cout, hout, wout = row[:6]
    stride = row[10]
    oc = np.arange(cout)
    oh, ow = np.arange(hout) * stride, np.arange(wout) * stride
    acc = None
    for t, dh, dw in _taps(row):
        ih, iw = oh + dh, ow + dw
        okh, okw = (ih >= 0) & (ih < hin), (iw >= 0) & (iw < win)
        v = a32[:, _digit(row, oc, t)][:, :, np.clip(ih, 0, hin - 1)][:, :, :, np.clip(iw, 0, win - 1)]
        v = np.where((okh[:, None] & okw[None, :])[None, None], v, np.float32(0.0)).astype(np.float32)
        acc = v if acc is None else (acc + v).astype(np.float32)
    return acc


def _choose(s32, lw32, u):
    """s32 [M, count] float32 scores or None (bare weights), lw32 [M, count], u [M] -> (pick [M], margin [M])."""
    lw = lw32.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        if s32 is None:
            e = np.exp(lw)
        else:
            s = s32.astype(np.float64)
            m = np.max(s, axis=1)                                    # (np.max propagates NaN)
            live = m > -np.inf                                       # False for -inf and for NaN
            shift = np.where(live, m, 0.0)[:, None]
            e = np.where(live[:, None], np.exp(s - shift), np.exp(lw))
    cdf = np.cumsum(e, axis=1)
    cn = cdf / cdf[:, -1:]
    uu = u.astype(np.float64)[:, None]
    pick = np.minimum((cn <= uu).sum(axis=1), lw.shape[1] - 1)
    margin = np.abs(cn - uu).min(axis=1)
    return pick, margin


def topdown_sample(geom, in_features, acts, logws, loc, scale, x, y, seed, n_rows=None):
    """geom: geometry(...); acts: [leaf output [B, K, H, W], sum layer 1 output, ...] (a leading dimension of 1 stands for B
    identical rows) or None (no evidence: the weights alone); logws: log-softmax weights of the sum layers 1 .. L-1, then of
    the root; loc, scale [K, C, H, W]; x [B, C, H, W] with NaN = to be drawn, or None (n_rows rows, everything drawn); y [B]
    integer labels or None (class 0).  Host tensors / arrays.
    Returns (samples [B, C, H, W] float32, root index [B], component per pixel [B, H W] (-1: out of scope), margin [B])."""
    f32 = lambda t: np.ascontiguousarray((t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)), dtype=np.float32)
    C, H, W = in_features
    L = len(geom)
    if x is None:
        B = int(n_rows)
        x = np.full((B, C, H, W), np.nan, np.float32)
    else:
        x = f32(x)
        B = x.shape[0]
    if acts is not None:
        acts = [f32(a) for a in acts]
        assert len(acts) == L
    logws = [f32(w) for w in logws]
    assert len(logws) == L
    loc, scale = f32(loc), f32(scale)
    ycls = np.zeros(B, np.int64) if y is None else (y.cpu().numpy() if torch.is_tensor(y) else np.asarray(y)).astype(np.int64)
    base, slots = slot_layout(geom, C, H, W)
    rows_all = np.arange(B)
    ctr0 = rows_all.astype(np.uint64) * np.uint64(slots)
    margin = np.full(B, np.inf)

    def prod_of(level, rows):
        """[len(rows), Cout, Hout, Wout] product values of `level` for these rows, or None without evidence."""
        if acts is None:
            return None
        a = acts[level]
        pm = product_map(geom[level], a if a.shape[0] == 1 else a[rows])
        return np.broadcast_to(pm, (len(rows),) + pm.shape[1:]) if a.shape[0] == 1 and len(rows) != 1 else pm

    def activate(level, chosen_below, rows, oc, oh, ow):
        row = geom[level]
        for t, dh, dw in _taps(row):
            ih, iw = oh * row[10] + dh, ow * row[10] + dw
            ok = (ih >= 0) & (ih < row[1]) & (iw >= 0) & (iw < row[2])
            r, hh, ww = rows[ok], (ih[ok] if np.ndim(ih) else ih), (iw[ok] if np.ndim(iw) else iw)
            if len(r) == 0:
                continue
            assert (chosen_below[r, hh, ww] == -1).all(), 'a position is reached twice: the circuit is not decomposable'
            chosen_below[r, hh, ww] = _digit(row, oc[ok], t)

    # ---- root: one of the Cr Hr Wr products of the last level
    g = geom[L - 1]
    hw = g[4] * g[5]
    lw = logws[L - 1][ycls]
    pm = prod_of(L - 1, rows_all)
    s = None if pm is None else (pm.reshape(B, -1) + lw).astype(np.float32)
    root, m = _choose(s, lw, counter_uniform(seed, ctr0))
    margin = np.minimum(margin, m)
    chosen = np.full((B, g[1], g[2]), -1, np.int64)              # the map of sum layer L - 1 (the leaf map when L = 1)
    oc, p = root // hw, root % hw
    activate(L - 1, chosen, rows_all, oc, p // g[5], p % g[5])

    # ---- sum layers, top to bottom: layer t sits on product level t - 1
    for t in range(L - 1, 0, -1):
        g = geom[t - 1]
        below = np.full((B, g[1], g[2]), -1, np.int64)
        lwt = logws[t - 1]                                       # [S, Cout, Hout, Wout]
        active_rows = np.nonzero((chosen >= 0).any(axis=(1, 2)))[0]
        pm = prod_of(t - 1, active_rows)                         # rows of pm follow active_rows
        where = np.full(B, -1, np.int64)
        where[active_rows] = np.arange(len(active_rows))
        for h in range(g[4]):
            for w in range(g[5]):
                rows = np.nonzero(chosen[:, h, w] >= 0)[0]
                if len(rows) == 0:
                    continue
                lw = lwt[chosen[rows, h, w], :, h, w]            # [R, count]
                s = None if pm is None else (pm[where[rows], :, h, w] + lw).astype(np.float32)
                u = counter_uniform(seed, ctr0[rows] + np.uint64(base[t] + h * g[5] + w))
                c, m = _choose(s, lw, u)
                margin[rows] = np.minimum(margin[rows], m)
                activate(t - 1, below, rows, c, np.full(len(rows), h), np.full(len(rows), w))
        chosen = below

    # ---- leaves
    comp = chosen.reshape(B, H * W)
    k = np.maximum(chosen, 0)                                    # [B, H, W]
    cc, hh, ww = np.meshgrid(np.arange(C), np.arange(H), np.arange(W), indexing='ij')
    kk = k[:, None].repeat(C, axis=1)                            # [B, C, H, W]
    q0 = loc[kk, cc[None], hh[None], ww[None]].astype(np.float64)
    q1 = scale[kk, cc[None], hh[None], ww[None]].astype(np.float64)
    f = ((cc * H + hh) * W + ww).astype(np.uint64)[None]
    ctr = ctr0[:, None, None, None] + np.uint64(base[L]) + np.uint64(2) * f
    u1 = counter_uniform(seed, ctr).astype(np.float64)
    u2 = counter_uniform(seed, ctr + np.uint64(1)).astype(np.float64)
    z = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)
    v = (q0 + q1 * z).astype(np.float32)
    draw = np.isnan(x) & (chosen >= 0)[:, None]
    out = np.where(draw, v, x)
    return torch.from_numpy(out), torch.from_numpy(root), torch.from_numpy(comp), margin


# ---- the cases of the host and device tests ----------------------------------------------------------------------------
CASES = {
    'dw4': dict(in_features=(1, 4, 4), n_batch=2, sum_channels=2, depthwise=True, n_pooling=0),
    # an odd map under a pooling level: the last row and column are in nobody's scope
    'odd5': dict(in_features=(1, 5, 5), n_batch=3, sum_channels=2, depthwise=True, n_pooling=1),
    # the channel decode, multi-channel leaves, classes
    'mixed6': dict(in_features=(2, 6, 6), n_batch=2, sum_channels=2, depthwise=[False, True], n_pooling=1, out_classes=3),
    # not depthwise throughout: the root over 16 x 4 x 4
    'full3': dict(in_features=(1, 3, 3), n_batch=2, sum_channels=2, depthwise=False, n_pooling=0),
    # maps up to 27 x 27: more positions than threads
    'dw12': dict(in_features=(1, 12, 12), n_batch=6, sum_channels=7, depthwise=True, n_pooling=0),
    # 81 inputs a sum node (more than a wave's 64 lanes: the wave scan of the sum layers), the root over 81 x 4 x 4
    'wide3': dict(in_features=(1, 3, 3), n_batch=3, sum_channels=3, depthwise=False, n_pooling=0),
}
B = 301
STAT_ROWS = 1 << 16
STAT_SEED = 20250311


def case_geometry(case):
    kw = CASES[case]
    return geometry(kw['in_features'], kw['n_batch'], kw['sum_channels'], kw['depthwise'], kw['n_pooling'])


def case_plan(case):
    kw = CASES[case]
    return dorc.schedule(kw['in_features'], kw['n_batch'], kw['sum_channels'], kw['depthwise'], kw['n_pooling'])


def make_model(case, seed=31):
    """The case's model on the host, eval mode, with leaf scales away from 1 so that a wrong scale shows."""
    from deeprob.spn.models import DgcSpn
    torch.manual_seed(seed)
    model = DgcSpn(**CASES[case]).eval()
    with torch.no_grad():
        gen = torch.Generator().manual_seed(seed + 1)
        model.base_layer.scale.copy_(0.5 + torch.rand(model.base_layer.scale.shape, generator=gen))
    return model


def make_evidence(model, case, b=B, seed=32):
    """[b, C, H, W] on the host: 50 % NaN, row 0 all NaN, row 1 fully observed, row 2 with its observed pixels at
    loc + 40 scale of component 0 -- every score of that row is far below where expf underflows -- and labels (or None)."""
    kw = CASES[case]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(b, *kw['in_features'], generator=gen)
    if b > 2:
        x[2] = (model.base_layer.loc[0] + 40.0 * model.base_layer.scale[0]).detach()
    x[torch.rand(x.shape, generator=gen) < 0.5] = float('nan')
    x[0] = float('nan')
    if b > 1:
        x[1] = torch.nan_to_num(x[1], nan=0.0)
    if b > 2:
        assert torch.isnan(x[2]).any() and not torch.isnan(x[2]).all()
    y = (torch.arange(b) % kw['out_classes']) if kw.get('out_classes', 1) > 1 else None
    return x, y


def state(model, dtype=torch.float32):
    return {k: (v.detach().to(dtype) if v.is_floating_point() else v.detach().clone()) for k, v in model.state_dict().items()}


def host_activations(sd, x, plan):
    """The activations topdown_sample wants, from the oracle's forward: the leaf map, then every sum layer's output."""
    _, acts = dorc.dgcspn_forward(sd, x, plan, return_activations=True)
    keep = [acts[0]] + [acts[i + 1] for i, step in enumerate(plan) if step[0] == 'sum']
    return [a.detach() for a in keep]


def host_logws(sd, plan):
    out = [torch.log_softmax(sd['layers.{}.weight'.format(i)], dim=1) for i, step in enumerate(plan) if step[0] == 'sum']
    out.append(torch.log_softmax(sd['root_layer.weight'], dim=1))
    return out


def exact_marginals(sd64, x_row, plan, cls=0):
    """d log p(x_observed, y = cls) / d z in float64, z the leaf layer's output: [K, H, W], the exact posterior probability
    that pixel (h, w) is reached with component k (0 everywhere at a pixel out of scope)."""
    with torch.enable_grad():
        z = dorc.spatial_gaussian(x_row.double(), sd64['base_layer.loc'], sd64['base_layer.scale']).detach().requires_grad_(True)
        out = dorc.dgcspn_forward(sd64, x_row.double(), plan, z=z)
        grad, = torch.autograd.grad(out[0, cls], z)
    return grad[0].numpy()


def half_observed_row(model, case, seed=33):
    """[1, C, H, W]: half of the pixels observed, at values a component or two away from the leaf locations."""
    kw = CASES[case]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(1, *kw['in_features'], generator=gen)
    c, h, w = kw['in_features']
    hide = torch.zeros(h * w, dtype=torch.bool)
    hide[torch.randperm(h * w, generator=gen)[:(h * w) // 2]] = True
    x[:, :, hide.view(h, w)] = float('nan')
    return x


def component_frequencies(comp, n_components):
    """[K, H W] frequencies of the components among the rows of comp [N, H W] (-1 counts for none)."""
    comp = comp.numpy() if torch.is_tensor(comp) else np.asarray(comp)
    return np.stack([(comp == k).mean(axis=0) for k in range(n_components)])


def check_frequencies(freq, marg, n, where=''):
    """Every (component, pixel) frequency within 5 standard errors of the exact marginal, over the cells with an expected
    count of at least 50; a cell of marginal exactly 0 (a pixel out of scope) must be empty."""
    marg = marg.reshape(freq.shape)
    se = np.sqrt(marg * (1.0 - marg) / n)
    cells = marg * n >= 50
    assert cells.sum() >= freq.shape[1] // 2, 'a posterior worth testing has populated cells'
    dev = np.abs(freq - marg)[cells] / np.maximum(se[cells], 1e-300)
    print('%s: %d cells, largest deviation %.2f standard errors' % (where, int(cells.sum()), float(dev.max())))
    assert (dev <= 5.0).all(), (where, float(dev.max()))
    assert (freq[marg == 0.0] == 0.0).all()
