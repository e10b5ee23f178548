"""Restatement of RatSpn.posterior_moments' top-down pass (dpr_ratspn_moments, csrc/rat/ratspn_moments.hip) in plain numpy
on the host, taking the activations of the bottom-up pass as input.

The definition, for a row b with the class cls of the root:
  root:    s(q) = fl(fl(a_i + a_j) + lw(q)) over the reps N^2 inputs of class cls (over the C reps N^2 inputs of all classes
           when there are no labels and `all_classes` is set), formed in the dtype of the activations handed in -- numpy
           float32 arithmetic, this operand order, on the fp32 activations of a device; float64 on the oracle's;
           m = max_q s(q), e(q) = exp(s(q) - m), r(q) = e(q) / sum e: m, e, the flows and the moments in float64;
           F[2p][i] = sum_j r(p, i, j), F[2p + 1][j] = sum_i r(p, i, j);
  level t, top to bottom: for region g and node o with F[g][o] > 0 the scores of that node's N^2 inputs with logw[t][g, o, :],
           m / e / r as above (normalised by their own sum), F'[2g][i] += F[g][o] sum_j r(i, j) and
           F'[2g + 1][j] += F[g][o] sum_i r(i, j); nodes with zero flow are skipped;
  leaves:  for a NaN variable f over every repetition and channel k of its leaf region (through src):
           w = sum F_k, mean = sum F_k m_k / w, var = sum F_k (v_k + (m_k - mean)^2) / w,
           (m_k, v_k) = (loc, scale^2) / (p, p (1 - p)) with p = sigmoid(logit);
  an observed entry returns x[b, f] and var 0; a row whose root maximum is -inf or NaN returns NaN in its NaN entries (and
  in all of its leaf flows).

A helper module (no tests in it)."""
import numpy as np
import torch

ROW_CHUNK = 32          # rows per step: the level-1 scores of the 784-variable model are 65 536 a row


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _flows(acts, logws, reps, ycls, all_classes):
    """acts [depth] arrays of one dtype (float32 or float64), logws the same dtype, ycls [B] or None.
    Returns (leaf flows [B, reps 2^depth, I] float64, impossible [B] bool)."""
    depth = len(acts)
    B = acts[0].shape[0]
    A = acts[depth - 1]
    N = A.shape[2]
    A = A.reshape(B, reps, 2, N)
    pre = A[:, :, 0, :, None] + A[:, :, 1, None, :]                          # [B, reps, N, N], the activations' dtype
    lw_root = logws[depth - 1]
    C = lw_root.shape[0]
    if ycls is None:
        lw = lw_root.reshape(C, reps, N, N)[None] if all_classes else lw_root[0].reshape(1, 1, reps, N, N)
    else:
        lw = lw_root[ycls].reshape(B, 1, reps, N, N)
    with np.errstate(invalid='ignore', over='ignore'):
        s = (pre[:, None] + lw).astype(pre.dtype)                            # [B, nC, reps, N, N]
        s64 = s.astype(np.float64)
        m = np.max(s64.reshape(B, -1), axis=1)                               # (np.max propagates NaN)
        impossible = ~(m > -np.inf)
        e = np.exp(s64 - np.where(impossible, 0.0, m)[:, None, None, None, None])
        r = e / e.reshape(B, -1).sum(axis=1)[:, None, None, None, None]
        r = np.where(impossible[:, None, None, None, None], 0.0, r)
    F = np.stack([r.sum(axis=(1, 4)), r.sum(axis=(1, 3))], axis=2)           # [B, reps, 2, N]
    F = F.reshape(B, reps * 2, N)
    for t in range(depth - 1, 0, -1):
        A = acts[t - 1]                                                      # [B, reps 2G, N]
        N = A.shape[2]
        RG, S = F.shape[1], F.shape[2]
        lw = logws[t - 1].reshape(1, RG, S, N, N)
        pre = A[:, 0::2, :, None] + A[:, 1::2, None, :]                      # [B, RG, N, N]
        with np.errstate(invalid='ignore', over='ignore'):
            s = (pre[:, :, None] + lw).astype(pre.dtype).astype(np.float64)  # [B, RG, S, N, N]
            m = s.max(axis=(3, 4), keepdims=True)
            e = np.exp(s - m)
            r = e / e.sum(axis=(3, 4), keepdims=True)
        live = (F > 0)[:, :, :, None, None]
        fr = np.where(live, F[:, :, :, None, None] * np.where(live, r, 0.0), 0.0)
        fr = fr.sum(axis=2)                                                  # [B, RG, N, N]
        F = np.stack([fr.sum(axis=3), fr.sum(axis=2)], axis=2).reshape(B, RG * 2, N)
    F = np.where(impossible[:, None, None], np.nan, F)
    return F, impossible


def posterior_moments(acts, logws, src, leaf, x, y=None, all_classes=False):
    """acts: [leaf output [B, reps 2^depth, I], sum level 1 output, ...], all float32 (a device's) or all float64 (the
    oracle's); logws: log-softmax weights of the sum levels 1 .. depth-1, then of the root (RatSpn._topdown_logw()); src
    [reps, D] (RatSpn._topdown_src()); leaf = (dist, p0, p1) (RatSpn._leaf_params()); x [B, D] with NaN = unobserved; y [B]
    integer labels or None.  Returns (mean [B, D], var [B, D], leaf_flow [B, reps 2^depth, I]) as float64 arrays."""
    acts = [np.ascontiguousarray(_np(a)) for a in acts]
    dtype = acts[0].dtype
    assert dtype in (np.float32, np.float64) and all(a.dtype == dtype for a in acts)
    logws = [np.ascontiguousarray(_np(w)).astype(dtype) for w in logws]
    x = _np(x).astype(np.float64)
    B, D = x.shape
    src = _np(src).astype(np.int64)
    reps = src.shape[0]
    dist, p0, p1 = leaf
    p0 = _np(p0).astype(np.float64)
    G0 = 1 << len(acts)
    d = p0.shape[2]
    ycls = None if y is None else _np(y).astype(np.int64)
    if dist == 0:
        mk_all, vk_all = p0, _np(p1).astype(np.float64) ** 2
    else:
        mk_all = 1.0 / (1.0 + np.exp(-p0))
        vk_all = mk_all * (1.0 - mk_all)
    mean, var = np.empty((B, D)), np.empty((B, D))
    flows = np.empty((B, reps * G0, p0.shape[1]))
    for lo in range(0, B, ROW_CHUNK):
        hi = min(B, lo + ROW_CHUNK)
        F, impossible = _flows([a[lo:hi] for a in acts], logws, reps, None if ycls is None else ycls[lo:hi], all_classes)
        flows[lo:hi] = F
        F = np.nan_to_num(F)
        per_rep = []
        for rep in range(reps):
            rl, j = src[rep] // d, src[rep] % d
            region = rep * G0 + rl
            per_rep.append((F[:, region, :], mk_all[region, :, j][None], vk_all[region, :, j][None]))   # [b, D, I], [1, D, I]
        w = sum(Fk.sum(axis=2) for Fk, _, _ in per_rep)
        with np.errstate(invalid='ignore', divide='ignore'):
            mu = sum((Fk * mk).sum(axis=2) for Fk, mk, _ in per_rep) / w
            va = sum((Fk * (vk + (mk - mu[:, :, None]) ** 2)).sum(axis=2) for Fk, mk, vk in per_rep) / w
        mu[impossible] = np.nan
        va[impossible] = np.nan
        hidden = np.isnan(x[lo:hi])
        mean[lo:hi] = np.where(hidden, mu, x[lo:hi])
        var[lo:hi] = np.where(hidden, va, 0.0)
    return mean, var, flows


def restate_model(model, acts, x, y=None, all_classes=None):
    """The restatement on a model's own tables (host or device tensors)."""
    dist, p0, p1 = model._leaf_params()
    if all_classes is None:
        all_classes = y is None
    return posterior_moments([a.detach().cpu() for a in acts], [w.detach().cpu() for w in model._topdown_logw()],
                             model._topdown_src().cpu(), (dist, p0.detach().cpu(), None if p1 is None else p1.detach().cpu()),
                             x.cpu(), None if y is None else y.cpu(), all_classes)
