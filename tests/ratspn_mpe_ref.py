"""Restatement of RatSpn.mpe's top-down pass (mode 0 of dpk_ratspn_topdown, csrc/ratspn_topdown.hip) in plain numpy on the
host, statement for statement, from the fp32 activations the caller hands in -- the DEVICE's own, when a device result is
replayed (tests/ratspn_posterior_ref.py does the same for mode 2).

For one sum node with `count` inputs:
  1. s(n) = fl(fl(a_i + a_j) + lw(n)) in np.float32, this operand order;
  2. the choice is the FIRST maximum of s: ties go to the smallest n (every lane keeps its first best, the wave reduction
     prefers the smaller index among equal values).
Leaves: an observed variable keeps x[b, f]; a NaN variable takes the mode of the chosen channel of its region: loc (Gaussian),
[1 / (1 + exp(-logit)) >= 0.5] in float32 (Bernoulli).

Every operation is an fp32 addition, a comparison or a table look-up, so there is no rounding freedom between this and the
kernel: every row must agree.  (The Bernoulli mode evaluates exp in float32 here as there; the two exponentials can differ
by an ulp only where exp(-logit) is within an ulp of 1, |logit| < 1e-7 and not 0 -- the tests keep such logits out.)

A helper module (no tests in it)."""
import numpy as np
import torch


def _f32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t), dtype=np.float32)


def _first_max(s: np.ndarray) -> np.ndarray:
    """s [..., count] float32 without NaN -> index of the first maximum along the last axis."""
    assert not np.isnan(s).any(), 'mpe_replay: NaN score (the kernel keeps a NaN it meets first in a lane; not restated)'
    return np.argmax(s, axis=-1)


def mpe_replay(acts, logws, src, leaf, x, y):
    """acts: [leaf output [B, reps 2^depth, I], sum level 1 output [B, reps 2^(depth-1), S], ...] fp32; logws: log-softmax
    weights of the sum levels 1 .. depth-1, then of the root (RatSpn._topdown_logw()); src [reps, D]
    (RatSpn._topdown_src()); leaf = (dist, p0, p1) (RatSpn._leaf_params()); x [B, D] with NaN = to be completed; y [B] integer
    labels or None (class 0); all host or device tensors / arrays.
    Returns (completion [B, D] float32, repetition [B], leaf channels [B, 2^depth])."""
    x = _f32(x)
    B, D = x.shape
    acts = [_f32(a) for a in acts]
    logws = [_f32(w) for w in logws]
    src = (src.cpu().numpy() if torch.is_tensor(src) else np.asarray(src)).astype(np.int64)
    dist, p0 = leaf[0], _f32(leaf[1])
    depth = len(acts)
    reps = src.shape[0]
    G0 = 1 << depth
    d = p0.shape[2]
    C = logws[depth - 1].shape[0]
    ycls = np.zeros(B, np.int64) if y is None else (y.cpu().numpy() if torch.is_tensor(y) else np.asarray(y)).astype(np.int64)
    ycls = np.clip(ycls, 0, C - 1)                               # (the kernel clamps a label outside [0, C))
    rows = np.arange(B)

    # ---- root: one of the reps * N^2 inputs (partition = repetition, (i, j) = nodes of its two regions)
    A = acts[depth - 1]
    N = A.shape[2]
    NN = N * N
    A = A.reshape(B, reps, 2, N)
    s = (A[:, :, 0, :, None] + A[:, :, 1, None, :]).reshape(B, reps * NN) + logws[depth - 1][ycls]
    assert s.dtype == np.float32
    pick = _first_max(s)
    rep = pick // NN
    e = pick - rep * NN
    cur = np.stack([e // N, e % N], axis=1)                      # [B, 2]: the node chosen in each region of the level

    # ---- sum levels, top to bottom: level t has G = 2^(depth - t) regions in the repetition
    for t in range(depth - 1, 0, -1):
        G = 1 << (depth - t)
        A = acts[t - 1]
        N = A.shape[2]
        NN = N * N
        g = rep[:, None] * G + np.arange(G)[None, :]             # [B, G]
        lw = logws[t - 1][g, cur]                                # [B, G, NN]
        a_i, a_j = A[rows[:, None], 2 * g], A[rows[:, None], 2 * g + 1]
        s = (a_i[:, :, :, None] + a_j[:, :, None, :]).reshape(B, G, NN) + lw
        assert s.dtype == np.float32
        pick = _first_max(s)
        cur = np.stack([pick // N, pick % N], axis=2).reshape(B, 2 * G)

    # ---- leaves: every variable from the chosen channel of its region, in variable order
    sf = src[rep]                                                # [B, D]
    rl, j = sf // d, sf % d
    chan = cur[rows[:, None], rl]
    q0 = p0[rep[:, None] * G0 + rl, chan, j]
    if dist == 0:
        v = q0
    else:
        with np.errstate(over='ignore'):
            sig = np.float32(1.0) / (np.float32(1.0) + np.exp(-q0))
        assert sig.dtype == np.float32
        v = (sig >= np.float32(0.5)).astype(np.float32)
    out = np.where(np.isnan(x), v, x).astype(np.float32)
    return torch.from_numpy(out), torch.from_numpy(rep), torch.from_numpy(cur)
