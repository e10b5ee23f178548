"""Restatement of RatSpn.sample_conditional's top-down pass (mode 2 of dpk_ratspn_topdown) in plain numpy on the host.

The definition is the one at the top of csrc/ratspn_topdown.hip, statement for statement.  For one sum node with `count`
inputs:
  1. s(n) = fl(fl(a_i + a_j) + lw(n)) in fp32, this operand order (here: numpy float32 arithmetic on the fp32 activations
     the caller hands in -- the DEVICE's, when a device result is replayed);
  2. m = max_n s(n);
  3. m = -inf or NaN: the choice by the bare weights, the inverse CDF over exp(lw(n));
  4. otherwise e(n) = exp(s(n) - m) and the inverse CDF over e(n): the first n with u * total < c(n), the last input when
     there is none -- m, e(n) and the CDF in float64 here, where the kernel has fp32;
  5. u = the counter-based uniform of slot 1 (root), G + gl (region gl of a sum level with G regions), 2^depth + 2 f, + 1
     (the two uniforms of variable f's leaf), counter = row * (2^depth + 2 D) + slot.
Leaves: an observed variable keeps x[b, f]; a NaN variable is drawn from the chosen channel of its region (Box-Muller in
float64 / u1 < sigmoid(logit)).

Besides the samples it returns per row the MARGIN: the smallest distance, over the row's categorical draws, between u and a
step of the normalised float64 CDF.  A row whose margin is below what fp32 rounding of the kernel's CDF can move may
legitimately choose another input there; tests compare on the rows above a threshold.

A helper module (no tests in it)."""
import numpy as np
import torch

from oracle import ratspn_oracle as orc

#: the library's counter-based uniform (splitmix64 of seed + ctr * golden, its top 24 bits), float32
counter_uniform = orc.hash_uniform


def _choose(s32: np.ndarray, lw32: np.ndarray, u: np.ndarray):
    """s32, lw32 [M, count] float32 scores / log-weights, u [M] float32 -> (pick [M], margin [M])."""
    s = s32.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        m = np.max(s, axis=1)                                    # (np.max propagates NaN)
        live = m > -np.inf                                       # False for -inf and for NaN
        shift = np.where(live, m, 0.0)[:, None]
        e = np.where(live[:, None], np.exp(s - shift), np.exp(lw32.astype(np.float64)))
    cdf = np.cumsum(e, axis=1)
    cn = cdf / cdf[:, -1:]
    uu = u.astype(np.float64)[:, None]
    pick = np.minimum((cn <= uu).sum(axis=1), s.shape[1] - 1)
    margin = np.abs(cn - uu).min(axis=1)
    return pick, margin


def posterior_sample(acts, logws, src, leaf, x, y, seed: int):
    """acts: [leaf output [B, reps 2^depth, I], sum level 1 output [B, reps 2^(depth-1), S], ...] fp32 (a leading dimension
    of 1 stands for B identical rows); logws: log-softmax weights of the sum levels 1 .. depth-1, then of the root
    (RatSpn._topdown_logw()); src [reps, D] (RatSpn._topdown_src()); leaf = (dist, p0, p1) (RatSpn._leaf_params()); x [B, D]
    with NaN = to be drawn; y [B] integer labels or None (class 0); all host tensors / arrays.
    Returns (samples [B, D] float32, repetition [B], leaf channels [B, 2^depth], margin [B])."""
    f32 = lambda t: np.ascontiguousarray((t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)), dtype=np.float32)
    x = f32(x)
    B, D = x.shape
    acts = [np.broadcast_to(a, (B,) + a.shape[1:]) for a in map(f32, acts)]
    logws = [f32(w) for w in logws]
    src = (src.cpu().numpy() if torch.is_tensor(src) else np.asarray(src)).astype(np.int64)
    dist, p0, p1 = leaf
    p0 = f32(p0)
    depth = len(acts)
    reps = src.shape[0]
    G0 = 1 << depth
    d = p0.shape[2]
    ycls = np.zeros(B, np.int64) if y is None else (y.cpu().numpy() if torch.is_tensor(y) else np.asarray(y)).astype(np.int64)
    rows = np.arange(B)
    ctr0 = rows.astype(np.uint64) * np.uint64(G0 + 2 * D)

    # ---- root: one of the reps * N^2 inputs (partition = repetition, (i, j) = nodes of its two regions)
    A = acts[depth - 1]
    N = A.shape[2]
    NN = N * N
    A = A.reshape(B, reps, 2, N)
    s = (A[:, :, 0, :, None] + A[:, :, 1, None, :]).reshape(B, reps * NN) + logws[depth - 1][ycls]
    pick, margin = _choose(s, logws[depth - 1][ycls], counter_uniform(seed, ctr0 + np.uint64(1)))
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
        u = counter_uniform(seed, ctr0[:, None] + np.uint64(G) + np.arange(G, dtype=np.uint64)[None, :])
        pick, m = _choose(s.reshape(B * G, NN), lw.reshape(B * G, NN), u.reshape(B * G))
        margin = np.minimum(margin, m.reshape(B, G).min(axis=1))
        pick = pick.reshape(B, G)
        cur = np.stack([pick // N, pick % N], axis=2).reshape(B, 2 * G)

    # ---- leaves: every variable from the chosen channel of its region, in variable order
    sf = src[rep]                                                # [B, D]
    rl, j = sf // d, sf % d
    chan = cur[rows[:, None], rl]
    region = rep[:, None] * G0 + rl
    q0 = p0[region, chan, j].astype(np.float64)
    c = ctr0[:, None] + np.uint64(G0) + np.uint64(2) * np.arange(D, dtype=np.uint64)[None, :]
    u1 = counter_uniform(seed, c).astype(np.float64)
    if dist == 0:
        u2 = counter_uniform(seed, c + np.uint64(1)).astype(np.float64)
        z = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)
        v = q0 + f32(p1)[region, chan, j].astype(np.float64) * z
    else:
        v = (u1 < 1.0 / (1.0 + np.exp(-q0))).astype(np.float64)
    out = np.where(np.isnan(x), v.astype(np.float32), x)
    return torch.from_numpy(out), torch.from_numpy(rep), torch.from_numpy(cur), margin


def host_activations(sd, x, depth: int):
    """The activations posterior_sample wants, from the oracle's forward: leaf output, then every sum level's output."""
    _, acts = orc.ratspn_forward(sd, x, return_activations=True)
    return [acts['leaf']] + [acts['layer{}'.format(2 * t - 1)] for t in range(1, depth)]


# ---- the model small enough to enumerate (host test of the restatement, device test of the kernel) -----------------------
ENUM_KW = dict(in_features=6, rg_depth=2, rg_repetitions=2, rg_batch=2, rg_sum=2)
ENUM_ROWS = 200000
ENUM_SEED = 20240607


def enumerable_case():
    """(model on the host, evidence row [1, 6] with variables 1, 3, 4 missing, the 8 completions [8, 6], their posterior
    p(x) / sum p(x) in float64 from the oracle's forward)."""
    from deeprob.spn.models import BernoulliRatSpn
    torch.manual_seed(11)
    model = BernoulliRatSpn(random_state=3, **ENUM_KW).eval()
    with torch.no_grad():
        model.base_layer.logits.copy_(1.5 * torch.randn(model.base_layer.logits.shape, generator=torch.Generator().manual_seed(12)))
    row = torch.tensor([[1.0, float('nan'), 0.0, float('nan'), float('nan'), 1.0]])
    missing = [1, 3, 4]
    full = row.repeat(8, 1)
    for k in range(8):
        for bit, f in enumerate(missing):
            full[k, f] = float((k >> bit) & 1)
    sd64 = {k: (v.detach().double() if v.is_floating_point() else v.detach().clone()) for k, v in model.state_dict().items()}
    ll = orc.ratspn_forward(sd64, full.double())[:, 0]
    post = torch.softmax(ll, dim=0).numpy()
    return model, row, full, post


def completion_counts(samples: torch.Tensor, full: torch.Tensor) -> np.ndarray:
    """How often each row of `full` occurs among `samples` (every sample must be one of them)."""
    weights = (2 ** torch.arange(full.shape[1])).double()
    code = lambda t: (t.double() * weights).sum(dim=1).long()
    codes = code(full)
    got = code(samples.cpu())
    counts = np.array([(got == c).sum().item() for c in codes])
    assert counts.sum() == samples.shape[0], 'a sample is none of the enumerated completions'
    return counts
