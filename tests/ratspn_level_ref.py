"""Closed-form reference of one RAT-SPN level -- ProductLayer followed by a SumLayer or the RootLayer -- and of the bare
layers, in plain torch on the host: values, input gradient and weight gradient for a given incoming gradient g.

    prod[b,p,iN+j] = x[b,2p,i] + x[b,2p+1,j]                 (ProductLayer)
    lw  = log_softmax(w)   over the inputs of a sum node
    out = logsumexp(prod + lw)
    r   = exp(prod + lw - out)  where out > -inf, otherwise 0   (responsibilities)
    glw = sum_b g r ;  gW = glw - softmax(w) * sum_n glw      (log-softmax Jacobian)
    gprod = sum_s g r ;  gx[2p,i] = sum_j gprod ;  gx[2p+1,j] = sum_i gprod

This is what the HIP kernels evaluate (csrc/ratspn_level_bwd.hip, and sum_bwd_kernel / product_bwd_kernel of
csrc/ratspn_layers.hip).  On inputs without dead rows it is autograd through the oracle's layers
(tests/test_ratspn_level_backward_host.py); a sum node whose inputs are all -inf has out = -inf, and its gradient is DEFINED as
zero here and in the kernels -- torch's logsumexp backward gives NaN there (for the dead inputs and, summed over the batch,
for every weight of the node: the whole weight tensor of a root).

Evaluated in float64 this is the reference of tests/test_ratspn_level_backward_gpu.py; the same code evaluated in float32 is
the yardstick "how far float32 arithmetic of the plain formula is from float64".  The batch is walked in chunks, so that no
temporary exceeds a few tens of MB.  Also here: the inputs of the test cases (regimes), drawn in float32 from a seed.

A helper module (no tests in it)."""
import zlib

import torch

_CHUNK_ELEMS = 1 << 21      # elements of the [b, P, S, N] temporaries of a chunk (16 MB in float64)


def product_forward(x):
    """x [B, 2P, N] -> [B, P, N*N]."""
    B, R, N = x.shape
    return (x[:, 0::2, :, None] + x[:, 1::2, None, :]).reshape(B, R // 2, N * N)


def product_backward(gprod, N, dtype=torch.float64):
    """gprod [B, P, N*N] -> gx [B, 2P, N]: plain sums over j (child 2p) and over i (child 2p+1)."""
    gprod = gprod.to(dtype)
    B, P, _ = gprod.shape
    gp = gprod.reshape(B, P, N, N)
    gx = torch.empty((B, 2 * P, N), dtype=dtype)
    gx[:, 0::2] = gp.sum(dim=3)
    gx[:, 1::2] = gp.sum(dim=2)
    return gx


def sum_layer(xin, w, g, dtype=torch.float64):
    """A bare SumLayer: xin [B, P, N], w [P, S, N] raw weights, g [B, P, S] -> (out [B, P, S], gxin [B, P, N], gW [P, S, N])."""
    xin, w, g = xin.to(dtype), w.to(dtype), g.to(dtype)
    B, P, N = xin.shape
    S = w.shape[1]
    lw = torch.log_softmax(w, dim=2)
    out = torch.empty((B, P, S), dtype=dtype)
    gxin = torch.empty((B, P, N), dtype=dtype)
    glw = torch.zeros((P, S, N), dtype=dtype)
    step = max(1, _CHUNK_ELEMS // (P * S * N))
    for b0 in range(0, B, step):
        sl = slice(b0, min(B, b0 + step))
        t = xin[sl, :, None, :] + lw[None]                      # [b, P, S, N]
        o = torch.logsumexp(t, dim=3)
        live = (o > float('-inf'))[..., None]
        r = torch.where(live, torch.exp(t - torch.where(live, o[..., None], torch.zeros((), dtype=dtype))), torch.zeros((), dtype=dtype))
        gr = g[sl, :, :, None] * r
        out[sl] = o
        gxin[sl] = gr.sum(dim=2)
        glw += gr.sum(dim=0)
    gW = glw - torch.softmax(w, dim=2) * glw.sum(dim=2, keepdim=True)
    return out, gxin, gW


def root_layer(xin, w, g, dtype=torch.float64):
    """A bare RootLayer: xin [B, ...] (flattened to [B, M]), w [C, M], g [B, C] -> (out [B, C], gxin like xin, gW [C, M])."""
    B = xin.shape[0]
    out, gxin, gW = sum_layer(xin.reshape(B, 1, -1), w[None], g[:, None, :], dtype)
    return out[:, 0], gxin.reshape(xin.shape), gW[0]


def level(x, w, g, root, dtype=torch.float64):
    """One level: x [B, 2P, N]; w [P, S, N*N] (sum level) or [C, P*N*N] (root); g like the output.
    Returns (out, gx [B, 2P, N], gW like w) in `dtype`."""
    x = x.to(dtype)
    N = x.shape[2]
    prod = product_forward(x)
    out, gprod, gW = (root_layer if root else sum_layer)(prod, w, g, dtype)
    return out, product_backward(gprod, N, dtype), gW


# ---- inputs of the test cases ---------------------------------------------------------------------------------------------
REGIMES = ['plain', 'offset', 'two_live', 'dead']
OFFSETS = (-560.0, -1100.0, -1.0e4, 0.0)          # magnitudes of real leaf sums; cycling over the samples


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31)


def _two_live_weights(rows, n, free, period, gen):
    """[rows, n]: -200 everywhere except two entries per row, at 0 and -1, drawn from the columns m with m % period >= free."""
    allowed = torch.nonzero(torch.arange(n) % period >= free)[:, 0]
    w = torch.full((rows, n), -200.0)
    for r in range(rows):
        a, b = allowed[torch.randperm(allowed.numel(), generator=gen)[:2]].tolist()
        w[r, a], w[r, b] = 0.0, -1.0
    return w


def make_inputs(kind, P, N, S, B, regime):
    """float32 inputs (x, w, g) of a case.  kind 'sum' / 'root': a level, x [B, 2P, N]; 'sum_layer' / 'root_layer': a bare
    layer on x [B, P, N] (root_layer: P = 1, N = M inputs, S = C classes, w [C, M]).

    plain     x = randn 4, w = randn 2
    offset    per-sample constants so that the outputs sit near OFFSETS[b % 4]
    two_live  every weight -200 except two per softmax row (0 and -1); sample 0: inputs around -50 except one node at +60
              whose products all sit under -200 weights.  (Around: randn 4 - 50.  At exactly -50 the two live inputs of a
              node are equal, its responsibilities ARE softmax(w) and the sample's weight gradient is mathematically zero
              -- all there is at B = 1; no relative measure applies to that.)
    dead      sample 0: one whole region -inf; sample 1: node 0 of every region -inf; sample 2: everything at -1e4"""
    assert regime in REGIMES and kind in ('sum', 'root', 'sum_layer', 'root_layer')
    gen = torch.Generator().manual_seed(_seed(kind, P, N, S, B, regime))
    lvl = kind in ('sum', 'root')
    isroot = kind in ('root', 'root_layer')
    R = 2 * P if lvl else P
    n_in = N * N if lvl else N                       # inputs of a sum node per partition
    x = torch.randn(B, R, N, generator=gen) * 4
    if isroot:
        w = torch.randn(S, P * n_in, generator=gen) * 2
        g = torch.randn(B, S, generator=gen)
    else:
        w = torch.randn(P, S, n_in, generator=gen) * 2
        g = torch.randn(B, P, S, generator=gen)
    if regime == 'offset':
        off = torch.tensor(OFFSETS)[torch.arange(B) % len(OFFSETS)]
        x = x + (off / 2 if lvl else off)[:, None, None]
    elif regime == 'two_live':
        # the node at +60 is node 0 of (every even region of a level | every region of a bare layer): its products are the
        # first N (level: i = 0, every j) / the first (bare layer) inputs of each partition, kept under -200 weights
        free = N if lvl else 1
        if isroot:
            w = _two_live_weights(S, P * n_in, free, n_in, gen)
        else:
            w = _two_live_weights(P * S, n_in, free, n_in, gen).reshape(P, S, n_in)
        x[0] -= 50.0
        x[0, (slice(0, None, 2) if lvl else slice(None)), 0] = 60.0
    elif regime == 'dead':
        x[0, 0, :] = float('-inf')
        if B > 1:
            x[1, :, 0] = float('-inf')
        if B > 2:
            x[2] = -1.0e4
    return x.contiguous(), w.contiguous(), g.contiguous()


_cache = {}


def reference(kind, P, N, S, B, regime, shift=None):
    """(x, w, g, want, own) of a case, made once and left unchanged: the float32 inputs, the float64 results
    {'out', 'gx', 'gW'} as numpy arrays, and the distance of the float32 evaluation of the same formula from them
    (tests.util.rel_err for 'out', grad_err for the gradients).  shift: per-sample constants (cycled) added to x in float32
    BEFORE the reference sees it -- the training forward's relative tensors."""
    from tests.util import rel_err, grad_err
    key = (kind, P, N, S, B, regime, shift)
    if key in _cache:
        return _cache[key]
    x, w, g = make_inputs(kind, P, N, S, B, regime)
    if shift is not None:
        x = (x + torch.tensor(shift)[torch.arange(B) % len(shift)][:, None, None]).contiguous()
    fn = {'sum': lambda d: level(x, w, g, False, d), 'root': lambda d: level(x, w, g, True, d),
          'sum_layer': lambda d: sum_layer(x, w, g, d), 'root_layer': lambda d: root_layer(x, w, g, d)}[kind]
    want = dict(zip(('out', 'gx', 'gW'), (t.numpy() for t in fn(torch.float64))))
    w32 = dict(zip(('out', 'gx', 'gW'), (t.double().numpy() for t in fn(torch.float32))))
    own = {k: (rel_err if k == 'out' else grad_err)(w32[k], want[k]) for k in want}
    # a case whose gradient is mathematically zero (rounding noise in float64, other noise in float32) would admit anything
    # under the bar max(1e-4, 2 own): the inputs have to be drawn so that there is none
    assert own['gx'] < 2e-3 and own['gW'] < 2e-3, (key, own)
    for v in want.values():
        v.setflags(write=False)
    _cache[key] = (x, w, g, want, own)
    return _cache[key]


def dead_input_mask(x, kind):
    """bool like x: the inputs whose gradient is exactly 0 by the convention (or plainly, for the root, whose other partitions
    live: exp(-inf)) -- a region that is -inf in every node and, in a level, its sibling: all their products are -inf."""
    dead = (x == float('-inf')).all(dim=2)                       # [B, R]
    if kind in ('sum', 'root'):
        dead = (dead[:, 0::2] | dead[:, 1::2]).repeat_interleave(2, dim=1)
    return dead[:, :, None].expand_as(x).clone()
