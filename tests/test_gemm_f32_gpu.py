"""The fp32-MFMA GEMM of the training routes (csrc/coupling_bwd.hip: gemm_f32_kernel / launch_gemm) past one tile, in
isolation: MaskedLinear reaches three of its four operand orientations with nothing but a 0/1 mask and a bias around
them,

    forward   y      = x (W o M)^T + b     A k-fast, B k-fast     M = B,   N = out, K = in
    grad_x    gy (W o M)                   A k-fast, B n-fast     M = B,   N = in,  K = out
    grad_W    M o (gy^T x)                 A m-fast, B n-fast     M = out, N = in,  K = B

(grad_b is maf_colsum_kernel).  The shapes are the smallest at which each mechanism of launch_gemm engages -- `plan`
below restates its decision, `test_shapes_engage_what_they_are_chosen_for` pins the table -- and every shape gets

  * integer data (-4 .. 4): every partial sum is an integer far below 2^24, so the fp32 result is exact in ANY summation
    order (MFMA, partial tiles, slice sums, atomics) and is compared with np.array_equal: one dropped, doubled or
    misplaced term fails;
  * Gaussian data against float64 under the componentwise forward-error bound of an fp32 dot product of length K;
  * three calls on the same inputs, bit-identical (the slice-order sums of the ticketed split-K are deterministic).

The atomicAdd fallback of the split-K (taken when the per-device pool cannot be allocated: the first split product of a
process issued inside a stream capture) runs in a child process: tests/_gemm_graph_case.py.

No test asserts which route ran: they assert results at shapes where the code, as written, takes it."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
EPS = 2.0 ** -24          # unit roundoff of fp32

# (B, in_features, out_features)
SHAPES = [(130, 200, 70), (257, 129, 65), (63, 127, 191), (64, 128, 64), (64, 127, 64), (5, 640, 3), (129, 65, 1568),
          (1000, 520, 100), (15, 13, 9)]
LEADING = {(63, 127, 191): (3, 21), (15, 13, 9): (3, 5)}       # x of shape [3, B / 3, in]: leading batch dimensions


def _cdiv(a, b):
    return -(-a // b)


def plan(M, N, K, cus=256):
    """launch_gemm's decision restated: (tiles, slices, K per slice, width of the last slice).  64 x 64 tiles; K is split
    when K >= 128 and the tiles fill less than 3/4 of the compute units, into min(ceil(cus / tiles), ceil(K / 64), 8)
    slices of a whole number of 64-wide slabs."""
    tiles = _cdiv(N, 64) * _cdiv(M, 64)
    ksplit, kchunk = 1, K
    if tiles < cus // 2 + cus // 4 and K >= 128:
        ksplit = min(_cdiv(cus, tiles), _cdiv(K, 64), 8)
    if ksplit > 1:
        kchunk = _cdiv(_cdiv(K, ksplit), 64) * 64
        ksplit = _cdiv(K, kchunk)
    return tiles, ksplit, kchunk, K - (ksplit - 1) * kchunk


def products(shape):
    B, fin, fout = shape
    return dict(forward=(B, fout, fin), grad_x=(B, fin, fout), grad_W=(fout, fin, B))


def test_shapes_engage_what_they_are_chosen_for():
    """The table the shapes were chosen by (256 compute units), so that the choice can be re-derived; pure arithmetic.
    Products of at most 15 tiles split on any device with >= 32 compute units."""
    def p(shape, which, cus=256):
        return plan(*products(shape)[which], cus=cus)
    assert p((130, 200, 70), 'forward') == (6, 4, 64, 8)
    assert p((130, 200, 70), 'grad_W') == (8, 3, 64, 2)
    assert p((130, 200, 70), 'grad_x')[:2] == (12, 1)
    assert p((257, 129, 65), 'forward')[1:] == (3, 64, 1)
    assert p((257, 129, 65), 'grad_W')[1:] == (5, 64, 1)
    assert p((257, 129, 65), 'grad_x')[:2] == (15, 1)
    assert p((63, 127, 191), 'grad_x')[:2] == (2, 3)
    assert p((64, 128, 64), 'forward') == (1, 2, 64, 64)
    assert p((64, 127, 64), 'forward')[:2] == (1, 1)
    assert p((5, 640, 3), 'forward') == (1, 5, 128, 128)
    assert p((129, 65, 1568), 'grad_x') == (6, 7, 256, 32)
    assert p((129, 65, 1568), 'forward')[:2] == (75, 1)
    assert p((129, 65, 1568), 'grad_W')[:2] == (50, 3)
    assert p((1000, 520, 100), 'grad_W')[:2] == (18, 8)
    assert p((1000, 520, 100), 'forward')[:2] == (32, 5)
    assert all(plan(*mnk)[1] == 1 for mnk in products((15, 13, 9)).values())
    for shape in SHAPES:
        for mnk in products(shape).values():
            if plan(*mnk)[0] <= 15 and plan(*mnk)[1] > 1:
                assert plan(*mnk, cus=32)[1] > 1, (shape, mnk)


@functools.lru_cache(maxsize=None)
def _data(shape, kind):
    """Inputs of one shape (CPU, read-only, made once): integers -4 .. 4 or Gaussians, and a random 0/1 mask."""
    B, fin, fout = shape
    rs = np.random.RandomState(1000 * B + 10 * fin + fout + (0 if kind == 'int' else 1))
    if kind == 'int':
        draw = lambda *s: rs.randint(-4, 5, size=s).astype(np.float32)
    else:
        draw = lambda *s: rs.standard_normal(size=s).astype(np.float32)
    out = dict(x=draw(B, fin), W=draw(fout, fin), b=draw(fout), gy=draw(B, fout), mask=rs.rand(fout, fin) < 0.5)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(shape, kind, bias):
    """The products in int64 (integer data: exact) or float64, and for the float data the magnitudes |A| |B| the
    forward-error bound is made of."""
    d = _data(shape, kind)
    t = np.int64 if kind == 'int' else np.float64
    x, gy, b = d['x'].astype(t), d['gy'].astype(t), d['b'].astype(t)
    wm = d['W'].astype(t) * d['mask'].astype(t)
    out = dict(y=x @ wm.T + (b if bias else 0), gx=gy @ wm, gW=(gy.T @ x) * d['mask'].astype(t), gb=gy.sum(0))
    if kind != 'int':
        out.update(y_mag=np.abs(x) @ np.abs(wm).T, gx_mag=np.abs(gy) @ np.abs(wm), gW_mag=(np.abs(gy).T @ np.abs(x)) * d['mask'],
                   gb_mag=np.abs(gy).sum(0), b_mag=np.abs(b) if bias else 0.0)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _layer(shape, kind, bias):
    from deeprob.torch.utils import MaskedLinear
    B, fin, fout = shape
    d = _data(shape, kind)
    lin = MaskedLinear(fin, fout, d['mask'])
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(d['W']))
        lin.bias.copy_(torch.from_numpy(d['b']))
    if not bias:
        lin.bias = None
    return lin.to(DEV)


def _run(lin, shape, kind):
    """One forward and backward on the device: y, grad_x, grad_W, grad_b (None without a bias) as CPU tensors."""
    B, fin, fout = shape
    d = _data(shape, kind)
    lead = LEADING.get(shape, (B,))
    x = torch.from_numpy(d['x']).reshape(*lead, fin).to(DEV).requires_grad_(True)
    gy = torch.from_numpy(d['gy']).reshape(*lead, fout).to(DEV)
    lin.zero_grad(set_to_none=True)
    y = lin(x)
    assert tuple(y.shape) == (*lead, fout)
    y.backward(gy)
    gb = lin.bias.grad.cpu() if lin.bias is not None else None
    return y.detach().cpu().reshape(B, fout), x.grad.cpu().reshape(B, fin), lin.weight.grad.cpu(), gb


@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_integer_data_is_exact(shape, bias):
    """No tolerance: operands are integers in -4 .. 4, |sum| <= 16 K <= 25088 < 2^24, so fp32 is exact in any order."""
    want = _want(shape, 'int', bias)
    y, gx, gW, gb = _run(_layer(shape, 'int', bias), shape, 'int')
    mask = _data(shape, 'int')['mask']
    for name, got, ref in (('y', y, want['y']), ('grad_x', gx, want['gx']), ('grad_W', gW, want['gW'])) + \
            ((('grad_b', gb, want['gb']),) if bias else ()):
        got = got.numpy().astype(np.float64)
        bad = np.argwhere(got != ref)                       # (a NaN differs from everything)
        assert np.array_equal(got, ref), '{} of {}: {} wrong elements, the first at {} (got {}, want {})'.format(
            name, shape, len(bad), bad[:1].tolist(), got[tuple(bad[0])] if len(bad) else None,
            ref[tuple(bad[0])] if len(bad) else None)
    assert np.all(gW.numpy()[~mask] == 0)


@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_gaussian_data_within_the_fp32_dot_product_bound(shape, bias):
    """|got - want| <= (K + 16) 2^-24 (|A| |B|) + 2 2^-24 |bias|, componentwise: the standard forward-error bound of an fp32
    dot product of length K in any order (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), the 16
    covering the at most 8 slice additions and the epilogue.  It is made of the operands, not of the kernel's result:
    numpy's own fp32 product sits at <= 0.03 of it for these shapes, a single dropped k-term exceeds it in >= 94 % of
    the entries.  grad_b: (B + 4) 2^-24 sum |gy|."""
    B, fin, fout = shape
    want = _want(shape, 'float', bias)
    y, gx, gW, gb = _run(_layer(shape, 'float', bias), shape, 'float')
    mask = _data(shape, 'float')['mask']
    checks = [('y', y, want['y'], (fin + 16) * EPS * want['y_mag'] + 2 * EPS * want['b_mag']),
              ('grad_x', gx, want['gx'], (fout + 16) * EPS * want['gx_mag']),
              ('grad_W', gW, want['gW'], (B + 16) * EPS * want['gW_mag'])]
    if bias:
        checks.append(('grad_b', gb, want['gb'], (B + 4) * EPS * want['gb_mag']))
    for name, got, ref, bound in checks:
        got = got.numpy().astype(np.float64)
        assert np.isfinite(got).all(), name
        err = np.abs(got - ref)
        over = np.argwhere(err > bound)
        worst = float(np.max(err / np.maximum(bound, 1e-300)))
        print('{} {} bias={}: worst |err| / bound = {:.3f}'.format(name, shape, bias, worst))
        assert not len(over), '{} of {}: {} elements above the bound, the first at {}, worst err / bound {:.3g}'.format(
            name, shape, len(over), over[:1].tolist(), worst)
    assert np.all(gW.numpy()[~mask] == 0)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_three_calls_are_bit_identical(shape):
    """The ticketed split-K adds the partial tiles in slice order whichever slice arrives last: forward and backward
    three times on the same inputs give the same bits (three calls, not a stress loop)."""
    lin = _layer(shape, 'float', True)
    first = _run(lin, shape, 'float')
    for _ in range(2):
        again = _run(lin, shape, 'float')
        for name, a, b in zip(('y', 'grad_x', 'grad_W'), first, again):
            assert torch.equal(a, b), '{} of {} differs between calls at {} elements'.format(name, shape, int((a != b).sum()))


def test_split_k_fallback_inside_a_graph_capture():
    """The atomicAdd fallback of the split-K: a process whose FIRST library call is a MaskedLinear forward and backward
    (130, 200, 70) captured into a graph cannot allocate the pool of partial tiles inside the capture; the zeroing of C
    and the epilogue are then captured launches of their own.  Integer data, two replays with fresh values copied
    into the static tensors and no synchronisation in between, as a training loop replays: both exact -- the second
    proves the zeroing is part of the graph.  (It was a hipMemsetAsync at first: as a captured memset node it left
    every fourth element of y, flat index 2 mod 4, with a stale fill pattern on the second replay; launch_gemm now
    zeroes C with a kernel.)  A fresh child process (tests/_gemm_graph_case.py), since the pool exists in this one as
    soon as any other test has run."""
    from tests import _gemm_graph_case as gc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, 'deeprob-kit_amd'), root,
                                                       os.environ.get('PYTHONPATH', '')]))
    r = subprocess.run([sys.executable, '-X', 'faulthandler', '-m', 'tests._gemm_graph_case'], cwd=root, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    out, err = r.stdout.decode(errors='replace'), r.stderr.decode(errors='replace')
    lines = [l for l in out.splitlines() if l.startswith(gc.MARK)]
    assert r.returncode == 0 and len(lines) == gc.REPLAYS, 'child failed (rc {}):\n{}\n{}'.format(
        r.returncode, out[-2000:], err[-4000:])
    for replay, line in enumerate(lines):
        got = json.loads(line[len(gc.MARK):])
        d = gc.inputs(replay)
        x, gy, b = (d[k].astype(np.int64) for k in ('x', 'gy', 'b'))
        wm = d['W'].astype(np.int64) * d['mask'].astype(np.int64)
        want = dict(y=x @ wm.T + b, gx=gy @ wm, gW=(gy.T @ x) * d['mask'].astype(np.int64), gb=gy.sum(0))
        for k, ref in want.items():
            g = np.asarray(got[k], dtype=np.float64).reshape(ref.shape)
            bad = np.argwhere(g != ref)
            assert np.array_equal(g, ref.astype(np.float64)), 'replay {}: {} has {} wrong elements, the first at {}'.format(
                replay, k, len(bad), bad[:1].tolist())
        assert np.all(np.asarray(got['gW'], dtype=np.float64).reshape(d['mask'].shape)[~d['mask']] == 0)
