"""The Gaussian RAT-SPN training backward, level by level, against the float64 closed form of tests/ratspn_level_ref.py (pinned
on the host by tests/test_ratspn_level_backward_host.py): every instantiation of csrc/ratspn_level_bwd.hip and the per-layer
chain of csrc/ratspn_layers.hip (product_bwd_kernel, lse_residual_kernel, sum_bwd_kernel, the two Jacobian kernels), at the
smallest shapes at which each of their code paths exists, under four input regimes (ratspn_level_ref.make_inputs).

Routes of a level: (a) ops.prodsum_autograd with the single-launch level kernel -- that it IS that kernel is read off the C
ABI's return code, not restated from the envelope; (b) the same with ops._LEVEL_BACKWARD off: the recompute chain of
ops._prodsum_backward; (c) ProductFn chained into SumFn / RootFn.

Bars (the project's, none derived from the code under test): forward values 1e-5 relative (LL_TOL), -inf exactly where the
reference has it; gradients max(1e-4, 2 x the distance of the float32 evaluation of the reference from float64) of the tensor's
largest magnitude -- the rule of test_ratspn_gpu.py::test_backward_golden.  Every measured error goes to the measured-errors
report next to the float32 reference's own distance.  No bit-identity: the weight gradients go through float atomics."""
import numpy as np
import pytest
import torch

from tests import ratspn_level_ref as ref
from tests.util import rel_err, grad_err, report_measured

pytestmark = pytest.mark.gpu

LL_TOL = 1e-5     # north-star: 1e-5 relative on fp32 log-likelihoods
GRAD_TOL = 1e-4   # relative to the largest magnitude of the tensor
DPK_OK = 0


def _cdiv(a, b):
    return (a + b - 1) // b


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def sum_level_tile(B, P):
    """dpk_prodsum_backward's sample tile of a sum level with 2 / 4 / 8 nodes: 256, halved down to 8 while the grid would
    leave compute units idle."""
    tile = 256
    while tile > 8 and _cdiv(B, tile) * P < 2 * _cus():
        tile //= 2
    return tile


def root_level_passes(B):
    """dpk_prodsum_backward's passes (of four samples) per work-group of the root level."""
    return min(64, max(1, B // (4 * 2 * _cus())))


class Held:
    """Measures every tensor of a case against the reference, reports it, and fails at the end with all that missed."""

    def __init__(self, test, case, want, own):
        self.test, self.case, self.want, self.own, self.missed = test, case, want, own, []

    def __call__(self, route, name, got):
        want, own = self.want[name], self.own[name]
        got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
        if name == 'out':
            err, tol = rel_err(got, want), LL_TOL
        else:
            assert np.isfinite(got).all(), (self.case, route, name, 'non-finite gradient')
            err, tol = grad_err(got, want), max(GRAD_TOL, 2.0 * own)
        report_measured('%s[%s] %s %s vs fp64' % (self.test, self.case, route, name), err, tol, '(reference fp32 vs fp64 = %.2e)' % own)
        if not err <= tol:
            self.missed.append('%s %s: %.3e > %.3e' % (route, name, err, tol))

    def zero_where(self, route, got, mask):
        if mask.any() and not (got.detach().cpu()[mask] == 0.0).all():
            self.missed.append('%s gx: dead inputs not exactly 0' % route)

    def done(self):
        assert not self.missed, (self.case, self.missed)


def level_kernel_rc(x, w, out, g, root):
    """dpk_prodsum_backward called the way ops._prodsum_backward calls it: (return code, gx, gW)."""
    from deeprob.hip import load_library, ptr, stream_ptr, ops, Workspace
    lib = load_library()
    B, R, N = x.shape
    S = w.shape[0] if root else w.shape[1]
    gx, gw = torch.empty_like(x), torch.empty_like(w)
    buf = ops._sum_ws(Workspace(), 0, R // 2, N * N, S, x.device)
    rc = lib.dpk_prodsum_backward(ptr(x), ptr(w), ptr(out), ptr(g), B, R, N, S, int(root), ptr(gx), ptr(gw), ptr(buf),
                                  buf.numel(), stream_ptr(x.device))
    torch.cuda.synchronize()
    return rc, gx, gw


def run_level(monkeypatch, test, kind, P, N, S, B, regime, in_envelope):
    from deeprob.hip import ops, Workspace, DPK_EUNSUPPORTED
    root = kind == 'root'
    x, w, g, want, own = ref.reference(kind, P, N, S, B, regime)
    held = Held(test, '%s-P%d-N%d-S%d-B%d-%s' % (kind, P, N, S, B, regime), want, own)
    dead = ref.dead_input_mask(x, kind)
    xd, wd, gd = x.cuda(), w.cuda(), g.cuda()

    def autograd(route, fn):
        xa, wa = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True)
        out = fn(xa, wa)
        gx, gw = torch.autograd.grad(out, [xa, wa], gd)
        held(route, 'out', out)
        held(route, 'gx', gx)
        held(route, 'gW', gw)
        held.zero_where(route, gx, dead)
        return out.detach()

    def folded(xa, wa):
        out = ops.prodsum_autograd(xa, wa, Workspace(), root=root)
        assert out is not None
        return out

    # (c) the layers chained
    out_c = autograd('layers', lambda xa, wa: (ops.RootFn if root else ops.SumFn).apply(ops.ProductFn.apply(xa), wa, Workspace()))
    # (a) the level kernel: the C ABI says whether it took the shape
    rc, kx, kw = level_kernel_rc(xd, wd, out_c, gd, root)
    assert rc == (DPK_OK if in_envelope else DPK_EUNSUPPORTED), (held.case, rc)
    if in_envelope:
        held('level-abi', 'gx', kx)
        held('level-abi', 'gW', kw)
    assert ops._LEVEL_BACKWARD[0] is True
    autograd('level' if in_envelope else 'level->chain', folded)
    # (b) the recompute chain of ops._prodsum_backward
    with monkeypatch.context() as m:
        m.setattr(ops, '_LEVEL_BACKWARD', [False])           # (a list has no .get: monkeypatch.setitem does not take it)
        autograd('recompute', folded)
    assert ops._LEVEL_BACKWARD[0] is True
    held.done()


# ---- sum levels: every instantiation; B = 37 leaves ragged sample slots in the UN = 2 unroll for every N and a ragged last
# trip of the 16-node kernel's two-samples-at-a-time walk; B = 1 leaves every slot but one empty ------------------------------
SUM_LEVELS = [(N, S) for N in (2, 4, 8) for S in (2, 4, 8)] + [(16, 8), (16, 16)]


@pytest.mark.parametrize('regime', ref.REGIMES)
@pytest.mark.parametrize('B', [1, 37])
@pytest.mark.parametrize('N,S', SUM_LEVELS)
def test_sum_level_every_instantiation(monkeypatch, N, S, B, regime):
    run_level(monkeypatch, 'test_sum_level_every_instantiation', 'sum', 3, N, S, B, regime, True)


@pytest.mark.parametrize('regime', ref.REGIMES)
@pytest.mark.parametrize('end', ['tile256', 'tile8'])
def test_sum_level_host_tile_choice_at_both_ends(monkeypatch, end, regime):
    """The longest tile (as many partitions as compute units, two tiles of samples: the grid covers the chip twice at 256)
    and the shortest (one partition, nine samples)."""
    P, N, S, B = (_cus(), 2, 2, 300) if end == 'tile256' else (1, 4, 4, 9)
    assert sum_level_tile(B, P) == (256 if end == 'tile256' else 8)
    run_level(monkeypatch, 'test_sum_level_host_tile_choice_at_both_ends', 'sum', P, N, S, B, regime, True)


# ---- the root level: M = P N^2 threads -- 1024 (the limit: sixteen waves), 80 (idle lanes in the second wave), 12; classes in
# one chunk kept in registers (1, 8) or two / three chunks with a ragged last one through atomics (9, 20); B = 7: a ragged
# last group of four samples ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', ref.REGIMES)
@pytest.mark.parametrize('B', [1, 7])
@pytest.mark.parametrize('C', [1, 8, 9, 20])
@pytest.mark.parametrize('N,P', [(8, 16), (4, 5), (2, 3)])
def test_root_level_every_instantiation(monkeypatch, N, P, C, B, regime):
    assert root_level_passes(B) == 1
    run_level(monkeypatch, 'test_root_level_every_instantiation', 'root', P, N, C, B, regime, True)


@pytest.mark.parametrize('regime', ref.REGIMES)
def test_root_level_two_passes_through_atomics(monkeypatch, regime):
    """More than 8 classes and two passes per work-group: the weight gradient of every pass and chunk goes through atomics."""
    B = 8 * _cus() * 2 + 3
    assert root_level_passes(B) == 2
    run_level(monkeypatch, 'test_root_level_two_passes_through_atomics', 'root', 4, 2, 9, B, regime, True)


@pytest.mark.parametrize('regime', ref.REGIMES)
@pytest.mark.parametrize('N,P', [(8, 17), (16, 2)])
def test_root_level_outside_the_kernel_falls_to_the_chain(monkeypatch, N, P, regime):
    """M = 1088 > 1024 threads, and 16 nodes: DPK_EUNSUPPORTED, and still correct through the chain."""
    run_level(monkeypatch, 'test_root_level_outside_the_kernel_falls_to_the_chain', 'root', P, N, 3, 7, regime, False)


# ---- the bare layers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', ref.REGIMES)
@pytest.mark.parametrize('kind,P,N,S,B', [
    ('sum_layer', 3, 9, 5, 37),         # thread-per-row residual, columns not a multiple of 64
    ('sum_layer', 2, 64, 33, 13),       # wave-per-row residual; three output blocks of 16: gx is read back and added to twice
    ('sum_layer', 5, 25, 17, 70),
    ('root_layer', 1, 2048, 3, 9),      # root_wide_kernel forward, logsoftmax_jacobian_wide_kernel
    ('root_layer', 1, 1024, 1, 5)])
def test_bare_sum_and_root_backward(kind, P, N, S, B, regime):
    from deeprob.hip import ops, Workspace
    x, w, g, want, own = ref.reference(kind, P, N, S, B, regime)
    held = Held('test_bare_sum_and_root_backward', '%s-P%d-N%d-S%d-B%d-%s' % (kind, P, N, S, B, regime), want, own)
    xa, wa = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    out = (ops.RootFn if kind == 'root_layer' else ops.SumFn).apply(xa, wa, Workspace())
    gx, gw = torch.autograd.grad(out, [xa, wa], g.cuda())
    held('layer', 'out', out)
    held('layer', 'gx', gx)
    held('layer', 'gW', gw)
    held.zero_where('layer', gx, ref.dead_input_mask(x, kind))
    held.done()


@pytest.mark.parametrize('spread', ['plain', 'wide'])
@pytest.mark.parametrize('N', [3, 5, 32])
def test_bare_product_backward(N, spread):
    """product_bwd_kernel sees the incoming gradient only (the regimes of x and w do not reach it): unit-scale terms, and
    terms spread over six decades within a row.  A sum of at most 32 float32 terms: 1e-6 of the largest magnitude."""
    from deeprob.hip import ops
    gen = torch.Generator().manual_seed(N)
    gp = torch.randn(5, 3, N * N, generator=gen)
    if spread == 'wide':
        gp = gp * 10.0 ** torch.randint(-3, 4, gp.shape, generator=gen).float()
    want = ref.product_backward(gp, N).numpy()
    xa = torch.zeros(5, 6, N, device='cuda', requires_grad=True)
    got, = torch.autograd.grad(ops.ProductFn.apply(xa), [xa], gp.cuda())
    err = grad_err(got.cpu().numpy(), want)
    report_measured('test_bare_product_backward[N%d-%s] gx vs fp64' % (N, spread), err, 1e-6,
                    '(reference fp32 vs fp64 = %.2e)' % grad_err(ref.product_backward(gp, N, torch.float32).double().numpy(), want))
    assert err <= 1e-6


# ---- what dpk_ratspn_forward_train hands the backward: tensors relative to a per-sample constant ------------------------------
@pytest.mark.parametrize('regime', ref.REGIMES)
@pytest.mark.parametrize('kind,P,N,S,B', [('sum', 3, 8, 8, 37), ('root', 8, 8, 1, 7)])
def test_direct_call_with_relative_tensors(monkeypatch, kind, P, N, S, B, regime):
    """ops._prodsum_backward on (x + c_b, out of those shifted inputs): no HIP forward involved -- `out` is the float64
    reference's, rounded to float32.  The kernels only use in - out, and the reference is shift-invariant: same bars."""
    from deeprob.hip import ops, Workspace
    root = kind == 'root'
    x, w, g, want, own = ref.reference(kind, P, N, S, B, regime, shift=(-1024.0, 512.0))
    held = Held('test_direct_call_with_relative_tensors', '%s-P%d-N%d-S%d-B%d-%s' % (kind, P, N, S, B, regime), want, own)
    dead = ref.dead_input_mask(x, kind)
    xd, wd, gd = x.cuda(), w.cuda(), g.cuda()
    out = torch.tensor(want['out'], dtype=torch.float32).cuda()
    rc, _, _ = level_kernel_rc(xd, wd, out, gd, root)
    assert rc == DPK_OK
    for route, on in (('level', True), ('recompute', False)):
        with monkeypatch.context() as m:
            m.setattr(ops, '_LEVEL_BACKWARD', [on])
            gx, gw = ops._prodsum_backward(xd, wd, out, gd, Workspace(), root, True, True)
        held(route, 'gx', gx)
        held(route, 'gW', gw)
        held.zero_where(route, gx, dead)
    held.done()
