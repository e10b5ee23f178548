"""The MAF kernels (csrc/maf.hip, deeprob/hip/ops_maf.py) across the envelope they advertise, against the float64
restatement of tests/maf_cases.py: every template instance and launch configuration of the fused density kernel, the
sampling kernel and the deep sampling kernel, and the backward formulas of all five activations.

Bars (the ones tests/test_maf_gpu.py uses): rel_err <= 1e-5 on u / ildj / MaskedLinear outputs, rel_err <= 1e-4
on sampled x / ldj, grad_err <= 1e-4 on gradients, each against float64 -- never against another route of the code under
test (fused-versus-chain agreement is asserted on top).  Every measured error is recorded with report_measured under its
group letter (A fused density, B sampling, C deep sampling, D backward)."""
import contextlib

import numpy as np
import pytest
import torch

from tests.util import rel_err, grad_err, report_measured
from tests import maf_cases as mc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
U_BAR, X_BAR, G_BAR = 1e-5, 1e-4, 1e-4
ALL_ACTS = ['relu', 'leaky-relu', 'softplus', 'tanh', 'sigmoid']


def _layer(D, units, depth=1, act='relu', seed=0, mode='seq', scale=0.3):
    """A seeded AutoregressiveLayer on the device: sequential ('seq'), reversed ('rev') or random ('random') degrees,
    nn.Linear's initial draws plus scale * N(0, 1 / fan_in) on every masked weight, ScaledTanh weight 0.5."""
    from deeprob.flows.layers.autoregressive import AutoregressiveLayer
    torch.manual_seed(seed)
    layer = AutoregressiveLayer(D, depth, units, act, reverse=mode == 'rev', sequential=mode != 'random',
                                random_state=np.random.RandomState(seed))
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        layer.scale_act.weight.fill_(0.5)
        for m in mc.masked_linears(layer):
            m.weight.add_(scale * torch.randn(m.weight.shape, generator=g) / np.sqrt(m.weight.shape[1]))
    return layer.to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


class _Checks:
    """Measures every (got, want) pair, records it, and fails at the end with all the pairs that missed their bar."""

    def __init__(self, group, case):
        self.group, self.case, self.failed = group, case, []

    def __call__(self, name, got, want, bar, grad=False):
        err = (grad_err if grad else rel_err)(_np(got) if torch.is_tensor(got) else got,
                                              _np(want) if torch.is_tensor(want) else want)
        report_measured('%s %s %s' % (self.group, self.case, name), err, bar)
        if not err <= bar:
            self.failed.append((name, err, bar))

    def done(self):
        assert not self.failed, (self.case, self.failed)


@contextlib.contextmanager
def _counting(entry, step_loop=False):
    """The calls ops_maf makes to one entry point of the C ABI, counted; the step loop is taken away unless wanted."""
    from deeprob.hip import ops_maf, load_library
    lib = load_library()
    real = getattr(lib, entry)
    calls = []

    def counted(*a):
        calls.append(1)
        return real(*a)
    counted.__name__ = entry

    class Counting:
        def __getattr__(self, name):
            return counted if name == entry else getattr(lib, name)
    loop = ops_maf.step_loop
    if not step_loop:
        ops_maf.step_loop = None
    ops_maf.load_library = lambda: Counting()
    try:
        yield calls
    finally:
        ops_maf.step_loop = loop
        ops_maf.load_library = load_library


# ---- A. fused density kernel ------------------------------------------------------------------------------------------
def _density64(layer, act, x, affine=None, acc=None):
    """(u, ildj) of apply_backward in float64 numpy, an eval-mode batch norm (scale, shift) folded in front and the
    log-det added to `acc` when given."""
    D = x.shape[1]
    xa = _np(x).astype(np.float64)
    if affine is not None:
        xa = xa * _np(affine[0]).astype(np.float64) + _np(affine[1]).astype(np.float64)
    wm, a = mc.layer_params(layer)
    z = mc.conditioner64(wm, act, xa)
    s = a * np.tanh(z[:, D:])
    ildj = -s.sum(1)
    if acc is not None:
        ildj = ildj + _np(acc).astype(np.float64)
    return (xa - z[:, :D]) * np.exp(-s), ildj


def _density_inputs(B, D, seed, affine):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g).to(DEV)
    if not affine:
        return x, None, None
    sc, sh = (torch.rand(D, generator=g) + 0.5).to(DEV), torch.randn(D, generator=g).to(DEV)
    return x, (sc, sh), torch.randn(B, generator=g).to(DEV)


# (D, units, degrees, activation, B, folded batch norm + accumulated ildj).  Units 129 .. 256: two hidden tiles per wave
# (NHT = 2) with HT = 5 (129, 160 units) and 8 (225, 256 units: UP = 256, 66 816 bytes of dynamic LDS, above the 64 KB
# a kernel gets unasked); D = 150 / 70 / 33 / 2: 3 / 2 / 1 / 1 chunks of 64 inputs and 5 / 3 / 2 / 1 output tiles over 4 waves.
FUSED_CASES = [
    (150, 160, 'random', 'softplus', 130, False),
    (150, 160, 'random', 'tanh', 65, True),
    (150, 256, 'seq', 'sigmoid', 130, True),
    (150, 256, 'seq', 'relu', 1, False),
    (70, 225, 'rev', 'leaky-relu', 64, False),
    (70, 225, 'rev', 'softplus', 65, True),
    (33, 129, 'seq', 'tanh', 1, False),
    (33, 129, 'random', 'leaky-relu', 130, True),
    (2, 256, 'seq', 'sigmoid', 64, False),
    (2, 256, 'rev', 'relu', 65, True),
]


@pytest.mark.parametrize('D,units,mode,act,B,affine', FUSED_CASES)
def test_fused_density_two_tiles_per_wave_vs_float64(D, units, mode, act, B, affine):
    from deeprob.hip import ops_maf
    assert 128 < units <= ops_maf.FUSED_MAX_UNITS
    layer = _layer(D, units, act=act, seed=D + units, mode=mode)
    assert ops_maf.fused_envelope(layer, D)
    x, aff, acc = _density_inputs(B, D, 7 * D + B, affine)
    with torch.no_grad():
        u, ildj = ops_maf.density_fused(x, layer, in_affine=aff, ildj=None if acc is None else acc.clone())
    want_u, want_ildj = _density64(layer, act, x, aff, acc)
    assert tuple(u.shape) == (B, D) and tuple(ildj.shape) == (B,)
    check = _Checks('A', 'fused[D %d, %d units, %s, %s, B %d%s]' % (D, units, mode, act, B, ', affine' if affine else ''))
    check('u', u, want_u, U_BAR)
    check('ildj', ildj, want_ildj, U_BAR)
    check.done()


def _arbitrary_masks(D, units, seed, zero_hidden, zero_outputs):
    """Bernoulli(0.5) masks of a depth-1 conditioner (translation and scale rows drawn separately): their non-zeros form
    no prefix in any packed order.  zero_hidden empties 40 rows of M1 (more than one 32-row tile once sorted by fan-in),
    zero_outputs empties the translation AND the scale row of M2 for 35 outputs."""
    rs = np.random.RandomState(seed)
    m1, m2 = rs.rand(units, D) < 0.5, rs.rand(2 * D, units) < 0.5
    if zero_hidden:
        m1[rs.choice(units, 40, replace=False)] = False
    if zero_outputs:
        outs = rs.choice(D, 35, replace=False)
        m2[outs] = False
        m2[outs + D] = False
    return m1, m2


@pytest.mark.parametrize('variant', ['bernoulli', 'zero-hidden-rows', 'zero-outputs', 'data-write'])
@pytest.mark.parametrize('D,units,act', [(77, 100, 'softplus'), (150, 160, 'leaky-relu')])
def test_fused_density_arbitrary_masks_vs_float64(D, units, act, variant):
    """The per-tile K extents come from the live masks: any mask gives the float64 numbers, whatever the packing order --
    one derived from the mask (first three variants) or one gone stale (the mask rewritten through `.data` after a first
    call, which leaves the (address, version) key of the cached order unchanged)."""
    from deeprob.hip import ops_maf
    layer = _layer(D, units, act=act, seed=3, mode='seq')
    x, _, _ = _density_inputs(130, D, 5, False)
    m1, m2 = _arbitrary_masks(D, units, 17, variant in ('zero-hidden-rows', 'data-write'),
                              variant in ('zero-outputs', 'data-write'))
    with torch.no_grad():
        if variant == 'data-write':
            ops_maf.density_fused(x, layer)                    # the order of the degree-built masks is cached here
            key = layer._orders[0]
            mc.set_masks(layer, [m1, m2], through_data=True)
        else:
            mc.set_masks(layer, [m1, m2])
        u, ildj = ops_maf.density_fused(x, layer)
        uc, ic = ops_maf.density_chain(x, layer)
    lins = mc.masked_linears(layer)
    assert np.array_equal(_np(lins[0].mask) != 0, m1) and np.array_equal(_np(lins[1].mask) != 0, m2)
    if variant == 'data-write':
        assert layer._orders[0] == key, 'the write was meant to leave the cached packing order stale'
    want_u, want_ildj = _density64(layer, act, x)
    check = _Checks('A', 'masks[D %d, %d units, %s, %s]' % (D, units, act, variant))
    check('fused u', u, want_u, U_BAR)
    check('fused ildj', ildj, want_ildj, U_BAR)
    check('chain u', uc, want_u, U_BAR)
    check('chain ildj', ic, want_ildj, U_BAR)
    check('fused vs chain u', u, uc, U_BAR)
    check('fused vs chain ildj', ildj, ic, U_BAR)
    check.done()


# ---- B. sampling kernel -----------------------------------------------------------------------------------------------
def _sample_check(layer, act, u, case, group='B'):
    """apply_forward under no_grad took the sampling kernel (one launch) and gives the float64 step loop's numbers."""
    from deeprob.hip import ops_maf
    assert ops_maf.sample_envelope(layer)
    with _counting('dpk_maf_sample_forward') as launches, torch.no_grad():
        x, ldj = layer.apply_forward(u)
    assert launches == [1]
    want_x, want_ldj = mc.sample_step_loop64(layer, act, _np(u))
    check = _Checks(group, case)
    check('x', x, want_x, X_BAR)
    check('ldj', ldj, want_ldj, X_BAR)
    check.done()


# five activations x units 8 / 40 / 70 / 128 (UP = 32 / 64 / 96 / 128); D in {5, 32, 33, 70} (less than one stage of 32
# steps, one exactly, one more, three) and B in {1, 255, 257} walk over the matrix
SAMPLE_CASES = [(act, units, (5, 32, 33, 70)[(a + k) % 4], (1, 255, 257)[(a + k) % 3])
                for a, act in enumerate(ALL_ACTS) for k, units in enumerate((8, 40, 70, 128))]


@pytest.mark.parametrize('act,units,D,B', SAMPLE_CASES)
def test_sampling_kernel_every_width_and_activation(act, units, D, B):
    layer = _layer(D, units, act=act, seed=units + D, mode=('seq', 'rev', 'random')[(units + D) % 3])
    u = torch.randn(B, D, generator=torch.Generator().manual_seed(B + D)).to(DEV)
    _sample_check(layer, act, u, 'sample[%s, %d units, D %d, B %d]' % (act, units, D, B))


@pytest.mark.parametrize('act,units', [('leaky-relu', 40), ('softplus', 128), ('tanh', 70), ('sigmoid', 8)])
def test_sampling_kernel_steps_with_an_all_zero_first_layer_column(act, units):
    """A custom mask whose W1m column is all zero at steps 0, 1, 5, 6, 20 and the last: those steps leave h -- and the
    kernel's cache of act(h) -- as they are, the steps in between must refresh it."""
    D = 33
    layer = _layer(D, units, act=act, seed=4, mode='random')
    rs = np.random.RandomState(units)
    m1, m2 = rs.rand(units, D) < 0.6, rs.rand(2 * D, units) < 0.6
    dead = np.asarray(layer.inv_ordering)[[0, 1, 5, 6, 20, D - 1]]
    m1[:, dead] = False
    mc.set_masks(layer, [m1, m2])
    u = torch.randn(70, D, generator=torch.Generator().manual_seed(units)).to(DEV)
    _sample_check(layer, act, u, 'zero-columns[%s, %d units]' % (act, units))


@pytest.mark.parametrize('act', ['softplus', 'sigmoid'])
def test_sampling_kernel_saturated_units(act):
    layer = _layer(33, 40, act=act, seed=5, mode='seq')
    mc.shift_biases(layer)
    u = torch.randn(255, 33, generator=torch.Generator().manual_seed(6)).to(DEV)
    _sample_check(layer, act, u, 'saturated[%s]' % act)


# ---- C. deep sampling kernel at its limits ------------------------------------------------------------------------------
# 512, 510 and 512 hidden units in all: 131 072, 130 560 and 131 072 bytes of LDS; the last one has the 8 hidden layers
@pytest.mark.parametrize('B', [1, 65])
@pytest.mark.parametrize('D,units,depth,act', [(24, 256, 2, 'softplus'), (40, 170, 3, 'sigmoid'), (20, 64, 8, 'leaky-relu')])
def test_deep_sampling_kernel_at_its_limits(D, units, depth, act, B):
    from deeprob.hip import ops_maf
    layer = _layer(D, units, depth=depth, act=act, seed=depth, mode='random' if depth == 3 else 'seq')
    assert not ops_maf.sample_envelope(layer) and ops_maf.deep_sample_envelope(layer)
    assert units * depth * 256 > 128 * 1024 - 1024
    # a 32-unit conditioner goes first (8 KB of LDS): the large launch must not depend on being the kernel's first
    small = _layer(10, 16, depth=2, act=act, seed=1)
    check = _Checks('C', 'deep[D %d, %d units x %d, %s, B %d]' % (D, units, depth, act, B))
    for tag, lay, width in (('small ', small, 10), ('', layer, D)):
        u = torch.randn(B, width, generator=torch.Generator().manual_seed(B + width)).to(DEV)
        with _counting('dpk_maf_sample_deep_forward') as launches, torch.no_grad():
            x, ldj = lay.apply_forward(u)
        assert launches == [1]
        want_x, want_ldj = mc.sample_step_loop64(lay, act, _np(u))
        check(tag + 'x', x, want_x, X_BAR)
        check(tag + 'ldj', ldj, want_ldj, X_BAR)
    check.done()


# ---- D. backward ------------------------------------------------------------------------------------------------------
def _masked_grads_are_zero(layer):
    for i, m in enumerate(mc.masked_linears(layer)):
        assert np.all(_np(m.weight.grad)[_np(m.mask) == 0] == 0), 'a masked weight of layer %d has a gradient' % i


def _chain_backward_check(layer, act, B, case):
    """Float32 autograd through ops_maf.autoregressive_backward, and density_chain directly, against the float64 torch
    restatement (maf_cases.density64_torch) and its autograd; a masked weight's gradient is exactly zero."""
    from deeprob.hip import ops_maf
    D = layer.in_features
    gen = torch.Generator().manual_seed(11)
    x, wu, wl = torch.randn(B, D, generator=gen), torch.randn(B, D, generator=gen), torch.randn(B, generator=gen)
    u64, ildj64, x64, a64, params64 = mc.density64_torch(layer, act, x)
    ((u64 * wu.double()).sum() + (ildj64 * wl.double()).sum()).backward()
    xg = x.to(DEV).requires_grad_(True)
    u, ildj = ops_maf.autoregressive_backward(xg, layer)
    ((u * wu.to(DEV)).sum() + (ildj * wl.to(DEV)).sum()).backward()
    with torch.no_grad():
        uc, ic = ops_maf.density_chain(xg.detach(), layer)
    check = _Checks('D', case)
    check('u', u, u64, U_BAR)
    check('ildj', ildj, ildj64, U_BAR)
    check('density_chain u', uc, u64, U_BAR)
    check('density_chain ildj', ic, ildj64, U_BAR)
    check('grad.x', xg.grad, x64.grad, G_BAR, grad=True)
    check('grad.scale_act.weight', layer.scale_act.weight.grad.reshape(-1), a64.grad.reshape(-1), G_BAR, grad=True)
    for i, (m, (w64, b64)) in enumerate(zip(mc.masked_linears(layer), params64)):
        check('grad.W%d' % i, m.weight.grad, w64.grad, G_BAR, grad=True)
        check('grad.b%d' % i, m.bias.grad, b64.grad, G_BAR, grad=True)
    _masked_grads_are_zero(layer)
    check.done()


@pytest.mark.parametrize('act', ['leaky-relu', 'softplus', 'sigmoid'])
@pytest.mark.parametrize('depth,mode', [(1, 'random'), (2, 'seq')], ids=['depth1-random', 'depth2-sequential'])
def test_chain_backward_multi_tile_other_activations_vs_float64(depth, mode, act):
    """test_chain_backward_multi_tile_vs_float64 (D = 150, 136 units, B = 200) for the three activation derivatives it
    leaves out: the leaky slope, softplus' derivative from its output (-expm1(-y)) and sigmoid's y (1 - y)."""
    layer = _layer(150, 136, depth=depth, act=act, seed=6, mode=mode)
    _chain_backward_check(layer, act, 200, 'chain-backward[depth %d, %s, %s]' % (depth, mode, act))


@pytest.mark.parametrize('act', ['leaky-relu', 'softplus', 'sigmoid'])
def test_chain_backward_saturated_units_vs_float64(act):
    """Two hidden units near +25 and two near -25: softplus beyond its threshold (y = h, derivative -expm1(-y) = 1 to
    float32) and far below it (y and its derivative about 1e-11), sigmoid where float32 rounds y to 1."""
    layer = _layer(12, 40, depth=2, act=act, seed=9, mode='seq')
    mc.shift_biases(layer)
    _chain_backward_check(layer, act, 33, 'chain-backward-saturated[%s]' % act)


@pytest.mark.parametrize('act', ['softplus', 'leaky-relu'])
@pytest.mark.parametrize('depth', [1, 2])
def test_rsample_gradient_vs_float64(depth, act):
    """apply_forward with autograd on (the differentiable step loop: D conditioner ops, each backward through the
    grad_Z entry of the chained backward) against the float64 torch restatement of the step loop and its autograd."""
    D, units, B = 12, 40, 33
    layer = _layer(D, units, depth=depth, act=act, seed=8, mode='random' if depth == 1 else 'rev')
    gen = torch.Generator().manual_seed(12)
    u, wx, wl = torch.randn(B, D, generator=gen), torch.randn(B, D, generator=gen), torch.randn(B, generator=gen)
    x64, ldj64, u64, a64, params64 = mc.sample64_torch(layer, act, u)
    ((x64 * wx.double()).sum() + (ldj64 * wl.double()).sum()).backward()
    ug = u.to(DEV).requires_grad_(True)
    with _counting('dpk_maf_density_chain_backward', step_loop=True) as backwards, torch.enable_grad():
        x, ldj = layer.apply_forward(ug)
        assert x.requires_grad and ldj.requires_grad
        ((x * wx.to(DEV)).sum() + (ldj * wl.to(DEV)).sum()).backward()
    assert len(backwards) == D
    check = _Checks('D', 'rsample[depth %d, %s]' % (depth, act))
    check('x', x, x64, X_BAR)
    check('ldj', ldj, ldj64, X_BAR)
    check('grad.u', ug.grad, u64.grad, G_BAR, grad=True)
    check('grad.scale_act.weight', layer.scale_act.weight.grad.reshape(-1), a64.grad.reshape(-1), G_BAR, grad=True)
    for i, (m, (w64, b64)) in enumerate(zip(mc.masked_linears(layer), params64)):
        check('grad.W%d' % i, m.weight.grad, w64.grad, G_BAR, grad=True)
        check('grad.b%d' % i, m.bias.grad, b64.grad, G_BAR, grad=True)
    _masked_grads_are_zero(layer)
    check.done()


@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'no-bias'])
def test_masked_linear_multi_tile_vs_float64(bias):
    """MaskedLinear at 150 -> 136 features on a [4, 50, 150] input (200 rows): several tiles in every product."""
    from deeprob.torch.utils import MaskedLinear
    fin, fout = 150, 136
    g = torch.Generator().manual_seed(6)
    mask = (torch.rand(fout, fin, generator=g) < 0.5).numpy()
    torch.manual_seed(2)
    lin = MaskedLinear(fin, fout, mask)
    if not bias:
        lin.bias = None
    lin = lin.to(DEV)
    x = torch.randn(4, 50, fin, generator=g).to(DEV).requires_grad_(True)
    gy = torch.randn(4, 50, fout, generator=g).to(DEV)
    y = lin(x)
    y.backward(gy)
    w = (lin.weight.detach() * lin.mask).double().cpu().numpy()
    xn, gyn = _np(x).astype(np.float64).reshape(-1, fin), _np(gy).astype(np.float64).reshape(-1, fout)
    assert tuple(y.shape) == (4, 50, fout) and tuple(x.grad.shape) == (4, 50, fin)
    check = _Checks('D', 'masked-linear[%s]' % ('bias' if bias else 'no bias'))
    check('y', _np(y).reshape(-1, fout), xn @ w.T + (_np(lin.bias).astype(np.float64) if bias else 0.0), U_BAR)
    check('grad.x', _np(x.grad).reshape(-1, fin), gyn @ w, G_BAR, grad=True)
    check('grad.W', lin.weight.grad, (gyn.T @ xn) * mask, G_BAR, grad=True)
    if bias:
        check('grad.b', lin.bias.grad, gyn.sum(0), G_BAR, grad=True)
    assert np.all(_np(lin.weight.grad)[~mask] == 0)
    check.done()
