"""The references and the route restatement of tests/test_ratspn_gaussian_gpu.py, pinned on the host before any device run:
the case table, which routes the device file's parametrisations reach (read from that file, not copied), the float64
reference against a direct numpy statement of the Gaussian leaf sum, and the float32 reference's own distance from it."""
import math

import numpy as np
import pytest
import torch

from tests import ratspn_gaussian_cases as gc
from tests import test_ratspn_gaussian_gpu as dev
from tests.ratspn_gaussian_cases import GRAD_TOL
from tests.util import rel_err, grad_err, report_measured


@pytest.mark.parametrize('variant', gc.VARIANTS)
@pytest.mark.parametrize('name', sorted(gc.CASES))
def test_case_table(name, variant):
    """make_model asserts R / I / d / pad of the table for both variants; the parameters are as documented and seeded."""
    model = gc.make_model(name, variant)
    base = model.base_layer
    if variant == 'scaled':
        s = base.scale.detach()
        assert (s == 0.05).sum().item() >= 1 and (s == 20.0).sum().item() >= 1 and s.min().item() >= 0.05
    else:
        assert not base.scale.requires_grad and bool((base.scale == 1).all())
    again = gc.make_model(name, variant)
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), again.state_dict().values()))
    far = gc.make_model(name, variant, 'far_means').base_layer.loc.detach()
    assert (far.abs() == 8).sum().item() >= 2 and base.loc.detach().abs().max().item() < 6.0


def _forward_routes():
    routes = set()
    for name in dev.FWD_NAMES:
        for variant in gc.VARIANTS:
            for B in dev.FWD_BATCHES:
                routes.add(gc.forward_route(name, variant, B))
    for name in dev.HINT_NAMES:
        routes.add(gc.forward_route(name, 'unit', dev.HINT_BATCH))
    for name in dev.MFMA_OFF_NAMES:
        routes.add(gc.forward_route(name, 'unit', dev.MFMA_OFF_BATCH, mfma=False))
    for variant in gc.VARIANTS:
        routes.add(gc.forward_route(dev.TWO_PER_LANE[0], variant, dev.TWO_PER_LANE[1]))
    return routes


def _backward_routes():
    """{(route, padded, ragged last column tile)} over the device file's backward parametrisations."""
    routes = set()

    def add(name, variant, B, **kw):
        routes.add((gc.backward_route(name, variant, B, variant == 'scaled', **kw),) + gc.moment_shape(name))

    for p in dev.BWD_PARAMS:
        name, variant, B = p.values[:3]
        add(name, variant, B)
    for name in dev.MISALIGNED_NAMES:
        for what in dev.MISALIGNED_WHAT:
            add(name, 'scaled', dev.MISALIGNED_BATCH, x_aligned=what == 'g', g_aligned=what == 'x')
    for name in dev.ILL_NAMES:
        for B in dev.ILL_BATCHES:
            add(name, 'scaled', B)
    for name in dev.DROPOUT_NAMES:
        for B in dev.DROPOUT_BATCHES:
            add(name, 'scaled', B, dropout=True)
    return routes


def test_forward_route_coverage():
    """Every forward route of the dispatch is reached by some parametrisation of the device file: the test fails when a
    combination loses its last case."""
    routes = _forward_routes()
    gemm = [r for r in routes if r[0] == 'gemm']
    valu = [r for r in routes if r[0] == 'valu']
    assert {r[1] for r in gemm} == {2, 4}                                     # NTG
    ragged_nch = {n for n in dev.FWD_NAMES if gc.forward_route(n, 'unit', 65)[0] == 'gemm' and gc.geometry(n)[0] % 32}
    ragged_ng = {n for n in dev.FWD_NAMES if gc.forward_route(n, 'unit', 65)[0] == 'gemm'
                 and (gc.geometry(n)[1] * gc.geometry(n)[2]) % (32 * gc.forward_route(n, 'unit', 65)[1])}
    assert ragged_nch and ragged_ng, (ragged_nch, ragged_ng)
    assert any(gc.geometry(n)[4] > 0 for n in dev.FWD_NAMES if gc.forward_route(n, 'unit', 65)[0] == 'gemm')   # padded GEMM
    assert {r[2] for r in valu} == {1, 2, 4, 8}                               # CB
    assert {r[1] for r in valu} == {2, 4}                                     # QB
    assert {r[3] for r in valu} == {1, 2}                                     # SPL
    assert ('valu', 4, 8, 2, True, False) in routes                           # SPL 2 at CB 8
    assert any(r[2] == 1 and not r[4] for r in valu)                          # GEN false at CB 1
    assert any(r[2] == 2 and not r[4] and r[5] for r in valu)                 # GEN false, compact records, CB 2
    assert any(r[2] == 2 and not r[4] and not r[5] for r in valu)             # GEN false at CB 2 without LDS records (I > 2)
    assert {r[2] for r in valu if r[4]} == {1, 2, 4, 8}                       # GEN true at every CB
    # the unit-scale VALU kernels at CB 8 and 4 (reached with the matrix-core route off, or beyond its 64 chunks)
    for name in dev.MFMA_OFF_NAMES:
        assert gc.forward_route(name, 'unit', dev.MFMA_OFF_BATCH)[0] == 'gemm'
    assert {gc.forward_route(n, 'unit', dev.MFMA_OFF_BATCH, mfma=False)[2] for n in dev.MFMA_OFF_NAMES} == {4, 8}
    assert gc.forward_route('beyond_gemm', 'unit', 65) == ('valu', 4, 8, 1, True, False)
    # the table's own claims
    assert gc.forward_route('mnist8', 'unit', 300) == ('gemm', 4, 1, 25)
    assert gc.forward_route('wide16_d1', 'unit', 300) == ('gemm', 4, 1, 4)
    assert gc.forward_route('ad4', 'unit', 300) == ('gemm', 4, 2, 49)
    assert gc.forward_route('pairs_gemm', 'unit', 300) == ('gemm', 2, 1, 3)
    assert gc.forward_route('pad2', 'unit', 300) == ('valu', 4, 2, 2, False, True)
    assert gc.forward_route('pad2', 'scaled', 300) == ('valu', 4, 2, 2, True, False)
    assert gc.forward_route('one', 'unit', 300) == ('valu', 4, 1, 2, False, False)
    assert gc.forward_route('six', 'unit', 300) == ('valu', 4, 2, 2, False, False)
    assert gc.forward_route('wide16_d1', 'scaled', 300) == ('valu', 2, 8, 1, True, False)
    assert gc.forward_route('mnist8', 'unit', 300, x_aligned=False)[0] == 'valu'


def test_backward_route_coverage():
    """Every backward route of the dispatch is reached by some parametrisation of the device file: the test fails when a
    combination loses its last case."""
    routes = _backward_routes()
    plain_routes = {r[0] for r in routes}
    for w1 in (True, False):
        assert any(r[0] == ('moment', w1) and r[1] for r in routes), ('moment, padded', w1)
        assert any(r[0] == ('moment', w1) and r[2] for r in routes), ('moment, ragged last column tile', w1)
    staged = [r for r in plain_routes if r[0] == 'staged']
    assert {r[1] for r in staged} == {1, 2, 4}                                # CBK
    assert {r[2] for r in staged} == {True, False}                            # WANT1
    assert {r[3] for r in staged} >= {1, 4}                                   # passes
    plain = [r for r in plain_routes if r[0] == 'plain']
    assert {(r[1], r[2]) for r in plain} == {(c, t) for c in (1, 2, 4) for t in (16, 64)}
    # the table's own claims
    assert gc.backward_route('many_groups', 'scaled', 1024, True) == ('staged', 1, True, 4)
    assert gc.backward_route('long_rows', 'scaled', 70, True) == ('plain', 1, 16)
    assert gc.backward_route('mnist8', 'scaled', 2048, True) == ('moment', True)
    assert gc.backward_route('mnist8', 'unit', 2049, False) == ('plain', 4, 64)
    assert gc.backward_route('pad2', 'scaled', 300, True) == ('staged', 2, True, 1)
    assert gc.backward_route('six', 'scaled', 1100, True) == ('plain', 2, 64)
    assert gc.backward_route('beyond_gemm', 'unit', 300, False) == ('moment', False)
    # I = 4 and 8 leave the moment kernel only when it declines: g misaligned.  mnist8 then reaches the staged kernel with
    # CBK 4; ad4's 16 rows of D + 4 R floats (111,872 B) exceed the staged kernel's 80 KB, so it takes the 16-sample kernel
    assert gc.backward_route('mnist8', 'scaled', 300, True, g_aligned=False) == ('staged', 4, True, 1)
    assert gc.backward_route('ad4', 'scaled', 300, True, g_aligned=False) == ('plain', 4, 16)
    assert gc.backward_route('mnist8', 'scaled', 300, True, x_aligned=False) == ('moment', True)
    assert gc.backward_route('mnist8', 'scaled', 300, True, x_aligned=False, g_aligned=False) == ('plain', 4, 16)


def _numpy_leaf(x, mask, pad_mask, loc, scale):
    """The Gaussian leaf sum stated directly: over the real, observed variables of a region."""
    z = (x[:, mask][:, :, None, :] - loc[None]) / scale[None]                 # [B, R, I, d]
    term = -0.5 * z * z - np.log(scale)[None] - 0.5 * math.log(2.0 * math.pi)
    keep = ~np.isnan(x[:, mask])[:, :, None, :] & (True if pad_mask is None else ~pad_mask[None])
    return np.where(keep, term, 0.0).sum(-1)


@pytest.mark.parametrize('kind', ['clean', 'nan', 'huge'])
@pytest.mark.parametrize('variant', gc.VARIANTS)
@pytest.mark.parametrize('name', ['pad2', 'heavy_pad'])
def test_forward_reference_is_the_leaf_sum(name, variant, kind):
    """The float64 reference on the two padded two-channel cases against the numpy statement: padding and NaN handling."""
    st = gc.leaf_state(gc.make_model(name, variant))
    x = gc.make_evidence(name, 70, kind)
    want = _numpy_leaf(x.double().numpy(), st['mask'].numpy(), None if st['pad_mask'] is None else st['pad_mask'].numpy(),
                       st['loc'].numpy(), st['scale'].numpy())
    got = gc.forward_reference(st, x)
    assert rel_err(got, want) <= 1e-12
    if kind == 'nan':
        assert (got[0] == 0).all() and not torch.isnan(x[1]).any()
        assert abs(torch.isnan(x[2:]).float().mean().item() - 0.2) < 0.05


def test_evidence_kinds():
    x = gc.make_evidence('mnist8', 300, 'huge')
    assert (x[2] == 7.0).all() and (x[2] ** 2).sum().item() > 36 * 784
    assert all((x == v).sum().item() >= 100 for v in (1e3, -1e3, 1e6, -1e6))
    x = gc.make_evidence('mnist8', 300, 'inf')
    assert gc.inf_row_mask(x).nonzero().flatten().tolist() == [2, 3]
    assert torch.isinf(x[2]).sum().item() == 1 and torch.isinf(x[3]).sum().item() == 1 and torch.isnan(x[0]).all()
    ref = gc.forward_reference(gc.leaf_state(gc.make_model('mnist8', 'unit')), x)
    assert np.isfinite(ref).all() and (np.abs(ref[2:4]).max(axis=(1, 2)) > 1e38).all()   # float32's largest, not float64's
    g = gc.make_upstream('mnist8', 300, 'negative')
    assert (g <= 0).all() and (gc.make_upstream('mnist8', 300, 'mixed') > 0).any()
    v = gc.misaligned(torch.arange(12.0).view(3, 4))
    assert v.data_ptr() % 16 != 0 and v.data_ptr() % 4 == 0 and torch.equal(v, torch.arange(12.0).view(3, 4))


@pytest.mark.parametrize('name', ['pad2', 'heavy_pad', 'odd3'])
def test_reference_grads_against_the_leaf_sum(name):
    """reference_grads is the gradient of the numpy leaf sum: central differences in one observed entry of x, one mean and
    one scale (NaN evidence, padding); x.grad is 0 at marginalised entries, parameter gradients 0 at padded positions; the
    row blocks add up to the whole batch."""
    st = gc.leaf_state(gc.make_model(name, 'scaled'))
    B = 70
    x, g = gc.make_evidence(name, B, 'nan'), gc.make_upstream(name, B, 'mixed')
    ref = gc.reference_grads(st, x, g)
    whole = gc.reference_grads(st, x, g, block=B)
    for k in ('loc', 'scale', 'x'):
        assert grad_err(ref[k], whole[k]) <= 1e-13, k
    nan = torch.isnan(x).numpy()
    assert (ref['x'][nan] == 0).all() and np.isfinite(ref['x']).all()
    mask = st['mask'].numpy()
    pm = None if st['pad_mask'] is None else st['pad_mask'].numpy()
    if pm is not None:
        full = np.broadcast_to(pm, ref['loc'].shape)
        assert (ref['loc'][full] == 0).all() and (ref['scale'][full] == 0).all()

    def f(xx, loc, scale):
        return (_numpy_leaf(xx, mask, pm, loc, scale) * g.double().numpy()).sum()

    x64, loc, scale = x.double().numpy(), st['loc'].numpy(), st['scale'].numpy()
    h = 1e-6
    b, v = np.argwhere(~nan)[11]
    xp, xm = x64.copy(), x64.copy()
    xp[b, v] += h
    xm[b, v] -= h
    assert abs((f(xp, loc, scale) - f(xm, loc, scale)) / (2 * h) - ref['x'][b, v]) <= 1e-6 * np.abs(ref['x']).max()
    real = np.argwhere(np.ones(loc.shape, bool) if pm is None else ~np.broadcast_to(pm, loc.shape))[5]
    for key, arr in (('loc', loc), ('scale', scale)):
        hh = h * abs(arr[tuple(real)]) if key == 'scale' else h
        up, dn = arr.copy(), arr.copy()
        up[tuple(real)] += hh
        dn[tuple(real)] -= hh
        args_up = (up, scale) if key == 'loc' else (loc, up)
        args_dn = (dn, scale) if key == 'loc' else (loc, dn)
        fd = (f(x64, *args_up) - f(x64, *args_dn)) / (2 * hh)
        assert abs(fd - ref[key][tuple(real)]) <= 1e-5 * np.abs(ref[key]).max(), key


@pytest.mark.parametrize('kind', ['clean', 'nan'])
@pytest.mark.parametrize('name', sorted(gc.CASES))
def test_float32_reference_distance_from_float64(name, kind):
    """What the widening term of the device bar, 2 * grad_err(ref32, ref64), amounts to in the plain regime: written down per
    case, and below GRAD_TOL / 10 -- there the device tests hold the kernels to GRAD_TOL itself."""
    st = gc.leaf_state(gc.make_model(name, 'scaled'))
    B = 300
    x, g = gc.make_evidence(name, B, kind), gc.make_upstream(name, B, 'mixed')
    ref64, ref32 = gc.reference_grads(st, x, g), gc.reference_grads(st, x, g, torch.float32)
    tag = 'test_float32_reference_distance_from_float64[%s-%s]' % (name, kind)
    err = rel_err(ref32['out'], ref64['out'])
    report_measured(tag + ' out', err, 1e-6)
    assert err <= 1e-6
    for k in ('loc', 'scale', 'x'):
        own = grad_err(ref32[k], ref64[k])
        report_measured(tag + ' grad.' + k, own, GRAD_TOL / 10)
        assert own <= GRAD_TOL / 10, (k, own)


@pytest.mark.parametrize('regime', gc.ILL_REGIMES)
def test_ill_regimes(regime):
    """The ill-conditioned regimes on a table case: |mu| / s is large, the float32 reference's own distance is written down
    (it may exceed GRAD_TOL / 10: what the widening term of the device bar is for), and the NaN kind marginalises 20 %."""
    model, x = gc.make_ill_case('ad4', regime, 64)
    base = model.base_layer
    assert (base.loc.detach().abs() / base.scale.detach()).median().item() > 10
    g = gc.make_upstream('ad4', 64, 'mixed')
    st = gc.leaf_state(model)
    ref64, ref32 = gc.reference_grads(st, x, g), gc.reference_grads(st, x, g, torch.float32)
    for k in ('loc', 'scale', 'x'):
        own = grad_err(ref32[k], ref64[k])
        report_measured('test_ill_regimes[%s] oracle fp32 vs fp64 grad.%s' % (regime, k), own, float('inf'), '(no bound: written down)')
        assert np.isfinite(ref64[k]).all() and np.isfinite(ref32[k]).all()
    _, xn = gc.make_ill_case('ad4', regime, 64, 'nan')
    assert torch.isnan(xn[0]).all() and not torch.isnan(xn[1]).any() and abs(torch.isnan(xn[2:]).float().mean().item() - 0.2) < 0.05
