"""DgcSpn.posterior_moments / expectation / variance on the device (dpm_dgcspn_moments, csrc/dgc/dgcspn_moments.hip): against
the restatement of tests/dgcspn_moments_ref.py run on the device's own fp32 activations, end to end against float64 (the
oracle's forward plus the restatement), against the statistics of sample_conditional, at its edges, across the grid-stride
loop, and under the buffer contract."""
import functools

import numpy as np
import pytest
import torch

from tests import dgcspn_moments_ref as mref
from tests import dgcspn_topdown_ref as ref
from tests.buffer_contract import contract, PATTERNS
from tests.util import report_measured

pytestmark = pytest.mark.gpu

B = ref.B
assert B == 301                # the odd size: more rows than one, fewer than the grid, no multiple of anything

# The worst error of the kernel against the restatement (float64 flows and moments from the same fp32 scores) over the
# eight variants below and all 301 rows of each, measured on an MI355X (DESIGN.md 18.1,
# profiles/dgcspn_moments_measured_errors.txt); the bound of a measure is ten times its measurement, floored at 1e-6.
MEASURED_WORST_MEAN = 4.913e-07  # (dw12) |mean - ref| / (1 + |ref|)
MEASURED_WORST_VAR = 3.743e-07  # (dw12) |var - ref| / ref (ref >= min scale^2 > 0)
MEASURED_WORST_FLOW = 4.007e-07  # (wide3) |leaf_flow - ref|
# the same measures end to end against float64 -- the oracle's forward and the restatement from x: the fp32 bottom-up pass
# is part of the error, so the floor is 1e-5, the project's bar for an fp32 forward
MEASURED_WORST_MEAN_F64 = 4.557e-04  # (mixed6_mixture)
MEASURED_WORST_VAR_F64 = 4.582e-04  # (mixed6_mixture)
MEASURED_WORST_FLOW_F64 = 3.869e-04  # (mixed6_mixture)


def bound(measured: float, floor: float = 1e-6) -> float:
    return max(10.0 * measured, floor)


# the six cases of the top-down tests, mixed6 with its labels and without (the mixture), and dw4 with its leaves moved to
# |loc| ~ 300 at scales of a few hundredths, where E[x^2] - mean^2 in fp32 has no correct digit left
VARIANTS = ['dw4', 'odd5', 'mixed6', 'mixed6_mixture', 'full3', 'dw12', 'wide3', 'dw4_shifted']


def moments(model, case, x, y, acts, all_classes=None, want_var=True, want_leaf_flow=True, ws=None):
    from deeprob.hip import Workspace, dgcm
    kw = ref.CASES[case]
    return dgcm.dgcspn_moments(kw['in_features'], dgcm.product_geometry(model._product_layers()), kw.get('out_classes', 1), x, y,
                               acts, model._topdown_logw(), model.base_layer.loc, model.base_layer.scale,
                               Workspace() if ws is None else ws, all_classes=(y is None) if all_classes is None else all_classes,
                               want_var=want_var, want_leaf_flow=want_leaf_flow)


@functools.lru_cache(maxsize=None)
def evaluated(variant: str):
    """(case, model on the device, x, y, activations, (mean, var, leaf_flow) of the device, the same of the restatement on the
    device's activations, the same in float64 end to end): computed once a variant and shared, never written to."""
    case = variant.split('_')[0]
    model = ref.make_model(case)
    if variant.endswith('_shifted'):
        with torch.no_grad():
            model.base_layer.loc.add_(300.0)
            model.base_layer.scale.mul_(0.05)
    x, y = ref.make_evidence(model, case)
    if variant.endswith('_shifted'):
        x[3:] = 300.0 + 0.05 * x[3:]                             # (rows 0 .. 2 are what make_evidence made them)
    if variant.endswith('_mixture'):
        y = None
    want64 = mref.restate_float64(model, case, x, y)
    model.cuda()
    xd, yd = x.cuda(), None if y is None else y.cuda()
    with torch.no_grad():
        acts = model._upward_for_sampling(xd)
        got = moments(model, case, xd, yd, acts)
    want = mref.restate_model(model, case, acts, xd, yd)
    return case, model, xd, yd, acts, got, want, want64


def _errors(got, want, hid_reached):
    mean, var, flow = (t.double().cpu().numpy() for t in got)
    rmean, rvar, rflow = want
    e_mean = float((np.abs(mean - rmean) / (1.0 + np.abs(rmean)))[hid_reached].max())
    e_var = float((np.abs(var - rvar)[hid_reached] / rvar[hid_reached]).max())
    e_flow = float(np.abs(flow - rflow).max())
    return e_mean, e_var, e_flow


def _reached(case, xd):
    """NaN entries of pixels in scope, [B, C, H, W] bool on the host."""
    _, h, w = ref.CASES[case]['in_features']
    scope = np.ones((h, w), bool)
    if case == 'odd5':
        scope[-1, :] = scope[:, -1] = False
    hid = torch.isnan(xd).cpu().numpy()
    return hid & scope[None, None], hid & ~scope[None, None]


@pytest.mark.parametrize('variant', VARIANTS)
def test_against_the_restatement(variant):
    """mean, var and leaf_flow of all 301 rows (row 0 all NaN, row 1 fully observed, row 2 at 40 scales: scores far below
    where expf underflows) against the restatement on the device's own activations, no row left out; the public methods
    are this launch; observed entries bit for bit with variance 0; a NaN entry out of scope is NaN in both outputs; no NaN
    anywhere else."""
    case, model, xd, yd, acts, got, want, _ = evaluated(variant)
    mean, var, flow = got
    kw = ref.CASES[case]
    assert tuple(mean.shape) == tuple(var.shape) == (B,) + tuple(kw['in_features']) and mean.is_cuda and mean.dtype == torch.float32
    assert tuple(flow.shape) == (B, kw['n_batch']) + tuple(kw['in_features'][1:]) == tuple(want[2].shape)
    pm, pv = model.posterior_moments(xd, yd)
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same(pm, mean) and same(pv, var)
    assert same(model.expectation(xd, yd), mean) and same(model.variance(xd, yd), var)
    obs = ~torch.isnan(xd)
    assert same(mean[obs], xd[obs]) and (var[obs] == 0).all()
    assert not obs[0].any() and obs[1].all() and obs[2].any() and not obs[2].all()
    reached, outside = _reached(case, xd)
    assert outside.any() == (case == 'odd5') and reached[0].any() and reached[2].any()
    mean_h, var_h, flow_h = (t.double().cpu().numpy() for t in got)
    assert np.isnan(mean_h[outside]).all() and np.isnan(var_h[outside]).all()
    assert np.isnan(want[0][outside]).all() and np.isnan(want[1][outside]).all()
    assert np.isfinite(mean_h[~outside]).all() and np.isfinite(var_h[~outside]).all() and np.isfinite(flow_h).all()
    assert np.isfinite(want[0][~outside]).all() and np.isfinite(want[2]).all() and (want[1][reached] > 0).all()
    assert want[1][reached].min() >= float(model.base_layer.scale.detach().min()) ** 2 * (1.0 - 1e-6)
    e_mean, e_var, e_flow = _errors(got, want, reached)
    b_mean, b_var, b_flow = bound(MEASURED_WORST_MEAN), bound(MEASURED_WORST_VAR), bound(MEASURED_WORST_FLOW)
    name = 'test_against_the_restatement[%s]' % variant
    report_measured(name + ' mean error', e_mean, b_mean)
    report_measured(name + ' var error', e_var, b_var)
    report_measured(name + ' max |leaf_flow - ref|', e_flow, b_flow)
    print('%s: mean %.3e var %.3e leaf_flow %.3e (row 2: mean %.3e)' % (
        variant, e_mean, e_var, e_flow, float(np.abs(mean_h[2] - want[0][2])[reached[2]].max())))
    assert e_mean <= b_mean, e_mean
    assert e_var <= b_var, e_var
    assert e_flow <= b_flow, e_flow


@pytest.mark.parametrize('variant', VARIANTS)
def test_end_to_end_against_float64(variant):
    """The same three measures against the oracle's float64 forward plus the restatement from x: what a user sees of the
    fp32 bottom-up pass and the fp32 top-down pass together."""
    case, model, xd, yd, acts, got, _, want64 = evaluated(variant)
    reached, _ = _reached(case, xd)
    e_mean, e_var, e_flow = _errors(got, want64, reached)
    b_mean, b_var, b_flow = (bound(m, 1e-5) for m in (MEASURED_WORST_MEAN_F64, MEASURED_WORST_VAR_F64, MEASURED_WORST_FLOW_F64))
    name = 'test_end_to_end_against_float64[%s]' % variant
    report_measured(name + ' mean error', e_mean, b_mean)
    report_measured(name + ' var error', e_var, b_var)
    report_measured(name + ' max |leaf_flow - ref|', e_flow, b_flow)
    rows = np.where(reached, np.abs(got[0].double().cpu().numpy() - want64[0]) / (1.0 + np.abs(want64[0])), 0.0).max(axis=(1, 2, 3))
    print('%s end to end: mean %.3e var %.3e leaf_flow %.3e (mean: worst row %d, worst of the rows but row 2 %.3e)' % (
        variant, e_mean, e_var, e_flow, int(rows.argmax()), float(np.delete(rows, 2).max())))
    assert e_mean <= b_mean, e_mean
    assert e_var <= b_var, e_var
    assert e_flow <= b_flow, e_flow


def test_labels_and_the_mixture():
    """mixed6 has three roots: a row's posterior under its label differs from the mixture of the classes (both are checked
    against the restatement above, the restatement's mixture against float64 autograd in the host tests); a model with one
    root ignores y."""
    case, model, xd, yd, acts, (mean, var, flow), _, _ = evaluated('mixed6')
    _, _, _, _, _, (mmean, mvar, mflow), _, _ = evaluated('mixed6_mixture')
    hid = torch.isnan(xd)
    assert (mean[hid] - mmean[hid]).abs().max() > 1e-3
    case1, single, x1, _, _, (mean1, var1, _), _, _ = evaluated('dw4')
    m, v = single.posterior_moments(x1, torch.full((B,), 2, device='cuda'))
    assert torch.equal(m.view(torch.int32), mean1.view(torch.int32)) and torch.equal(v.view(torch.int32), var1.view(torch.int32))


@pytest.mark.parametrize('case', ['dw4', 'mixed6'])
def test_mean_of_conditional_samples(case):
    """4 096 draws of sample_conditional (fixed seed) of one half-observed row: their mean within 5 standard errors,
    sqrt(var / n) with var from posterior_moments, of the expectation -- every NaN entry."""
    model = evaluated(case)[1]
    n = 4096
    row = ref.half_observed_row(model, case).cuda()
    y1 = torch.tensor([1], device='cuda') if case == 'mixed6' else None
    mean, var = model.posterior_moments(row, y1)
    draws = model.sample_conditional(row.expand(n, -1, -1, -1).contiguous(), None if y1 is None else y1.expand(n).contiguous(),
                                     seed=20250311)
    hid = torch.isnan(row[0])
    assert hid.any() and not hid.all() and torch.isfinite(mean).all()
    se = torch.sqrt(var[0].double() / n)
    z = ((draws.double().mean(dim=0) - mean[0].double()) / se)[hid]
    print(case, 'in standard errors', z.cpu().numpy())
    assert (z.abs() <= 5.0).all(), z


def test_grid_stride_reuses_a_workspace_slice():
    """B = DPM_MAX_GROUPS + 37: the last rows are the second image of their work-group and of its workspace slice; each is
    bit for bit the same row evaluated alone, and two calls agree bit for bit."""
    from deeprob.hip import dgcm
    case, model = evaluated('dw4')[:2]
    n = dgcm.DPM_MAX_GROUPS + 37
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(n, 1, 4, 4, generator=gen)
    x[torch.rand(x.shape, generator=gen) < 0.5] = float('nan')
    x = x.cuda()
    with torch.no_grad():
        acts = model._upward_for_sampling(x)
    first = moments(model, case, x, None, acts)
    again = moments(model, case, x, None, acts)
    for a, b in zip(first, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for k in (0, 36, 37, dgcm.DPM_MAX_GROUPS - 1, dgcm.DPM_MAX_GROUPS, n - 1):
        alone = moments(model, case, x[k:k + 1], None, [a[k:k + 1].contiguous() for a in acts])
        for a, b in zip(first, alone):
            assert torch.equal(a[k:k + 1].view(torch.int32), b.view(torch.int32)), k


@pytest.mark.parametrize('variant', ['odd5', 'mixed6', 'wide3'])
def test_buffer_contract(variant):
    """Poisoned, guard-banded mean / var / leaf_flow and workspace (0xFF, 0x7F), B = 301, 1 and 0, with and without the
    optional outputs: every element of every output written, nothing outside them or the workspace, nothing read from what
    they held, and the evidence, the labels, the activations, the tables and the leaf parameters bitwise what they were."""
    from deeprob.hip import Workspace
    case, model, xd, yd, acts, want, _, _ = evaluated(variant)
    logws = model._topdown_logw()
    for pattern in PATTERNS:
        for n in (B, 1, 0):
            for optional in (True, False):
                xs, ys, ac = xd[:n], None if yd is None else yd[:n], [a[:n].contiguous() for a in acts]
                with contract(pattern) as c:
                    c.frozen(xs, ys, model.base_layer.loc, model.base_layer.scale, *ac, *logws)
                    got = moments(model, case, xs, ys, ac, want_var=optional, want_leaf_flow=optional, ws=Workspace())
                    c.expect_written(*got)
                    assert len(c.allocations) >= (0 if n == 0 else 2)
                assert (got[1] is None) == (got[2] is None) == (not optional)
                for g, w in zip(got, want):
                    assert g is None or torch.equal(g.view(torch.int32), w[:n].view(torch.int32)), (pattern, n, optional)


def test_impossible_evidence_is_nan_in_the_nan_entries_only():
    """Rows whose root maximum is -inf or NaN, by activations of -inf / NaN handed to the launch (the leaf layer clamps log 0
    as the reference's nan_to_num does, so no evidence reaches this through the public method): NaN in the NaN entries of
    mean and var, the observed entries as given with variance 0, NaN flows; every other row is bit for bit what it was."""
    case, model, xd, yd, acts, (mean, var, flow), _, _ = evaluated('mixed6')
    bad = torch.zeros(B, dtype=torch.bool, device='cuda')
    bad[2::3] = True
    for fill in (float('-inf'), float('nan')):
        broken = [torch.where(bad[:, None, None, None], torch.full_like(a, fill), a) for a in acts]
        m, v, f = moments(model, case, xd, yd, broken)
        hid = torch.isnan(xd)
        assert torch.isnan(m[bad][hid[bad]]).all() and torch.isnan(v[bad][hid[bad]]).all() and torch.isnan(f[bad]).all()
        assert torch.equal(m[bad][~hid[bad]], xd[bad][~hid[bad]]) and (v[bad][~hid[bad]] == 0).all()
        same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert same(m[~bad], mean[~bad]) and same(v[~bad], var[~bad]) and same(f[~bad], flow[~bad])


def test_edges():
    """A non-contiguous x; an empty batch; labels out of range, of the wrong length, of another integer dtype; a wrong input
    shape; a CPU tensor; training-mode dropout."""
    from deeprob.hip import HipError
    from deeprob.spn.models import DgcSpn
    case, model, xd, yd, acts, (mean, var, flow), _, _ = evaluated('mixed6')
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    xt = xd.transpose(2, 3).contiguous().transpose(2, 3)
    assert not xt.is_contiguous() and same(xt, xd)
    m, v = model.posterior_moments(xt, yd)
    assert same(m, mean) and same(v, var) and m.is_contiguous()
    wide = torch.full((B, 2, 6, 12), float('nan'), device='cuda')
    wide[:, :, :, ::2] = xd
    m, v = model.posterior_moments(wide[:, :, :, ::2], yd)
    assert same(m, mean) and same(v, var)
    for y in (None, torch.empty(0, dtype=torch.long, device='cuda')):
        m, v = model.posterior_moments(xd[:0], y)
        assert tuple(m.shape) == tuple(v.shape) == (0, 2, 6, 6) and m.is_cuda
    assert model.posterior_moments(xd[:0], want_var=False)[1] is None
    for wrong in (3, -1):
        y = yd.clone()
        y[17] = wrong
        with pytest.raises(ValueError, match='labels must lie in'):
            model.posterior_moments(xd, y)
    with pytest.raises(ValueError):
        model.posterior_moments(xd, yd[:5])
    with pytest.raises(ValueError):
        model.posterior_moments(xd[:, :, :5], yd)
    with pytest.raises(ValueError):
        model.posterior_moments(xd[:, 0], yd)
    with pytest.raises(HipError):
        model.posterior_moments(xd.cpu(), yd)
    assert same(model.expectation(xd, yd.to(torch.int32)), mean)
    drop = DgcSpn((1, 4, 4), n_batch=2, sum_channels=2, depthwise=True, sum_dropout=0.2).cuda().train()
    with pytest.raises(NotImplementedError, match='dropout'):
        drop.posterior_moments(torch.randn(3, 1, 4, 4, device='cuda'))
    assert torch.isfinite(drop.eval().expectation(torch.randn(3, 1, 4, 4, device='cuda'))).all()
