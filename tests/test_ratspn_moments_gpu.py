"""RatSpn.posterior_moments / expectation / variance on the device (dpr_ratspn_moments, csrc/rat/ratspn_moments.hip):
against the restatement of tests/ratspn_moments_ref.py run on the device's own fp32 activations, against an enumerated
posterior and the statistics of sample_conditional, at its edges, for determinism, and under the buffer contract."""
import functools

import numpy as np
import pytest
import torch

from tests import ratspn_moments_ref as mref
from tests import ratspn_posterior_ref as pref
from tests.buffer_contract import contract, PATTERNS
from tests.test_ratspn_posterior_gpu import CASES, make_case, B
from tests.util import report_measured

pytestmark = pytest.mark.gpu

assert B == 301                # the odd size: more rows than one, fewer than the grid, no multiple of anything

# The worst error of the kernel against the restatement (float64 flows and moments from the same fp32 scores) over all seven
# cases below and all 301 rows of each, measured on an MI355X; the bound of a measure is ten times its
# measurement, floored at 1e-6 and capped at 1e-4.
MEASURED_WORST_MEAN = 7.394e-07  # (wide) |mean - ref| / (1 + |ref|), Gaussian leaves
MEASURED_WORST_VAR = 6.110e-07  # (wide) |var - ref| / ref, Gaussian leaves (ref >= min scale^2 > 0)
MEASURED_WORST_BERNOULLI = 9.925e-08  # |.| of mean and var, Bernoulli leaves
MEASURED_WORST_FLOW = 2.964e-07  # (pad) |leaf_flow - ref|
# the fp32 bottom-up pass's share of the error against the enumerated posterior (test 2): the restatement on the device's
# fp32 activations against the enumeration in float64
MEASURED_FORWARD_SHARE = 5.668e-09


def bound(measured: float) -> float:
    return min(max(10.0 * measured, 1e-6), 1e-4)


def moments(model, x, y, acts, all_classes=None, want_var=True, want_leaf_flow=True):
    from deeprob.hip import rat
    dist, p0, p1 = model._leaf_params()
    return rat.ratspn_moments(dist, model._fused_ctx, x, y, acts, model._topdown_logw(), model._topdown_src(), p0, p1,
                              all_classes=(y is None) if all_classes is None else all_classes, want_var=want_var,
                              want_leaf_flow=want_leaf_flow)


@functools.lru_cache(maxsize=None)
def evaluated(case: str):
    """(model on the device, x, y, activations, (mean, var, leaf_flow) of the device, the same of the restatement on the
    device's activations): computed once a case and shared, never written to."""
    name = {'classes_mixture': 'classes', 'shifted': 'pad'}.get(case, case)
    model, x, y = make_case(name)
    if case == 'classes_mixture':
        y = None
    if case == 'shifted':
        # |loc| >> scale: the channels of a variable lie near 300 with scales of a few hundredths, where E[x^2] - mean^2 in
        # fp32 has no correct digit left (mean^2 / var ~ 1e5 .. 1e7)
        with torch.no_grad():
            model.base_layer.loc.add_(300.0)
            model.base_layer.scale.mul_(0.05)
        x = x + 300.0
    model.cuda()
    xd, yd = x.cuda(), None if y is None else y.cuda()
    with torch.no_grad():
        acts = model._upward_for_mpe(xd)
        got = moments(model, xd, yd, acts)
    want = mref.restate_model(model, acts, xd, yd)
    return model, xd, yd, acts, got, want


ALL = ['depth1', 'pad', 'classes', 'classes_mixture', 'wide', 'bernoulli', 'shifted']


@pytest.mark.parametrize('case', ALL)
def test_against_the_restatement(case):
    """mean, var and leaf_flow of all 301 rows (row 0 all NaN, row 1 fully observed, row 2 with scores near -3e5) against the
    restatement on the device's own activations; the public methods are this launch; observed entries bit for bit with
    variance 0; no NaN anywhere."""
    model, xd, yd, acts, (mean, var, flow), (rmean, rvar, rflow) = evaluated(case)
    D = xd.shape[1]
    assert tuple(mean.shape) == tuple(var.shape) == (B, D) and mean.is_cuda and mean.dtype == torch.float32
    assert tuple(flow.shape) == tuple(rflow.shape)
    pm, pv = model.posterior_moments(xd, yd)
    assert torch.equal(pm, mean) and torch.equal(pv, var)
    assert torch.equal(model.expectation(xd, yd), mean) and torch.equal(model.variance(xd, yd), var)
    obs = ~torch.isnan(xd)
    assert torch.equal(mean[obs].view(torch.int32), xd[obs].view(torch.int32)) and (var[obs] == 0).all()
    assert not obs[0].any() and obs[1].all() and obs[2].any() and not obs[2].all()
    mean, var, flow = mean.double().cpu().numpy(), var.double().cpu().numpy(), flow.double().cpu().numpy()
    assert np.isfinite(mean).all() and np.isfinite(var).all() and np.isfinite(flow).all()
    assert np.isfinite(rmean).all() and np.isfinite(rvar).all() and np.isfinite(rflow).all()
    hid = ~obs.cpu().numpy()
    assert (rvar[hid] > 0).all()
    e_flow = float(np.abs(flow - rflow).max())
    report_measured('test_against_the_restatement[%s] max |leaf_flow - ref|' % case, e_flow, bound(MEASURED_WORST_FLOW))
    if case == 'bernoulli':
        e_mean, e_var = float(np.abs(mean - rmean)[hid].max()), float(np.abs(var - rvar)[hid].max())
        b_mean = b_var = bound(MEASURED_WORST_BERNOULLI)
    else:
        e_mean = float((np.abs(mean - rmean) / (1.0 + np.abs(rmean)))[hid].max())
        e_var = float((np.abs(var - rvar)[hid] / rvar[hid]).max())
        b_mean, b_var = bound(MEASURED_WORST_MEAN), bound(MEASURED_WORST_VAR)
        assert rvar[hid].min() >= float(model.base_layer.scale.detach().min()) ** 2 * (1.0 - 1e-6)
    report_measured('test_against_the_restatement[%s] mean error' % case, e_mean, b_mean)
    report_measured('test_against_the_restatement[%s] var error' % case, e_var, b_var)
    print('%s: mean %.3e var %.3e leaf_flow %.3e (row 2: mean %.3e)' % (
        case, e_mean, e_var, e_flow, float(np.abs(mean[2] - rmean[2]).max())))
    assert e_flow <= bound(MEASURED_WORST_FLOW), e_flow
    assert e_mean <= b_mean, e_mean
    assert e_var <= b_var, e_var


def test_expectation_is_the_enumerated_posterior():
    """The enumerable Bernoulli model: p(x_f = 1 | e) of the three missing variables from the 8 enumerated completions in
    float64.  The tolerance is the kernel's bound against the restatement plus the fp32 bottom-up pass's share, which is
    measured as the restatement on the device's activations against the enumeration."""
    model, row, full, post = pref.enumerable_case()
    model.cuda()
    want = (post[:, None] * full.double().numpy()).sum(axis=0)                 # [6]: the posterior marginals
    xd = row.cuda()
    got = model.expectation(xd).double().cpu().numpy()[0]
    var = model.variance(xd).double().cpu().numpy()[0]
    with torch.no_grad():
        acts = model._upward_for_mpe(xd)
    share = float(np.abs(mref.restate_model(model, acts, xd)[0][0] - want).max())
    err = float(np.abs(got - want).max())
    tol = bound(MEASURED_WORST_BERNOULLI) + bound(MEASURED_FORWARD_SHARE)
    report_measured('test_expectation_is_the_enumerated_posterior forward share', share, bound(MEASURED_FORWARD_SHARE))
    report_measured('test_expectation_is_the_enumerated_posterior max |p - enumerated|', err, tol)
    print('enumerated', want, 'device', got, 'error %.3e, forward share %.3e' % (err, share))
    assert share <= bound(MEASURED_FORWARD_SHARE), share
    assert err <= tol, err
    hid = torch.isnan(row[0]).numpy()
    assert np.abs(var - want * (1.0 - want))[hid].max() <= tol and (var[~hid] == 0).all()
    assert ((want[hid] > 0.02) & (want[hid] < 0.98)).all()                     # (nothing trivially 0 or 1)


def test_mean_of_conditional_samples():
    """4 000 draws of sample_conditional of one row of the padded Gaussian model: their mean within 5 standard errors,
    sqrt(var / n) with var from posterior_moments, of the expectation -- every NaN entry."""
    model, x, _ = make_case('pad')
    model.cuda()
    n = 4000
    row = x[5:6].cuda()
    assert torch.isnan(row).any() and not torch.isnan(row).all()
    mean, var = model.posterior_moments(row)
    draws = model.sample_conditional(row.expand(n, -1).contiguous(), seed=20240611)
    hid = torch.isnan(row[0])
    se = torch.sqrt(var[0].double() / n)
    z = ((draws.double().mean(dim=0) - mean[0].double()) / se)[hid]
    print('in standard errors', z.cpu().numpy())
    assert (z.abs() <= 5.0).all(), z


def test_all_nan_row_is_the_prior():
    """Nothing observed: every activation is log 1 and the moments are the prior's, which the restatement computes from
    all-zero activations; the device's own activations are zero within rounding of logsumexp(log_softmax)."""
    for case in ('pad', 'bernoulli', 'classes_mixture'):
        model, xd, yd, acts, (mean, var, flow), _ = evaluated(case)
        assert torch.isnan(xd[0]).all()
        zeros = [torch.zeros_like(a[:1]) for a in acts]
        pmean, pvar, pflow = mref.restate_model(model, zeros, xd[:1], None if yd is None else yd[:1])
        bern = case == 'bernoulli'
        e_mean = float(np.abs(mean[0].double().cpu().numpy() - pmean[0]).max())
        e_var = float((np.abs(var[0].double().cpu().numpy() - pvar[0]) / (1.0 if bern else pvar[0])).max())
        print('%s: prior mean %.3e var %.3e' % (case, e_mean, e_var))
        assert e_mean <= bound(MEASURED_WORST_BERNOULLI if bern else MEASURED_WORST_MEAN) * (1.0 + np.abs(pmean).max())
        assert e_var <= bound(MEASURED_WORST_BERNOULLI if bern else MEASURED_WORST_VAR)
        assert np.abs(flow[0].double().cpu().numpy() - pflow[0]).max() <= bound(MEASURED_WORST_FLOW)


def test_impossible_evidence_is_nan_in_the_nan_entries_only():
    """Rows whose root maximum is -inf or NaN, by activations of -inf / NaN handed to the launch (the route of
    test_impossible_evidence_falls_to_the_weights; the leaf layers clamp log 0 to the lowest finite float as the reference's
    nan_to_num does, so no evidence reaches this through the public method).  Such a row has NaN in its NaN entries of mean
    and var, its observed entries as given with variance 0, and NaN flows; every other row is bit for bit what it was."""
    model, xd, yd, acts, (mean, var, flow), _ = evaluated('pad')
    bad = torch.zeros(B, dtype=torch.bool, device='cuda')
    bad[2::3] = True
    for fill in (float('-inf'), float('nan')):
        broken = [torch.where(bad[:, None, None], torch.full_like(a, fill), a) for a in acts]
        m, v, f = moments(model, xd, yd, broken)
        hid = torch.isnan(xd)
        assert torch.isnan(m[bad][hid[bad]]).all() and torch.isnan(v[bad][hid[bad]]).all() and torch.isnan(f[bad]).all()
        assert torch.equal(m[bad][~hid[bad]], xd[bad][~hid[bad]]) and (v[bad][~hid[bad]] == 0).all()
        assert torch.equal(m[~bad], mean[~bad]) and torch.equal(v[~bad], var[~bad]) and torch.equal(f[~bad], flow[~bad])


def test_edges():
    """An empty batch; labels out of range; labels of another integer dtype; a label given to a model with one root; the
    optional outputs left out; what is not built."""
    from deeprob.hip import HipError
    from deeprob.spn.models import GaussianRatSpn
    model, xd, yd, acts, (mean, var, flow), _ = evaluated('classes')
    for y in (None, torch.empty(0, dtype=torch.long, device='cuda')):
        m, v = model.posterior_moments(torch.empty(0, 64, device='cuda'), y)
        assert tuple(m.shape) == tuple(v.shape) == (0, 64) and m.is_cuda
    m, v, f = moments(model, xd[:0], None, [a[:0] for a in acts])
    assert tuple(f.shape) == (0,) + tuple(flow.shape[1:])
    for wrong in (3, -1):
        y = yd.clone()
        y[17] = wrong
        with pytest.raises(ValueError, match='labels must lie in'):
            model.posterior_moments(xd, y)
    with pytest.raises(ValueError):
        model.posterior_moments(xd, yd[:5])
    with pytest.raises(ValueError):
        model.posterior_moments(xd[:, :60], yd)
    with pytest.raises(HipError):
        model.posterior_moments(xd.cpu(), yd)
    assert torch.equal(model.expectation(xd, yd.to(torch.int32)), mean)
    # the optional outputs: the same mean bit for bit without them
    m, v, f = moments(model, xd, yd, acts, want_var=False, want_leaf_flow=False)
    assert v is None and f is None and torch.equal(m, mean)
    m, v, f = moments(model, xd, yd, acts, want_var=True, want_leaf_flow=False)
    assert f is None and torch.equal(m, mean) and torch.equal(v, var)
    m, v, f = moments(model, xd, yd, acts, want_var=False, want_leaf_flow=True)
    assert v is None and torch.equal(m, mean) and torch.equal(f, flow)
    # one root: a label changes nothing
    single, x1, _, _, (mean1, var1, _), _ = evaluated('pad')
    m, v = single.posterior_moments(x1, torch.full((B,), 2, device='cuda'))
    assert torch.equal(m, mean1) and torch.equal(v, var1)
    # not built: training-mode dropout, a shape outside the envelope
    drop = GaussianRatSpn(15, rg_depth=2, rg_repetitions=2, rg_batch=2, rg_sum=2, in_dropout=0.2, random_state=1).cuda().train()
    with pytest.raises(NotImplementedError, match='dropout'):
        drop.posterior_moments(x1)
    assert torch.isfinite(drop.eval().expectation(torch.nan_to_num(x1))).all()
    from deeprob.spn.layers.ratspn import RegionGraphLayer
    from deeprob.spn.models import RatSpn

    class MyLeaf(RegionGraphLayer):
        """A leaf family of the user's: neither of the two whose parameters the kernel reads."""
        def _leaf_forward(self, x):
            raise AssertionError('posterior_moments must refuse before it evaluates anything')

        _leaf_forward_dropout = distribution_mode = _leaf_forward

    own = RatSpn(15, MyLeaf, rg_depth=2, rg_repetitions=2, rg_batch=2, rg_sum=2, random_state=1).cuda().eval()
    with pytest.raises(NotImplementedError, match='a user-defined leaf layer'):
        own.posterior_moments(x1)
    big = GaussianRatSpn(40, rg_depth=1, rg_repetitions=2, rg_batch=17, random_state=1).cuda().eval()
    with pytest.raises(NotImplementedError, match='I 17'):
        big.expectation(torch.randn(3, 40, device='cuda'))


def test_determinism_and_the_grid_stride_loop():
    """B = 5000 is more rows than work-groups in the grid (8 a compute unit): row k of the batch is the same row evaluated
    alone, bit for bit, and two calls agree bit for bit."""
    model, xd, yd, _, _, _ = evaluated('classes')
    n = 5000
    gen = torch.Generator(device='cuda').manual_seed(3)
    x = torch.randn(n, 64, device='cuda', generator=gen)
    x[torch.rand(n, 64, device='cuda', generator=gen) < 0.5] = float('nan')
    y = torch.arange(n, device='cuda') % 3
    with torch.no_grad():
        acts = model._upward_for_mpe(x)
    first = moments(model, x, y, acts)
    again = moments(model, x, y, acts)
    for a, b in zip(first, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    hid = torch.isnan(x)
    assert torch.isfinite(first[0]).all() and (first[1][hid] > 0).all() and torch.isfinite(first[2]).all()
    for k in (0, 1, 2047, 2048, 2049, 4095, 4096, 4999):
        alone = moments(model, x[k:k + 1], y[k:k + 1], [a[k:k + 1].contiguous() for a in acts])
        for a, b in zip(first, alone):
            assert torch.equal(a[k:k + 1].view(torch.int32), b.view(torch.int32)), k


@pytest.mark.parametrize('case', ['pad', 'bernoulli'])
def test_buffer_contract(case):
    """Poisoned, guard-banded mean / var / leaf_flow (0xFF, 0x7F): every element written, nothing outside them, and the
    evidence, the labels, the activations, the tables and the leaf parameters bitwise what they were."""
    model, xd, yd, acts, want, _ = evaluated(case)
    logws, src = model._topdown_logw(), model._topdown_src()
    dist, p0, p1 = model._leaf_params()
    from deeprob.hip import rat
    for pattern in PATTERNS:
        with contract(pattern) as c:
            c.frozen(xd, yd, src, p0, p1, *acts, *logws)
            got = c.expect_written(*rat.ratspn_moments(dist, model._fused_ctx, xd, yd, acts, logws, src, p0, p1,
                                                       all_classes=yd is None, want_leaf_flow=True))
            assert len(c.allocations) >= 3
        for g, w in zip(got, want):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32))
