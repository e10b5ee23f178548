"""Posterior queries on node-graph SPNs on the HIP path (deeprob.spn.algorithms.moments, inference.posterior /
likelihood; dpq_flat_spn_posterior) against the float64 oracle of tests/flat_spn_posterior_ref.py (ratios of forward
evaluations, no backward pass) and the reference's goldens (tools/gen_golden_spn_moments.py).

The error of an entry is ``|got - want| / max(1, scale)`` with the oracle's ``scale = sum_L r_L |m_k(L)|``: the size of the
terms the entry is a sum of, which covers odd moments whose leaf terms cancel.  No row is set aside.  MEASURED is the worst
case over every case of this file on an MI355X (DESIGN.md section 13.1 has the table); the bar is four times that, the
factor DESIGN.md section 14.2 allows for other inputs rounding differently."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import flat_spn_posterior_cases as pc
from tests import flat_spn_posterior_ref as pref
from tests.buffer_contract import contract
from tests.util import report_measured

pytestmark = pytest.mark.gpu

GOLD = pc.GOLD
MEASURED = 2.31e-6       # worst |got - want| / max(1, scale) over all cases below, moments and value probabilities alike
BAR = 4 * MEASURED
assert BAR <= 1e-5      # (the arithmetic is eval_backward's, held to 1e-5: above it there is a bug to find)
F32 = float(np.finfo(np.float32).eps)


def _spn(name):
    from deeprob.spn.structure.io import digraph_to_spn
    return digraph_to_spn(pc.circuit(name)[0])


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def _launch(spn, x, **kw):
    from deeprob.hip import spnq
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(_device())
    out = spnq.flat_spn_posterior(spn, xd, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _scope(spn, D):
    from deeprob.hip import spnq
    off, _ = spnq.leaf_table(spn)
    scope = np.zeros(D, bool)
    scope[:spn.n_features] = np.diff(off) > 0
    return scope


def _error(got, want, scale):
    """Worst |got - want| / max(1, scale); the NaN patterns must be equal."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), 'the NaN pattern differs from the oracle'
    live = ~np.isnan(want)
    if not live.any():
        return 0.0
    return float(np.max(np.abs(got[live].astype(np.float64) - want[live]) / np.maximum(1.0, scale[live])))


# ---- mode 0: moments ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', pc.BATCHES)
@pytest.mark.parametrize('name', pc.CIRCUITS)
def test_moments_against_the_oracle(name, B):
    from deeprob.hip import spnq
    spn = _spn(name)
    x = pc.inputs(name)[:B]
    want, scale = (a[:, :B] for a in pc.oracle_moments(name))
    rec = spn.circuit(_device())
    on_chip = spnq.load_library().dpq_flat_spn_posterior_workspace_bytes(B, ctypes.addressof(rec), 0) == 0
    assert on_chip == pc.ON_CHIP[name]
    got = _launch(spn, x, mode=spnq.DPQ_MODE_MOMENTS, n_orders=4)
    assert got.shape == (4, B, x.shape[1]) and got.dtype == np.float32
    # both routes and two calls give the same bytes
    assert np.array_equal(_bits(_launch(spn, x, mode=spnq.DPQ_MODE_MOMENTS, n_orders=4, force_workspace=True)), _bits(got))
    assert np.array_equal(_bits(_launch(spn, x, mode=spnq.DPQ_MODE_MOMENTS, n_orders=4)), _bits(got))
    # observed and out-of-scope entries, bit for bit
    scope = _scope(spn, x.shape[1])
    assert scope[:spn.n_features].all() and not scope[spn.n_features:].any()
    seen = ~np.isnan(x) & scope[None, :]
    power = x.copy()
    for k in range(4):
        assert np.array_equal(_bits(got[k][:, ~scope]), _bits(x[:, ~scope])), 'outside the scope: as given'
        assert np.array_equal(_bits(got[k][seen]), _bits(power[seen])), 'observed: x^%d' % (k + 1)
        with np.errstate(over='ignore', invalid='ignore'):
            power = power * x
    # zero-probability rows are in the case, and NaN exactly where the oracle has NaN
    dead = np.isnan(want[0][:, scope]) & np.isnan(x[:, scope])
    if B >= 3:
        assert dead[1].any() and dead[2].any()
    err = _error(got, want, scale)
    print('moments %-9s B %3d  err %.3e  (%s)' % (name, B, err, 'on chip' if on_chip else 'workspace'))
    report_measured('flat_spn_posterior moments %s B=%d' % (name, B), err, BAR)
    assert err <= BAR
    # fewer orders: the same planes
    if B == 65:
        for K in (1, 2, 3):
            assert np.array_equal(_bits(_launch(spn, x, mode=spnq.DPQ_MODE_MOMENTS, n_orders=K)), _bits(got[:K]))


def _stat_tolerance(f, m, scale):
    """First-order bound on the error of statistic f(m) when moment k is off by BAR * max(1, scale_k) (central
    differences in float64), plus the float32 rounding of the result and of the moments it is formed from."""
    base = f(m)
    tol = 4 * F32 * np.abs(base)
    for k in range(len(m)):
        h = 1e-6 * np.maximum(1.0, scale[k])
        up, dn = [a.copy() for a in m], [a.copy() for a in m]
        up[k] = up[k] + h
        dn[k] = dn[k] - h
        with np.errstate(invalid='ignore', divide='ignore'):
            slope = np.abs(f(up) - f(dn)) / (2 * h)
        tol = tol + 2 * slope * (BAR + F32) * np.maximum(1.0, scale[k])
    return base, tol


@pytest.mark.parametrize('name', pc.CIRCUITS)
def test_variance_skewness_kurtosis_against_the_oracle(name):
    from deeprob.spn.algorithms import moments as mom
    spn = _spn(name)
    x = np.array(pc.inputs(name)[:65])
    want, scale = (a[:, :65] for a in pc.oracle_moments(name))
    scope = _scope(spn, x.shape[1])
    nan = np.isnan(x) & scope[None, :]
    live = nan & ~np.isnan(want[0])
    seen = ~np.isnan(x) & scope[None, :]
    for fn, n, pick, point in ((mom.variance, 2, 0, 0.0), (mom.skewness, 3, 1, np.nan), (mom.kurtosis, 4, 2, np.nan)):
        got = fn(spn, x)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == x.shape
        base, tol = _stat_tolerance(lambda m: pref.statistics(list(m) + [m[0]] * (4 - len(m)))[pick],
                                    [want[k] for k in range(n)], [scale[k] for k in range(n)])
        # no entry is set aside: where the oracle's statistic is finite it is compared, and where it is not (0 / 0 or
        # x / 0 of a degenerate posterior, variance 0) the result is not finite either; the variance is always finite
        usable = live & np.isfinite(base)
        assert np.isfinite(tol[usable]).all()
        assert not np.isfinite(got[live & ~usable]).any()
        if fn is mom.variance:
            assert np.array_equal(usable, live)
        excess = np.abs(got[usable].astype(np.float64) - base[usable]) / tol[usable]
        print('%-9s %-9s worst error / tolerance %.3f over %d entries' % (fn.__name__, name, excess.max(), usable.sum()))
        assert excess.max() <= 1.0
        assert np.isnan(got[nan & ~live]).all()
        assert np.array_equal(got[seen], np.full(int(seen.sum()), point, np.float32), equal_nan=True)
        assert np.array_equal(_bits(got[:, ~scope]), _bits(x[:, ~scope]))
        t = fn(spn, torch.from_numpy(x).to(_device()))
        assert isinstance(t, torch.Tensor) and t.is_cuda and np.array_equal(_bits(t.cpu().numpy()), _bits(got))
    # moment / expectation are the planes of the four-order launch, bit for bit
    from deeprob.hip import spnq
    planes = _launch(spn, x, mode=spnq.DPQ_MODE_MOMENTS, n_orders=4)
    assert np.array_equal(_bits(mom.expectation(spn, x)), _bits(planes[0]))
    for k in (1, 2, 3, 4):
        assert np.array_equal(_bits(mom.moment(spn, k, x)), _bits(planes[k - 1]))
    assert np.array_equal(mom.moment(spn, 0, torch.from_numpy(x).to(_device())).cpu().numpy(), np.ones_like(x))


@pytest.mark.parametrize('name', ['binary16', 'mixed4'])
def test_unconditional_moments_match_the_reference(name):
    """Without x: [n_features] float32, the reference's numbers (its float32 results: 1e-6 of the scale beside BAR); the
    skewness is the standard one formed from the golden raw moments, not the reference's."""
    from deeprob.spn.algorithms import moments as mom
    g = np.load(os.path.join(GOLD, 'spn_moments.npz'))
    spn = _spn(name)
    raw = [g['%s.moment%d' % (name, k)].astype(np.float64) for k in (1, 2, 3, 4)]
    _, scale = pc.oracle_moments(name)
    scale = scale[:, 0, :spn.n_features]            # row 0 is all NaN
    for k in (1, 2, 3, 4):
        got = mom.moment(spn, k)
        assert got.dtype == np.float32 and got.shape == (spn.n_features,)
        err = float(np.max(np.abs(got - raw[k - 1]) / np.maximum(1.0, scale[k - 1])))
        print('moment %d %-9s err vs reference %.3e' % (k, name, err))
        assert err <= BAR + 1e-6
    assert np.array_equal(mom.expectation(spn), mom.moment(spn, 1))
    assert np.array_equal(mom.expectation(spn), mom.expectation(spn, np.full((1, spn.n_features), np.nan, np.float32))[0])
    var, skew, kurt = pref.statistics(raw)
    for fn, want, n, pick in ((mom.variance, g[name + '.variance'], 2, 0), (mom.skewness, skew, 3, 1),
                              (mom.kurtosis, g[name + '.kurtosis'], 4, 2)):
        got = fn(spn)
        assert got.dtype == np.float32 and got.shape == (spn.n_features,)
        # the golden raw moments are float32 themselves: their rounding enters through the same first-order bound
        _, tol = _stat_tolerance(lambda m: pref.statistics(list(m) + [m[0]] * (4 - len(m)))[pick], raw[:n], list(scale[:n]))
        assert np.max(np.abs(got - want) / tol) <= 2.0, fn.__name__
    if name == 'binary16':      # the deviation from the reference, on the variable the issue names: mean 0.47, nearly symmetric
        assert abs(mom.expectation(spn)[0] - 0.4727) < 1e-3 and abs(mom.skewness(spn)[0]) < 0.2


# ---- mode 1: the posterior of one variable ---------------------------------------------------------------------------------
@pytest.mark.parametrize('B', pc.BATCHES)
@pytest.mark.parametrize('name', pc.CIRCUITS)
def test_posterior_against_the_oracle_and_the_forward_pass(name, B):
    from deeprob.hip import spnq
    from deeprob.spn.algorithms.inference import posterior, log_likelihood
    spn = _spn(name)
    x = np.array(pc.inputs(name)[:B])
    for var in pc.discrete_variables(name):
        values, want = pc.oracle_posterior(name, var)
        want = want[:B]
        got = posterior(spn, x, var)
        assert got.dtype == np.float32 and got.shape == (B, len(values))
        assert np.array_equal(_bits(posterior(spn, x, var, values=values)), _bits(got)), 'the default values'
        assert np.array_equal(_bits(posterior(spn, x, var)), _bits(got)), 'two calls'
        forced = _launch(spn, x, mode=spnq.DPQ_MODE_VALUES, var=var, values=values, force_workspace=True)
        assert np.array_equal(_bits(forced), _bits(got)), 'both routes'
        err = _error(got, want, np.ones_like(want))
        print('posterior %-9s var %2d B %3d  err %.3e' % (name, var, B, err))
        report_measured('flat_spn_posterior values %s var=%d B=%d' % (name, var, B), err, BAR)
        assert err <= BAR
        live = ~np.isnan(got[:, 0])
        assert np.max(np.abs(got[live].astype(np.float64).sum(axis=1) - 1.0), initial=0.0) <= len(values) * F32
        seen = live & ~np.isnan(x[:, var])
        assert np.array_equal(got[seen], (values[None, :] == x[seen, var][:, None]).astype(np.float32))
        # a value outside every support, and the order of `values` is the caller's
        more = np.concatenate([values[::-1], [41.0]]).astype(np.float32)
        again = posterior(spn, x, var, values=more)
        assert np.array_equal(_bits(again[:, :-1]), _bits(got[:, ::-1]))
        assert np.array_equal(again[live, -1], np.zeros(int(live.sum()), np.float32))
        # an independent device-side check: the softmax over `values` of log_likelihood with var set to each value.
        # The forward pass is held to 1e-5 max(1, |ll|) (tests/test_flat_spn_gpu.py), twice that in a difference of two.
        ask = live & np.isnan(x[:, var])
        if ask.any():
            lls = []
            for v in values:
                xv = x[ask].copy()
                xv[:, var] = v
                lls.append(log_likelihood(spn, xv).astype(np.float64))
            lls = np.stack(lls, axis=1)
            soft = np.exp(lls - lls.max(axis=1, keepdims=True))
            soft /= soft.sum(axis=1, keepdims=True)
            tol = 2e-5 * np.maximum(1.0, np.abs(lls).max(axis=1, keepdims=True)) + BAR
            assert (np.abs(got[ask] - soft) <= tol).all()
    t = posterior(spn, torch.from_numpy(x).to(_device()), pc.discrete_variables(name)[0])
    assert isinstance(t, torch.Tensor) and t.is_cuda
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(posterior(spn, x, pc.discrete_variables(name)[0])))


@pytest.mark.parametrize('pattern', [0xFF, 0x7F])
@pytest.mark.parametrize('name', ['mixed4', 'random5'])
def test_posterior_writes_exactly_its_output(name, pattern):
    """Mode 1 on guard-banded, poisoned memory (both routes: mixed4 on chip, random5 through the workspace): every element
    of [B, V] written, nothing outside it, the inputs untouched."""
    from deeprob.spn.algorithms.inference import posterior
    from deeprob.spn.algorithms.moments import kurtosis
    spn = _spn(name)
    var = pc.discrete_variables(name)[0]
    xd = torch.from_numpy(np.array(pc.inputs(name)[:65])).to(_device())
    want = posterior(spn, xd, var)
    with contract(pattern, record=False) as c:
        c.frozen(xd)
        got = c.expect_written(posterior(spn, xd, var))
        assert got.shape == want.shape
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want.cpu().numpy()))
    planes = kurtosis(spn, xd)
    with contract(pattern, record=False) as c:
        c.frozen(xd)
        again = kurtosis(spn, xd)
    assert np.array_equal(_bits(again.cpu().numpy()), _bits(planes.cpu().numpy()))


def test_classifier_posterior_gives_the_class_frequencies():
    """learn_classifier on small discrete data, three classes (the data of tests/test_learnspn_gpu.py::test_classifier):
    the root is a sum over the classes weighted by their frequencies, so on an all-NaN query the class posterior is the
    class frequency of the training rows; with the features observed its argmax classifies, and -- what mpe cannot
    give -- the rows are probabilities."""
    from deeprob.spn.learning import learn_classifier
    from deeprob.spn.algorithms.inference import posterior
    from tests.test_learnspn_gpu import classifier_data, spec
    data, ks = classifier_data()
    dists, doms, _, _ = spec(ks)
    flat = learn_classifier(data, dists, doms, class_idx=-1, verbose=False, split_rows='random', split_cols='gvs',
                            min_rows_slice=64, random_state=0)
    class_idx = data.shape[1] - 1
    freq = np.bincount(data[:, -1].astype(int), minlength=3) / len(data)
    query = data[:64].copy()
    query[:, -1] = np.nan
    query[0, :] = np.nan
    got = posterior(flat, query, class_idx)
    assert got.shape == (64, 3) and got.dtype == np.float32
    print('class posterior', got[0], 'frequencies', freq)
    assert np.abs(got[0] - freq).max() <= 1e-6 + BAR            # (the weights are the frequencies to 1e-6, as that test holds)
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() <= 3 * F32
    assert np.mean(np.argmax(got[1:], axis=1) == data[1:64, -1]) >= 0.9


def test_likelihood_on_the_device():
    from deeprob.spn.algorithms.inference import likelihood, log_likelihood
    spn = _spn('mixed4')
    x = np.array(pc.inputs('mixed4')[:65, :4])
    ll = log_likelihood(spn, x)
    got = likelihood(spn, x)
    assert got.dtype == np.float32 and np.array_equal(got, np.exp(ll)) and (got[ll <= -1e30] == 0).all()
    a, table = likelihood(spn, x, return_results=True)
    assert np.array_equal(a, got) and table.shape == (spn.n_nodes, 65)
    t = likelihood(spn, torch.from_numpy(x).to(_device()))
    assert isinstance(t, torch.Tensor) and t.is_cuda and np.allclose(t.cpu().numpy(), got, rtol=1e-6, atol=0)
