"""RatSpn.posterior_moments without a device: the header and the exports of the sixth library, the argument errors raised
before anything reaches the device, and the restatement the GPU tests compare with (tests/ratspn_moments_ref.py) pinned
against two things that share no code with it: ratios of the float64 oracle's forward, and float64 autograd through it."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import ratspn_oracle as orc
from tests import ratspn_moments_ref as mref
from tests import ratspn_posterior_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ['dpr_abi_version', 'dpr_last_error', 'dpr_ratspn_moments']
PAD_KW = dict(in_features=15, rg_depth=2, rg_repetitions=3, rg_batch=3, rg_sum=5, optimize_scale=True)   # = CASES['pad']
CLASSES_KW = dict(in_features=9, out_classes=3, rg_depth=2, rg_repetitions=2, rg_batch=2, rg_sum=3)
AGREE = 1e-9


# ---- the header and the library --------------------------------------------------------------------------------------------
def test_rat_header_parses_and_declares_its_entry_points_once():
    from deeprob import hip
    from deeprob.hip import rat
    text = open(os.path.join(ROOT, 'include', 'deeprob_rat.h')).read()
    sigs, consts, structs = hip.parse_header(text, prefix='dpr', header='deeprob_rat.h')
    assert sigs == rat.SIGNATURES and not structs
    assert sorted(sigs) == ENTRY_POINTS
    assert consts['DPR_OK'] == 0 and consts['DPR_EINVAL'] == -1 and consts['DPR_EUNSUPPORTED'] == -2
    assert consts['DPR_DIST_GAUSSIAN'] == 0 and consts['DPR_DIST_BERNOULLI'] == 1 and consts['DPR_MAX_DEPTH'] == 10
    declared = re.findall(r'\b(dpr_\w+)\s*\(', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    assert sorted(declared) == sorted(set(declared)) == sorted(sigs), 'every entry point is declared once'
    assert len(sigs['dpr_ratspn_moments'][1]) == 21


def test_missing_rat_library_and_header_raise(monkeypatch):
    from deeprob.hip import HipError, rat
    monkeypatch.setattr(rat, '_lib', None)
    monkeypatch.setattr(rat, 'LIB_PATH', os.path.join(ROOT, 'no', 'such', 'libdeeprob_rat.so'))
    with pytest.raises(HipError) as e:
        rat.load_library()
    assert 'make -C deeprob-kit_amd/csrc' in str(e.value)
    monkeypatch.setattr(rat, 'HEADER_PATH', os.path.join(ROOT, 'no', 'such', 'deeprob_rat.h'))
    with pytest.raises(HipError, match='deeprob_rat.h'):
        rat._read_header()


def _raw(lib, **over):
    """dpr_ratspn_moments on null tables with the sizes of a small model, some overridden: what the entry point says before
    it touches a pointer or the device."""
    kw = dict(dist=0, B=0, D=15, depth=2, reps=3, I=3, S=5, C=1, d=4)
    kw.update(over)
    return lib.dpr_ratspn_moments(kw['dist'], kw['B'], kw['D'], kw['depth'], kw['reps'], kw['I'], kw['S'], kw['C'], kw['d'],
                                  None, None, 0, None, None, None, None, None, None, None, None, None)


def test_bad_sizes_are_reported_by_the_raw_handle():
    from deeprob.hip import rat
    lib = rat.load_library()
    assert _raw(lib) == rat.DPR_OK                                  # (B = 0: nothing to do, nothing launched)
    for over in (dict(dist=2), dict(B=-1), dict(D=0), dict(depth=0), dict(reps=0), dict(I=0), dict(S=-3), dict(C=0), dict(d=0)):
        assert _raw(lib, **over) == rat.DPR_EINVAL, over
        assert b'ratspn_moments' in lib.dpr_last_error()
    assert _raw(lib, B=4) == rat.DPR_EINVAL and b'null pointer' in lib.dpr_last_error()
    # outside the envelope: the sizes are in the text
    assert _raw(lib, depth=11, D=4096) == rat.DPR_EUNSUPPORTED and b'depth 11' in lib.dpr_last_error()
    assert _raw(lib, S=17) == rat.DPR_EUNSUPPORTED and b'S 17' in lib.dpr_last_error()
    assert _raw(lib, depth=10, I=16, S=16, D=20000) == rat.DPR_EUNSUPPORTED and b'bytes of LDS' in lib.dpr_last_error()
    # the envelope the kernel promises: any depth <= 10 with I, S <= 16
    assert _raw(lib, depth=10, I=16, S=16, D=1024, d=1) == rat.DPR_OK
    assert _raw(lib, depth=2, I=16, S=16, D=784, reps=8, d=196) == rat.DPR_OK


def test_argument_errors_need_no_device():
    """A CPU tensor raises HipError (no silent fallback); training-mode dropout and a user-defined leaf layer are not built
    and say so in the words of sample_conditional."""
    from deeprob.hip import HipError
    from deeprob.spn.layers.ratspn import RegionGraphLayer
    from deeprob.spn.models import GaussianRatSpn, RatSpn
    model = GaussianRatSpn(random_state=4, **PAD_KW).eval()
    x = torch.randn(3, 15)
    for method in (model.posterior_moments, model.expectation, model.variance):
        with pytest.raises(HipError):
            method(x)
    for kw in (dict(in_dropout=0.2), dict(sum_dropout=0.2)):
        drop = GaussianRatSpn(random_state=4, **dict(PAD_KW, **kw)).train()
        with pytest.raises(NotImplementedError, match='training mode with in_dropout / sum_dropout set'):
            drop.expectation(x)
        with pytest.raises(HipError):
            drop.eval().expectation(x)

    class MyLeaf(RegionGraphLayer):
        """A leaf family of the user's: neither of the two whose parameters the kernel reads."""
        def _leaf_forward(self, x):
            raise AssertionError('posterior_moments must refuse before it evaluates anything')

        _leaf_forward_dropout = distribution_mode = _leaf_forward

    own = RatSpn(15, MyLeaf, rg_depth=2, rg_repetitions=2, rg_batch=2, rg_sum=2, random_state=1).eval()
    for method in (own.posterior_moments, own.expectation, own.variance):
        with pytest.raises(NotImplementedError, match='a user-defined leaf layer'):
            method(x)


# ---- the restatement against the oracle ------------------------------------------------------------------------------------
def _sd64(model):
    return {k: (v.detach().double() if v.is_floating_point() else v.detach().clone()) for k, v in model.state_dict().items()}


def _restate64(model, sd64, x, y=None, all_classes=None):
    depth = model.rg_depth
    acts = pref.host_activations(sd64, x.double(), depth)
    dist, p0, p1 = model._leaf_params()
    logws = [w.detach() for w in model.double()._topdown_logw()]
    if all_classes is None:
        all_classes = y is None
    return mref.posterior_moments([a.double() for a in acts], logws, model._topdown_src(),
                                  (dist, p0.detach().double(), None if p1 is None else p1.detach().double()), x.double(), y,
                                  all_classes)


def _log_evidence(sd64, x, y, all_classes):
    """log p(e) of every row under the class / the mixture of classes the moments are asked for."""
    out = orc.ratspn_forward(sd64, x.double())
    if y is not None:
        return out[torch.arange(x.shape[0]), y]
    return torch.logsumexp(out, dim=1) if all_classes else out[:, 0]


def _bernoulli_ratio_check(model, x, y):
    sd64 = _sd64(model)
    mean, var, _ = _restate64(model, sd64, x, y)
    base = _log_evidence(sd64, x, y, True)
    checked = 0
    for b in range(x.shape[0]):
        for f in torch.isnan(x[b]).nonzero().flatten().tolist():
            one = x[b:b + 1].clone()
            one[0, f] = 1.0
            p = float(torch.exp(_log_evidence(sd64, one, None if y is None else y[b:b + 1], True) - base[b]))
            assert abs(mean[b, f] - p) <= AGREE and abs(var[b, f] - p * (1.0 - p)) <= AGREE, (b, f, mean[b, f], p)
            checked += 1
    obs = ~torch.isnan(x)
    assert np.array_equal(mean[obs.numpy()], x[obs].double().numpy()) and (var[obs.numpy()] == 0.0).all()
    return checked


def test_restatement_is_the_forward_ratio_bernoulli():
    """p(x_f = 1 | e) = p(x_f = 1, e) / p(e) from the float64 oracle, for every NaN entry: the enumerable model, and a
    model with three classes with labels and without (the mixture over classes under the uniform prior)."""
    model, row, _, _ = pref.enumerable_case()
    x = torch.cat([row, torch.full((1, 6), float('nan')), torch.tensor([[float('nan'), 1.0, 1.0, 0.0, float('nan'), 0.0]])])
    assert _bernoulli_ratio_check(model, x, None) == 3 + 6 + 2
    from deeprob.spn.models import BernoulliRatSpn
    torch.manual_seed(5)
    model = BernoulliRatSpn(random_state=6, **CLASSES_KW).eval()
    with torch.no_grad():
        model.base_layer.logits.copy_(1.5 * torch.randn(model.base_layer.logits.shape, generator=torch.Generator().manual_seed(7)))
    gen = torch.Generator().manual_seed(8)
    x = (torch.rand(4, 9, generator=gen) < 0.5).float()
    x[torch.rand(4, 9, generator=gen) < 0.5] = float('nan')
    assert _bernoulli_ratio_check(model, x, torch.tensor([0, 1, 2, 1])) > 8
    assert _bernoulli_ratio_check(model, x, None) > 8
    # (class 0 alone is another answer than the mixture: the root of the all-classes pass is what was checked)
    m0 = _restate64(model, _sd64(model), x, None, all_classes=False)[0]
    ma = _restate64(model, _sd64(model), x, None, all_classes=True)[0]
    assert np.nanmax(np.abs(m0 - ma)) > 1e-3


def _pad_case():
    from deeprob.spn.models import GaussianRatSpn
    torch.manual_seed(21)
    model = GaussianRatSpn(random_state=4, **PAD_KW).eval()
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(3, 15, generator=gen)
    x[torch.rand(3, 15, generator=gen) < 0.5] = float('nan')
    x[2, 1:] = float('nan')
    return model, x


def test_restatement_is_the_quadrature_gaussian():
    """E[x_f | e] and Var[x_f | e] by trapezoid quadrature of t^k p(t, e) on the float64 oracle over loc +- 12 scale of the
    variable's channels, with a step of a third of the smallest scale (the trapezoid rule on a mixture of Gaussians converges
    geometrically: the error at this step is far below 1e-9)."""
    model, x = _pad_case()
    sd64 = _sd64(model)
    mean, var, _ = _restate64(model, sd64, x)
    src = model._topdown_src().long()
    base = model.base_layer
    d = base.dimension
    G0 = 1 << model.rg_depth
    checked = 0
    for b in range(x.shape[0]):
        for f in torch.isnan(x[b]).nonzero().flatten().tolist():
            locs, scales = [], []
            for rep in range(src.shape[0]):
                rl, j = int(src[rep, f]) // d, int(src[rep, f]) % d
                locs.append(sd64['base_layer.loc'][rep * G0 + rl, :, j])
                scales.append(sd64['base_layer.scale'][rep * G0 + rl, :, j])
            locs, scales = torch.cat(locs), torch.cat(scales)
            lo, hi = float((locs - 12.0 * scales).min()), float((locs + 12.0 * scales).max())
            n = int(np.ceil((hi - lo) / (float(scales.min()) / 3.0))) + 1
            t = torch.linspace(lo, hi, n, dtype=torch.float64)
            rows = x[b:b + 1].double().repeat(n, 1)
            rows[:, f] = t
            ll = orc.ratspn_forward(sd64, rows)[:, 0]
            p = torch.exp(ll - ll.max())
            z = torch.trapezoid(p, t)
            e1 = float(torch.trapezoid(p * t, t) / z)
            e2 = float(torch.trapezoid(p * (t - e1) ** 2, t) / z)
            assert abs(mean[b, f] - e1) <= AGREE * (1.0 + abs(e1)) and abs(var[b, f] - e2) <= AGREE * (1.0 + e2), \
                (b, f, mean[b, f], e1, var[b, f], e2)
            checked += 1
    assert checked >= 14 + 5


@pytest.mark.parametrize('case', ['pad', 'classes_labels', 'classes_mixture'])
def test_leaf_flow_is_the_gradient_of_the_log_evidence(case):
    """d log p(e) / d (leaf activation), by float64 autograd through the oracle's forward, is leaf_flow."""
    if case == 'pad':
        model, x = _pad_case()
        y = None
        param = 'base_layer.loc'
    else:
        from deeprob.spn.models import BernoulliRatSpn
        torch.manual_seed(5)
        model = BernoulliRatSpn(random_state=6, **CLASSES_KW).eval()
        gen = torch.Generator().manual_seed(8)
        x = (torch.rand(4, 9, generator=gen) < 0.5).float()
        x[torch.rand(4, 9, generator=gen) < 0.5] = float('nan')
        y = torch.tensor([0, 1, 2, 1]) if case == 'classes_labels' else None
        param = 'base_layer.logits'
    sd64 = _sd64(model)
    _, _, flow = _restate64(model, sd64, x, y)
    sd64[param].requires_grad_(True)                               # (so that the leaf activations are part of the graph)
    out, acts = orc.ratspn_forward(sd64, x.double(), return_activations=True)
    if y is not None:
        ll = out[torch.arange(x.shape[0]), y]
    else:
        ll = torch.logsumexp(out, dim=1)
    grad, = torch.autograd.grad(ll.sum(), acts['leaf'])
    assert flow.shape == tuple(grad.shape)
    assert np.abs(flow - grad.numpy()).max() <= AGREE
    # every region of every repetition receives the repetition's share: the flows of a row sum to 2^depth
    assert np.allclose(flow.sum(axis=(1, 2)), float(1 << model.rg_depth), atol=1e-9)
