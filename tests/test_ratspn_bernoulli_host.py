"""The references of tests/test_ratspn_bernoulli_gpu.py, pinned on the host before any device run: the case table, the float64
oracle on every (case, evidence kind), the masked reference gradient, and the numpy restatement of the MPE top-down pass
(tests/ratspn_mpe_ref.py) against the oracle's own."""
import numpy as np
import pytest
import torch

from oracle import ratspn_oracle as orc
from tests import ratspn_bernoulli_cases as bc
from tests.ratspn_mpe_ref import mpe_replay
from tests.ratspn_posterior_ref import host_activations
from tests.util import grad_err

# the five models of test_ratspn_gpu.py::test_mpe_vs_oracle_padded_and_deep
MPE_CASES = [dict(in_features=15, rg_depth=2, rg_repetitions=3, rg_batch=3, rg_sum=5, optimize_scale=True),
             dict(in_features=15, rg_depth=3, rg_repetitions=2, rg_batch=2, rg_sum=2),
             dict(in_features=70, out_classes=4, rg_depth=4, rg_repetitions=3, rg_batch=5, rg_sum=3),
             dict(in_features=784, rg_depth=2, rg_repetitions=8, rg_batch=16, rg_sum=16),
             dict(in_features=33, rg_depth=5, rg_repetitions=2, rg_batch=2, rg_sum=2)]


def mpe_case(kw, B=300):
    """Model (host), evidence and labels of test_mpe_vs_oracle_padded_and_deep."""
    from deeprob.spn.models import GaussianRatSpn
    torch.manual_seed(5)
    model = GaussianRatSpn(random_state=9, **kw).eval()
    D = kw['in_features']
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(B, D, generator=gen)
    x[torch.rand(B, D, generator=gen) < 0.5] = float('nan')
    x[0] = float('nan')
    y = (torch.arange(B) % kw['out_classes']) if kw.get('out_classes', 1) > 1 else None
    return model, x, y


@pytest.mark.parametrize('name', sorted(bc.CASES))
def test_case_table(name):
    """make_model asserts R / d / pad of the table; the logits are as documented."""
    model = bc.make_model(name)
    lg = model.base_layer.logits.detach()
    assert (lg == 0).sum().item() >= 1 and (lg.abs() == 40).sum().item() >= 2
    assert ((lg != 0) & (lg.abs() < 1e-3)).sum().item() == 0
    again = bc.make_model(name)
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), again.state_dict().values()))


def test_many_groups_reaches_several_passes():
    assert bc.staged_passes('many_groups', 1024) >= 2
    # the staged kernel's other conditions for this case: tile rows within 80 KB of LDS
    kw = bc.CASES['many_groups'][0]
    assert 16 * (kw['in_features'] + 64 * 1) * 4 <= 80 * 1024


@pytest.mark.parametrize('kind', ['binary', 'nan', 'soft'])
@pytest.mark.parametrize('name', [n for n in sorted(bc.CASES) if n != 'two_per_lane'])
def test_oracle_ll_is_finite(name, kind):
    model = bc.make_model(name)
    x = bc.make_evidence(name, 300, kind)
    ll = orc.ratspn_forward(bc.sd64(model), x.double())
    planted = bc.inf_row_mask(x)
    assert planted.sum().item() == (2 if kind == 'nan' else 0)
    assert torch.isfinite(ll[~planted]).all()
    if kind == 'nan':
        assert ll[0].abs().max().item() < 1e-9           # the all-NaN row: log 1
        assert not torch.isnan(x[1]).any()


@pytest.mark.parametrize('name', ['pad2', 'wide16_d1'])
def test_masked_reference_grads(name):
    model = bc.make_model(name)
    sd = bc.sd64(model)
    y = bc.labels(name, 50)
    x = bc.make_evidence(name, 50, 'soft')
    plain = bc.reference_grads(sd, x, y)
    masked = bc.masked_reference_grads(sd, x, torch.zeros_like(x, dtype=torch.bool), y=y)
    assert sorted(plain) == sorted(masked)
    for k in plain:
        assert np.array_equal(plain[k], masked[k]), k
    # 20 % NaN: the reference's own backward computes 0 * NaN (the documented quirk); the masked gradient is finite, and 0 in
    # the marginalised entries of x
    xn = bc.make_evidence(name, 50, 'nan', inf_rows=False)
    nan_mask = torch.isnan(xn)
    assert abs(nan_mask[2:].float().mean().item() - 0.2) < 0.05
    plain = bc.reference_grads(sd, xn, y)
    assert np.isnan(plain['base_layer.logits']).any()    # ((sigmoid(l) - NaN) * 0; d/dx = l * 0 stays finite for these leaves)
    masked = bc.masked_reference_grads(sd, xn, nan_mask, y=y)
    assert all(np.isfinite(v).all() for v in masked.values())
    assert (masked['x'][nan_mask.numpy()] == 0).all()
    # and it is the gradient of the same function: a central difference in one observed entry of x and one logit
    def ll_sum(sd_, x_):
        return orc.ratspn_loss(orc.ratspn_forward(sd_, x_), y).item()
    obs = (~nan_mask).nonzero()[7]
    h = 1e-6
    xp, xm = xn.double().clone(), xn.double().clone()
    xp[obs[0], obs[1]] += h
    xm[obs[0], obs[1]] -= h
    fd = (ll_sum(sd, xp) - ll_sum(sd, xm)) / (2 * h)
    assert abs(fd - masked['x'][obs[0], obs[1]]) <= 1e-6 * max(1.0, np.abs(masked['x']).max())


def test_sample_replay_leaves_few_rows_aside():
    """The device test of sampling at width judges the rows whose categorical draws clear a CDF step by 3e-6 and asks for at
    least 97 % of them: what the oracle's replay gives for that model and seed, before any device run."""
    model = bc.make_model('mnist8')
    _, _, _, margin = orc.ratspn_sample_replay(bc.sd_as(model, torch.float32), 5000, 2, 784, seed=987654321)
    assert (margin > 3e-6).mean() >= 0.99


@pytest.mark.parametrize('case', list(range(len(MPE_CASES))) + ['mnist8'])
def test_mpe_replay_is_the_oracles_mpe(case):
    """mpe_replay fed with the ORACLE's float32 activations makes the oracle's choices on every row."""
    if case == 'mnist8':
        model = bc.make_model('mnist8')
        x = bc.make_evidence('mnist8', 300, 'nan', nan_frac=0.5, inf_rows=False)
        y = None
    else:
        model, x, y = mpe_case(MPE_CASES[case])
    depth = model.rg_depth
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    want, og, oo = orc.ratspn_mpe(sd, x, depth, y=y, return_choice=True)
    with torch.no_grad():
        got, rep, chan = mpe_replay(host_activations(sd, x, depth), model._topdown_logw(), model._topdown_src(),
                                    model._leaf_params(), x, y)
    assert torch.equal(rep, torch.div(og[:, 0], 2 ** depth, rounding_mode='floor'))
    assert torch.equal(chan, oo)
    assert torch.equal(got, want)
