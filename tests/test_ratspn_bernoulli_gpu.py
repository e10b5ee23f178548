"""BernoulliRatSpn on the HIP path across the envelope of its kernels (tests/ratspn_bernoulli_cases.py: which case reaches
which DIST = 1 instantiation), against the oracle in float64: forward (model and leaf layer alone), backward (every parameter
and the evidence), and the top-down passes (MPE pinned row by row through tests/ratspn_mpe_ref.py, sampling replayed)."""
import functools

import numpy as np
import pytest
import torch

from oracle import ratspn_oracle as orc
from tests import ratspn_bernoulli_cases as bc
from tests.ratspn_mpe_ref import mpe_replay
from tests.ratspn_posterior_ref import host_activations
from tests.util import rel_err, grad_err, report_measured

pytestmark = pytest.mark.gpu

LL_TOL = 1e-5     # the project's bar: 1e-5 relative on fp32 log-likelihoods
GRAD_TOL = 1e-4   # relative to the largest magnitude of the tensor

FWD_CASES = [n for n in sorted(bc.CASES) if n != 'two_per_lane']


@functools.lru_cache(maxsize=None)
def host_model(name):
    return bc.make_model(name)


@functools.lru_cache(maxsize=None)
def device_model(name):
    return bc.make_model(name).cuda()


@functools.lru_cache(maxsize=None)
def state64(name):
    return bc.sd64(host_model(name))


# ---- forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['binary', 'nan', 'soft'])
@pytest.mark.parametrize('B', [1, 63, 65, 300])
@pytest.mark.parametrize('name', FWD_CASES)
def test_forward_vs_oracle(name, B, kind):
    """Log-likelihoods and the leaf layer's output alone (a leaf error cannot hide behind the log-sum-exp above it) against
    the float64 oracle; the all-NaN row gives 0; rows evaluated as a slice give the same bits as in the full batch.  The two
    rows with a +inf and a -inf entry must give what the oracle gives -- in float32 for these rows, where the largest finite
    number nan_to_num clamps to is the reference's (ratspn_bernoulli_cases.forward_reference) -- +inf included: rel_err asks
    for the same non-finite pattern."""
    model, sd = device_model(name), state64(name)
    x = bc.make_evidence(name, B, kind)
    want, want_leaf = bc.forward_reference(sd, x)
    xc = x.cuda()
    lo = min(5, B - 1)
    hi = max(lo + 1, B - 3)
    with torch.no_grad():
        got = model(xc)
        leaf = model.base_layer(xc)
        part = model(xc[lo:hi])
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    err, err_leaf = rel_err(got.cpu().numpy(), want), rel_err(leaf.cpu().numpy(), want_leaf)
    tag = 'test_forward_vs_oracle[%s-%d-%s]' % (name, B, kind)
    report_measured(tag + ' ll', err, LL_TOL)
    report_measured(tag + ' leaf', err_leaf, LL_TOL)
    assert err <= LL_TOL
    assert err_leaf <= LL_TOL
    if kind == 'nan':
        assert np.all(np.abs(got[0].cpu().numpy()) < 1e-5)
    assert torch.equal(part, got[lo:hi])


def test_two_samples_per_lane():
    """40000 samples > 32768: the 8-channel blocks with two samples per lane.  A scattered subset against the oracle, and the
    first 300 rows evaluated alone (one sample per lane) against the full launch -- to LL_TOL, not bit for bit: the two
    mappings sum in different orders."""
    name, B = 'two_per_lane', 40000
    model, sd = device_model(name), state64(name)
    x = bc.make_evidence(name, B, 'nan', nan_frac=0.25)
    rows = torch.randint(0, B, (512,), generator=torch.Generator().manual_seed(8))
    rows[:8] = torch.tensor([0, 1, 2, 3, 63, 64, B - 2, B - 1])
    want, _ = bc.forward_reference(sd, x[rows])
    xc = x.cuda()
    with torch.no_grad():
        big = model(xc)
        small = model(xc[:300])
    err = rel_err(big[rows.cuda()].cpu().numpy(), want)
    report_measured('test_two_samples_per_lane 512 rows vs fp64', err, LL_TOL)
    assert err <= LL_TOL
    assert abs(big[0].item()) < 1e-5
    assert rel_err(small.cpu().numpy(), big[:300].cpu().numpy()) <= LL_TOL


def test_normalisation_at_eight_channels():
    """sum over all 2^12 assignments of exp(LL) = 1, and the same for the marginal over the last 5 variables with the first 7
    marginalised (the reference's known-answer test at a second shape: CB 8, one sample per lane)."""
    from deeprob.spn.models import BernoulliRatSpn
    torch.manual_seed(17)
    model = BernoulliRatSpn(12, rg_depth=2, rg_repetitions=3, rg_batch=8, rg_sum=4, random_state=3).eval()
    with torch.no_grad():
        model.base_layer.logits.mul_(2.0)
    model.cuda()
    bits = ((np.arange(2 ** 12)[:, None] >> np.arange(11, -1, -1)[None, :]) & 1).astype(np.float32)
    sub = bits[:32].copy()                        # (the first 32 rows run through every assignment of the last 5 variables)
    sub[:, :7] = np.nan
    with torch.no_grad():
        ll = model(torch.from_numpy(bits).cuda()).double()
        ll_sub = model(torch.from_numpy(sub).cuda()).double()
    total, total_sub = torch.exp(ll).sum().item(), torch.exp(ll_sub).sum().item()
    report_measured('test_normalisation_at_eight_channels |sum exp(LL) - 1|', abs(total - 1.0), 1e-5)
    report_measured('test_normalisation_at_eight_channels marginal |sum exp(LL) - 1|', abs(total_sub - 1.0), 1e-5)
    assert abs(total - 1.0) < 1e-5
    assert abs(total_sub - 1.0) < 1e-5


# ---- backward ---------------------------------------------------------------------------------------------------------------
BWD_CASES = [('mnist8', 300), ('wide16_d1', 300), ('ad4', 300),       # moment kernel: four waves x 75 rows, ragged 64-row chunks
             ('mnist8', 2048), ('mnist8', 2049),                      # its last batch size / the first on the 64-sample kernel, CBK 4
             ('pad2', 300), ('odd3', 300), ('one', 300),              # staged kernel
             ('many_groups', 1024),                                   # staged kernel, several tiles per work-group
             ('pad2', 1100), ('odd3', 1100),                          # 64-sample kernel: 17 full tiles plus 12 rows
             ('heavy_pad', 37)]                                       # d/dx with pad >= d


@functools.lru_cache(maxsize=None)
def backward_reference(name, B, kind):
    """(x, y, ref64, ref32): the oracle's gradients in float64 and in float32 -- plain autograd for clean evidence, the masked
    gradient for NaN evidence (without the inf rows)."""
    sd = state64(name)
    y = bc.labels(name, B)
    x = bc.make_evidence(name, B, kind, inf_rows=False)
    if kind == 'binary':
        refs = [bc.reference_grads(sd, x, y, dtype) for dtype in (torch.float64, torch.float32)]
    else:
        nan_mask = torch.isnan(x)
        refs = [bc.masked_reference_grads(sd, x, nan_mask, dtype, y=y) for dtype in (torch.float64, torch.float32)]
    return x, y, refs[0], refs[1]


# one variant with x.requires_grad and one without (they select different launches in leaf_backward_common), on clean and on
# NaN evidence; the case that is about d/dx runs with x.requires_grad only
BWD_PARAMS = [pytest.param(name, B, kind, x_grad, id='%s-%d-%s-%s' % (name, B, kind, 'dx' if x_grad else 'nodx'))
              for name, B in BWD_CASES for kind in ('binary', 'nan') for x_grad in (True, False)
              if x_grad or name != 'heavy_pad']


@pytest.mark.parametrize('name,B,kind,x_grad', BWD_PARAMS)
def test_backward_vs_oracle(name, B, kind, x_grad):
    """Gradients of the loss w.r.t. the logits, every sum weight, the root weight and (x_grad) the evidence.  Bar per tensor, as
    in test_backward_wide_model_vs_oracle: distance to float64 <= GRAD_TOL, widened to twice the float32 oracle's own distance
    from float64 -- a term that comes from the reference alone."""
    model = device_model(name)
    x, y, ref64, ref32 = backward_reference(name, B, kind)
    for p in model.parameters():
        p.grad = None
    xg = x.cuda().requires_grad_(x_grad)
    with torch.enable_grad():
        model.loss(model(xg), None if y is None else y.cuda()).backward()
    got = {k: p.grad.cpu().numpy() for k, p in model.named_parameters()}
    assert sorted(got) == sorted(k for k in ref64 if k != 'x')
    if x_grad:
        got['x'] = xg.grad.cpu().numpy()
        nan_mask = torch.isnan(x).numpy()
        assert (got['x'][nan_mask] == 0).all()
    failed = []
    for k in sorted(got):
        assert np.isfinite(got[k]).all(), k
        own = grad_err(ref32[k], ref64[k])
        tol = max(GRAD_TOL, 2.0 * own)
        err = grad_err(got[k], ref64[k])
        report_measured('test_backward_vs_oracle[%s-%d-%s-%s] grad.%s vs fp64' % (name, B, kind, 'dx' if x_grad else 'nodx', k),
                        err, tol, '(oracle fp32 vs fp64 = %.2e)' % own)
        if err > tol:
            failed.append((k, err, tol))
    assert not failed, failed


# ---- top-down ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['mnist8', 'wide16_d1'])
def test_mpe_at_width(name):
    """MPE with Bernoulli leaves at 8 / 16 channels: the bottom-up activations against the float64 oracle, the top-down pass
    against its numpy restatement from the device's own activations on EVERY row, and every completed entry = [logit >= 0] of
    the chosen channel (logits that are exactly 0 included: sigmoid(0) >= 0.5)."""
    from deeprob.hip import ops
    model, sd = device_model(name), state64(name)
    B = 300
    x = bc.make_evidence(name, B, 'nan', nan_frac=0.5, inf_rows=False)
    y = bc.labels(name, B)
    xc, yc = x.cuda(), (None if y is None else y.cuda())
    depth = model.rg_depth
    with torch.no_grad():
        acts = model._upward_for_mpe(xc)
        for t, (a, want) in enumerate(zip(acts, host_activations(sd, x.double(), depth))):
            assert rel_err(a.cpu().numpy(), want.numpy()) <= LL_TOL, t
        leaf = model._leaf_params()
        out, choice = ops.ratspn_topdown(0, leaf[0], B, model._fused_ctx, xc, yc, acts, model._topdown_logw(),
                                         model._topdown_src(), leaf[1], leaf[2], want_choice=True)
        want, rep, chan = mpe_replay(acts, model._topdown_logw(), model._topdown_src(), leaf, x, y)
        got = model.mpe(xc, y=yc)
    choice = choice.cpu().long()
    assert torch.equal(choice[:, 0], rep)
    assert torch.equal(choice[:, 1:], chan)
    assert torch.equal(out.cpu(), want)
    assert torch.equal(got, out)
    # the completion from the choices and the logits alone
    G0, d = 2 ** depth, model.base_layer.dimension
    src = model._topdown_src().cpu().long()[rep]                 # [B, D]
    rl, j = torch.div(src, d, rounding_mode='floor'), src % d
    lg = model.base_layer.logits.detach().cpu()[rep[:, None] * G0 + rl, torch.gather(chan, 1, rl), j]
    missing = torch.isnan(x)
    assert torch.equal(out.cpu()[missing], (lg >= 0).float()[missing])
    assert torch.equal(out.cpu()[~missing], x[~missing])


def test_sample_replays_against_the_oracle_at_width():
    """test_ratspn_gpu.py::test_sample_replays_against_the_oracle's protocol on the 784-variable, 8-channel model."""
    from deeprob.hip import ops
    name, n, seed = 'mnist8', 5000, 987654321
    model = device_model(name)
    sd = bc.sd_as(host_model(name), torch.float32)
    kw = bc.CASES[name][0]
    want, rep, chan, margin = orc.ratspn_sample_replay(sd, n, kw['rg_depth'], kw['in_features'], seed=seed)
    got = model.sample(n, seed=seed)
    assert tuple(got.shape) == (n, kw['in_features']) and got.is_cuda and torch.isfinite(got).all()
    leaf = model._leaf_params()
    out, choice = ops.ratspn_topdown(1, leaf[0], n, model._fused_ctx, None, None, None, model._topdown_logw(),
                                     model._topdown_src(), leaf[1], leaf[2], seed=seed, want_choice=True)
    assert torch.equal(out, got)
    choice = choice.cpu()
    clear = torch.from_numpy(margin > 3e-6)
    assert clear.float().mean().item() >= 0.97
    assert torch.equal(choice[clear, 0].long(), rep[clear])
    assert torch.equal(choice[clear, 1:].long(), chan[clear])
    flips = (got.cpu()[clear] != want[clear]).float().mean().item()
    report_measured('test_sample_replays_against_the_oracle_at_width flipped u1 < p draws', flips, 1e-4)
    assert flips < 1e-4
