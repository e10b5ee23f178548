"""DgcSpn.sample / sample_conditional on the device (dpg_dgcspn_topdown, csrc/dgc/dgcspn_topdown.hip): replayed by the
restatement of tests/dgcspn_topdown_ref.py from the device's own activations and the same counter-based uniforms, checked
for exactness against the float64 posterior marginals, under the buffer contract, and at its edges."""
import functools

import numpy as np
import pytest
import torch

from oracle import dgcspn_oracle as dorc
from tests import dgcspn_topdown_ref as ref
from tests.buffer_contract import contract, PATTERNS
from tests.util import report_measured

pytestmark = pytest.mark.gpu

SEED = 987654321
B = ref.B                     # 301: a ragged batch, one work-group a row

# A row is CLEAR when every categorical draw of its restatement keeps this distance (of u from a step of the normalised
# float64 CDF).  Measured over all cases below: the largest margin of any row whose choices differ from the restatement's is
# MEASURED_WORST_MARGIN (fp32 expf and an fp32 CDF of up to 1296 terms against float64); the threshold is ten times that and
# not below 3e-6, the project's rule (tests/test_ratspn_posterior_gpu.py).  On the restatement's margins alone a threshold
# of 3e-6 leaves 98.7 % of the 12 x 12 case's rows clear (about 290 categorical draws a row) and 8e-6 still 97 %.
MEASURED_WORST_MARGIN = 0.0   # (measured on an MI355X: none of the 6 x 301 rows differed)
CLEAR_MARGIN = max(10.0 * MEASURED_WORST_MARGIN, 3e-6)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    """Bitwise equality (a pixel out of scope may be NaN in both)."""
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def topdown(model, mode, x, y, acts, seed, n=None):
    from deeprob.hip import dgc
    return dgc.dgcspn_topdown(mode, x.shape[0] if n is None else n, model.in_features,
                              dgc.product_geometry(model._product_layers()), model.out_classes, x, y, acts,
                              model._topdown_logw(), model.base_layer.loc, model.base_layer.scale, seed, want_choice=True)


def restate(case, model, acts, x, y, seed, n_rows=None):
    return ref.topdown_sample(ref.case_geometry(case), ref.CASES[case]['in_features'],
                              None if acts is None else [a.cpu() for a in acts], [w.cpu() for w in model._topdown_logw()],
                              model.base_layer.loc.detach().cpu(), model.base_layer.scale.detach().cpu(),
                              None if x is None else x.cpu(), None if y is None else y.cpu(), seed, n_rows=n_rows)


@functools.lru_cache(maxsize=None)
def device_case(case):
    """(model on the device, evidence, labels or None, the device's bottom-up activations, the restatement's replay of
    sample_conditional(x, y, SEED) from them): made once, shared by the tests, never written to."""
    model = ref.make_model(case)
    x, y = ref.make_evidence(model, case)
    model.cuda()
    xd, yd = x.cuda(), None if y is None else y.cuda()
    with torch.no_grad():
        acts = model._upward_for_sampling(xd)
    return model, xd, yd, acts, restate(case, model, acts, xd, yd, SEED)


@pytest.mark.parametrize('case', list(ref.CASES))
def test_replays_against_the_restatement(case):
    """The same root index and components as the restatement on every clear row, drawn values within 1e-4 (the bar of the
    RAT-SPN replay tests), observed entries bit for bit, no NaN among the outputs in scope, out-of-scope pixels as given with
    component -1."""
    model, xd, yd, acts, (want, root, comp, margin) = device_case(case)
    got = model.sample_conditional(xd, y=yd, seed=SEED)
    assert tuple(got.shape) == tuple(xd.shape) and got.is_cuda and got.dtype == torch.float32
    clear = torch.from_numpy(margin > CLEAR_MARGIN)
    print('%s: %d of %d rows clear' % (case, int(clear.sum()), B))
    assert clear.float().mean().item() >= 0.97, clear.float().mean().item()

    out, choice = topdown(model, 2, xd, yd, acts, SEED)
    assert same_bits(out, got)                         # (the method is this launch)
    got, choice, x = got.cpu(), choice.cpu().long(), xd.cpu()
    C, H, W = ref.CASES[case]['in_features']
    scope = (comp[0] >= 0).view(H, W)                  # (the same for every row: it follows from the geometry)
    assert (comp >= 0).view(B, H, W)[:, scope].all() and scope.all() == (case != 'odd5')
    obs = ~torch.isnan(x)
    assert torch.equal(got[obs], x[obs])
    assert not torch.isnan(got[:, :, scope]).any()
    assert same_bits(got[:, :, ~scope], x[:, :, ~scope]) and (choice[:, 1:].view(B, H, W)[:, ~scope] == -1).all()
    assert (choice[:, 1:].view(B, H, W)[:, scope] >= 0).all()
    differs = (choice[:, 0] != root) | (choice[:, 1:] != comp).any(dim=1)
    worst = float(margin[differs.numpy()].max()) if differs.any() else 0.0
    report_measured('test_dgcspn_topdown replay[%s] largest margin of a row that differs (%d rows)' % (case, int(differs.sum())),
                    worst, CLEAR_MARGIN)
    print('%s: %d rows differ, largest margin %.3e' % (case, int(differs.sum()), worst))
    assert not differs[clear].any(), (worst, differs.nonzero().flatten().tolist())
    assert torch.equal(torch.isnan(got[clear]), torch.isnan(want[clear]))
    err = torch.nan_to_num(got[clear] - want[clear], nan=0.0).abs().max().item()
    report_measured('test_dgcspn_topdown replay[%s] max |sample - replay|' % case, err, 1e-4)
    assert err <= 1e-4, err


@pytest.mark.parametrize('case', ['odd5', 'dw12'])
def test_all_nan_evidence_is_the_prior(case):
    """Nothing observed: every activation is log 1 up to rounding, the posterior of every node is its weights -- the choices
    (and so the values) of sample(B, seed) on the rows that are clear in both restatements."""
    model, xd, _, _, _ = device_case(case)
    nan = torch.full_like(xd, float('nan'))
    with torch.no_grad():
        acts = model._upward_for_sampling(nan)
    m_post = restate(case, model, acts, nan, None, SEED)[3]
    m_prior = restate(case, model, None, None, None, SEED, n_rows=B)[3]
    clear = torch.from_numpy((m_post > CLEAR_MARGIN) & (m_prior > CLEAR_MARGIN))
    assert clear.float().mean().item() >= 0.97
    post, c_post = topdown(model, 2, nan, None, acts, SEED)
    prior, c_prior = topdown(model, 1, nan, None, None, SEED)
    assert same_bits(post, model.sample_conditional(nan, seed=SEED)) and same_bits(prior, model.sample(B, seed=SEED))
    assert torch.equal(c_post.cpu()[clear], c_prior.cpu()[clear])
    assert same_bits(post.cpu()[clear], prior.cpu()[clear])


@pytest.mark.parametrize('case', ['mixed6', 'wide3'])
def test_impossible_evidence_falls_to_the_weights(case):
    """When no input of a node is possible (every score -inf) or a score is NaN, the node is chosen as mode 1 chooses it: a
    mode-2 launch on such activations gives the mode-1 batch bit for bit, and nothing downstream is NaN."""
    model, xd, yd, acts, _ = device_case(case)
    nan = torch.full_like(xd, float('nan'))
    prior, c_prior = topdown(model, 1, nan, yd, None, SEED)
    assert not torch.isnan(prior).any() and (c_prior >= 0).all()
    for fill in (float('-inf'), float('nan')):
        out, choice = topdown(model, 2, nan, yd, [torch.full_like(a, fill) for a in acts], SEED)
        assert torch.equal(choice, c_prior) and same_bits(out, prior)


def test_exact_posterior_on_the_device():
    """The 4 x 4 case of the host test as 2^16 identical rows: every (component, pixel) frequency from `choice` within 5
    standard errors of d log p / d z in float64 (cells with an expected count below 50 are skipped), and the drawn pixels'
    means within 5 standard errors of the oracle's mpe in float64, which is the posterior mean.  A kernel that samples from
    the weights alone, or from scores that are not normalised per node, cannot pass."""
    case = 'dw4'
    model = device_case(case)[0]
    plan = ref.case_plan(case)
    sd64 = {k: v.cpu() for k, v in ref.state(model, torch.float64).items()}
    row = ref.half_observed_row(model, case)
    marg = ref.exact_marginals(sd64, row, plan)
    n = ref.STAT_ROWS
    xd = row.cuda().expand(n, -1, -1, -1).contiguous()
    with torch.no_grad():
        acts = model._upward_for_sampling(xd)
    out, choice = topdown(model, 2, xd, None, acts, ref.STAT_SEED)
    assert same_bits(out, model.sample_conditional(xd, seed=ref.STAT_SEED))
    out, comp = out.cpu(), choice.cpu()[:, 1:]
    ref.check_frequencies(ref.component_frequencies(comp, ref.CASES[case]['n_batch']), marg, n, 'device ' + case)
    hid = torch.isnan(row[0]).numpy()
    mean = dorc.dgcspn_mpe(sd64, row.double(), plan)[0].numpy()
    got, spread = out.double().mean(dim=0).numpy(), out.double().std(dim=0).numpy()
    dev = (np.abs(got - mean)[hid] / (spread[hid] / np.sqrt(n))).max()
    print('means: largest deviation %.2f standard errors' % dev)
    assert dev <= 5.0 and torch.equal(out[:, ~torch.isnan(row[0])], row[0][~torch.isnan(row[0])].expand(n, -1))


def test_determinism_and_the_row_counter():
    """The same seed gives the same bytes, another seed another batch; a row gives the same draw at the same index whether
    the batch around it is 3 rows or 301."""
    model, xd, yd, _, _ = device_case('mixed6')
    first = model.sample_conditional(xd, y=yd, seed=7)
    assert same_bits(first, model.sample_conditional(xd, y=yd, seed=7))
    assert not same_bits(first, model.sample_conditional(xd, y=yd, seed=8))
    assert same_bits(first[:3], model.sample_conditional(xd[:3], y=yd[:3], seed=7))
    prior = model.sample(B, y=yd, seed=7)
    assert same_bits(prior, model.sample(B, y=yd, seed=7)) and same_bits(prior[:3], model.sample(3, y=yd[:3], seed=7))
    assert not same_bits(prior, model.sample(B, y=yd, seed=8)) and not torch.isnan(prior).any()


@pytest.mark.parametrize('case', ['dw4', 'mixed6', 'odd5'])
def test_buffer_contract(case):
    """Poisoned, guard-banded out / choice (0xFF, 0x7F) for B = 1, 301 and 0: every element written, nothing outside them,
    and the evidence, the activations, the tables and the leaf parameters bitwise what they were.  (With pixels out of scope
    `choice` legitimately holds -1, the 0xFF poison itself: under that pattern `out` alone is expected written there.)"""
    from deeprob.hip import dgc
    model, xd, yd, acts, _ = device_case(case)
    logws = model._topdown_logw()
    geom = dgc.product_geometry(model._product_layers())
    loc, scale = model.base_layer.loc, model.base_layer.scale
    for b in (1, B, 0):
        xb, yb, ab = xd[:b], None if yd is None else yd[:b], [a[:b] for a in acts]
        for mode in (dgc.DPG_MODE_POSTERIOR, dgc.DPG_MODE_PRIOR):
            args = (mode, b, model.in_features, geom, model.out_classes, xb, yb, ab if mode == 2 else None, logws, loc, scale, SEED)
            want = dgc.dgcspn_topdown(*args, want_choice=True)
            for pattern in PATTERNS:
                with contract(pattern) as c:
                    c.frozen(xb, yb, loc, scale, *ab, *logws)
                    got = dgc.dgcspn_topdown(*args, want_choice=True)
                    c.expect_written(got[0], None if case == 'odd5' and pattern == 0xFF else got[1])
                assert same_bits(got[0], want[0]) and torch.equal(got[1], want[1])
                assert tuple(got[0].shape) == (b,) + tuple(model.in_features) and tuple(got[1].shape) == (b, 1 + xd.shape[2] * xd.shape[3])


def test_edges():
    """Three classes without labels: every row is the draw of one of the three per-class calls; a non-contiguous x is
    accepted (and read as the values it holds) or refused with ValueError; labels of another integer dtype; an empty batch;
    nothing to draw."""
    model, xd, yd, _, _ = device_case('mixed6')
    got = model.sample_conditional(xd, seed=SEED)
    per_class = [model.sample_conditional(xd, y=torch.full((B,), c, device='cuda'), seed=SEED) for c in range(3)]
    same = torch.stack([(bits(got) == bits(o)).flatten(1).all(dim=1) for o in per_class], dim=1)
    assert same.any(dim=1).all(), 'a row drawn without labels is the draw of no class'
    assert not torch.isnan(got).any()
    wide = torch.full((B, 2, 6, 12), 123.0, device='cuda')
    wide[:, :, :, ::2] = xd
    view = wide[:, :, :, ::2]
    assert not view.is_contiguous()
    try:
        assert same_bits(model.sample_conditional(view, y=yd, seed=SEED), model.sample_conditional(xd, y=yd, seed=SEED))
    except ValueError:
        pass
    assert same_bits(model.sample_conditional(xd, y=yd.to(torch.int32), seed=4), model.sample_conditional(xd, y=yd, seed=4))
    for y in (None, torch.empty(0, dtype=torch.long, device='cuda')):
        empty = model.sample_conditional(xd[:0], y=y)
        assert tuple(empty.shape) == (0, 2, 6, 6) and empty.is_cuda
    assert tuple(model.sample(0).shape) == (0, 2, 6, 6)
    full = torch.nan_to_num(xd, nan=0.5)
    assert torch.equal(model.sample_conditional(full, y=yd, seed=1), full)
    with pytest.raises(ValueError):
        model.sample_conditional(xd[:, :1], y=yd)
    # a label outside [0, classes) is an error, not a sample of another class
    for bad in (3, -1):
        wrong = yd.clone()
        wrong[5] = bad
        with pytest.raises(ValueError, match='labels'):
            model.sample_conditional(xd, y=wrong, seed=1)
        with pytest.raises(ValueError, match='labels'):
            model.sample(B, y=wrong, seed=1)
