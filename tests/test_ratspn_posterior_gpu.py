"""RatSpn.sample_conditional on the device (mode 2 of dpk_ratspn_topdown, csrc/ratspn_topdown.hip): replayed by the
restatement of tests/ratspn_posterior_ref.py from the device's own activations and the same counter-based uniforms,
checked for exactness against an enumerated posterior, under the buffer contract, and at its edges."""
import numpy as np
import pytest
import torch

from oracle import ratspn_oracle as orc
from tests import ratspn_posterior_ref as ref
from tests.buffer_contract import contract, PATTERNS
from tests.util import report_measured

pytestmark = pytest.mark.gpu

SEED = 987654321
B = 301                       # a ragged last work-group (4 rows a work-group)

# A row is CLEAR when every categorical draw of its restatement keeps this distance (of u from a step of the normalised
# float64 CDF).  Measured over all cases below: the largest margin of any row whose choices differ from the restatement's is
# MEASURED_WORST_MARGIN (fp32 expf and an fp32 CDF of up to 2048 terms against float64); the threshold is ten times that and
# not below 3e-6, the value of test_sample_replays_against_the_oracle.
MEASURED_WORST_MARGIN = 0.0   # (measured on an MI355X: none of the 6 x 301 rows differed)
CLEAR_MARGIN = max(10.0 * MEASURED_WORST_MARGIN, 3e-6)

CASES = {
    # the root only, 27 inputs: lanes with empty chunks
    'depth1': dict(in_features=8, rg_depth=1, rg_repetitions=3, rg_batch=3),
    # padded region graph
    'pad': dict(in_features=15, rg_depth=2, rg_repetitions=3, rg_batch=3, rg_sum=5, optimize_scale=True),
    'classes': dict(in_features=64, out_classes=3, rg_depth=3, rg_repetitions=4, rg_batch=4, rg_sum=4),
    # root count 2048 = 32 inputs per lane, 256 per sum node
    'wide': dict(in_features=784, rg_depth=2, rg_repetitions=8, rg_batch=16, rg_sum=16),
    'bernoulli': dict(in_features=32, out_classes=2, rg_depth=3, rg_repetitions=3, rg_batch=3, rg_sum=2),
}


def make_case(case: str):
    """(model on the host, evidence [B, D] on the host, labels or None): 50 % NaN, row 0 all NaN, row 1 fully observed, row
    2 (Gaussian leaves) with its observed entries at loc + 40 scale of channel 0 of repetition 0 -- every score of that row
    is then far below the -104 under which expf alone returns 0."""
    from deeprob.spn.models import GaussianRatSpn, BernoulliRatSpn
    kw = CASES[case]
    bern = case == 'bernoulli'
    torch.manual_seed(21)
    model = (BernoulliRatSpn if bern else GaussianRatSpn)(random_state=4, **kw).eval()
    D = kw['in_features']
    gen = torch.Generator().manual_seed(22)
    x = (torch.rand(B, D, generator=gen) < 0.5).float() if bern else torch.randn(B, D, generator=gen)
    if not bern:
        base = model.base_layer
        s = model._topdown_src()[0].long()
        rl, j = torch.div(s, base.dimension, rounding_mode='floor'), s % base.dimension
        x[2] = (base.loc[rl, 0, j] + 40.0 * base.scale[rl, 0, j]).detach()
    x[torch.rand(B, D, generator=gen) < 0.5] = float('nan')
    x[0] = float('nan')
    x[1] = torch.nan_to_num(x[1], nan=0.0)
    assert torch.isnan(x[2]).any() and not torch.isnan(x[2]).all()
    y = (torch.arange(B) % kw['out_classes']) if kw.get('out_classes', 1) > 1 else None
    return model, x, y


def topdown(model, mode, x, y, acts, seed, n=None):
    from deeprob.hip import ops
    dist, p0, p1 = model._leaf_params()
    return ops.ratspn_topdown(mode, dist, x.shape[0] if n is None else n, model._fused_ctx, x, y, acts, model._topdown_logw(),
                              model._topdown_src(), p0, p1, seed=seed, want_choice=True)


def restate(model, acts, x, y, seed):
    dist, p0, p1 = model._leaf_params()
    return ref.posterior_sample([a.cpu() for a in acts], [w.detach().cpu() for w in model._topdown_logw()],
                                model._topdown_src().cpu(), (dist, p0.detach().cpu(), None if p1 is None else p1.detach().cpu()),
                                x.cpu(), None if y is None else y.cpu(), seed)


@pytest.mark.parametrize('case', ['depth1', 'pad', 'classes', 'classes_drawn', 'wide', 'bernoulli'])
def test_replays_against_the_restatement(case):
    """The same repetition and leaf channels as the restatement on every clear row, the same values (Gaussian: within 1e-4,
    the bar of test_sample_replays_against_the_oracle; Bernoulli: u < p flips only within rounding of p), observed entries
    bit for bit, no NaN.  `classes_drawn`: without labels -- the class the model drew is read back by comparing with the
    calls that pass each class, and the restatement gets it explicitly."""
    drawn = case == 'classes_drawn'
    name = 'classes' if drawn else case
    model, x, y = make_case(name)
    model.cuda()
    xd = x.cuda()
    if drawn:
        got = model.sample_conditional(xd, seed=SEED)
        per_class = [model.sample_conditional(xd, y=torch.full((B,), c, device='cuda'), seed=SEED) for c in range(3)]
        same = torch.stack([(got == o).all(dim=1) for o in per_class], dim=1)
        assert same.any(dim=1).all(), 'a row drawn without labels is the draw of no class'
        yd = torch.argmax(same.int(), dim=1)
    else:
        yd = None if y is None else y.cuda()
        got = model.sample_conditional(xd, y=yd, seed=SEED)
    assert tuple(got.shape) == tuple(x.shape) and got.is_cuda and got.dtype == torch.float32
    acts = model._upward_for_mpe(xd)
    want, rep, chan, margin = restate(model, acts, xd, yd, SEED)
    # the cap, on the restatement's margins alone: with ~2^depth + 1 draws a row and a threshold near 1e-5 far less than
    # 1 % of the rows are set aside; at least 97 % clear is the cap of the two existing top-down tests
    clear = torch.from_numpy(margin > CLEAR_MARGIN)
    assert clear.float().mean().item() >= 0.97, clear.float().mean().item()
    assert clear[2], 'the row of far-away evidence must be compared'

    out, choice = topdown(model, 2, xd, yd, acts, SEED)
    assert torch.equal(out, got)                      # (the method is this launch)
    got, choice = got.cpu(), choice.cpu().long()
    obs = ~torch.isnan(x)
    assert not torch.isnan(got).any()
    assert torch.equal(got[obs], x[obs])
    differs = (choice[:, 0] != rep) | (choice[:, 1:] != chan).any(dim=1)
    worst = float(margin[differs.numpy()].max()) if differs.any() else 0.0
    report_measured('test_replays_against_the_restatement[%s] largest margin of a row that differs (%d rows)'
                    % (case, int(differs.sum())), worst, CLEAR_MARGIN)
    print('%s: %d rows differ, largest margin %.3e; %d of %d rows clear' % (case, int(differs.sum()), worst, int(clear.sum()), B))
    assert not differs[clear].any(), (worst, differs.nonzero().flatten().tolist())
    if name == 'bernoulli':
        assert (got[clear] != want[clear]).any(dim=1).float().mean().item() < 1e-4
    else:
        err = (got[clear] - want[clear]).abs().max().item()
        report_measured('test_replays_against_the_restatement[%s] max |sample - replay|' % case, err, 1e-4)
        assert err <= 1e-4, err


def test_all_nan_evidence_is_the_prior():
    """Nothing observed: every activation is log 1, the posterior of every node is its weights -- the choices (and so the
    values) of sample(B, seed) on the rows that are clear in both restatements."""
    model, x, _ = make_case('pad')
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.cuda()
    xd = torch.full_like(x, float('nan')).cuda()
    acts = model._upward_for_mpe(xd)
    _, _, _, m_post = restate(model, acts, xd, None, SEED)
    _, _, _, m_prior = orc.ratspn_sample_replay(sd, B, 2, 15, seed=SEED)
    clear = torch.from_numpy((m_post > CLEAR_MARGIN) & (m_prior > CLEAR_MARGIN))
    assert clear.float().mean().item() >= 0.97
    post, c_post = topdown(model, 2, xd, None, acts, SEED)
    prior, c_prior = topdown(model, 1, None, None, None, SEED, n=B)
    assert torch.equal(post, model.sample_conditional(xd, seed=SEED)) and torch.equal(prior, model.sample(B, seed=SEED))
    assert torch.equal(c_post.cpu()[clear], c_prior.cpu()[clear])
    assert torch.equal(post.cpu()[clear], prior.cpu()[clear])


def test_impossible_evidence_falls_to_the_weights():
    """Step 3 of the definition: when no input of a node is possible (every score -inf) or a score is NaN, the node is
    chosen as mode 1 chooses it -- the same batch as sample(B, seed), and never a NaN downstream."""
    model, x, _ = make_case('pad')
    model.cuda()
    xd = torch.full_like(x, float('nan')).cuda()
    prior, c_prior = topdown(model, 1, None, None, None, SEED, n=B)
    for fill in (float('-inf'), float('nan')):
        acts = [torch.full_like(a, fill) for a in model._upward_for_mpe(xd)]
        out, choice = topdown(model, 2, xd, None, acts, SEED)
        assert torch.equal(choice, c_prior) and torch.equal(out, prior)


def test_exact_posterior_on_the_device():
    """The enumerable model and evidence of the host test as 200 000 identical rows: each of the 8 frequencies within 5
    standard errors of the enumerated posterior.  A kernel that samples from the weights alone, or from scores that are not
    normalised per node, cannot pass."""
    model, row, full, post = ref.enumerable_case()
    model.cuda()
    n = ref.ENUM_ROWS
    got = model.sample_conditional(row.cuda().expand(n, -1).contiguous(), seed=ref.ENUM_SEED)
    freq = ref.completion_counts(got, full) / n
    se = np.sqrt(post * (1.0 - post) / n)
    print('frequencies', freq, 'posterior', post, 'in standard errors', (freq - post) / se)
    assert (np.abs(freq - post) <= 5.0 * se).all(), (freq, post, se)


@pytest.mark.parametrize('case', ['pad', 'bernoulli'])
def test_buffer_contract(case):
    """Poisoned, guard-banded out / choice (0xFF, 0x7F): every element written, nothing outside them, and the evidence, the
    activations, the tables and the leaf parameters bitwise what they were."""
    model, x, y = make_case(case)
    model.cuda()
    xd, yd = x.cuda(), None if y is None else y.cuda()
    acts = model._upward_for_mpe(xd)
    logws, src = model._topdown_logw(), model._topdown_src()
    dist, p0, p1 = model._leaf_params()
    from deeprob.hip import ops
    want = ops.ratspn_topdown(2, dist, B, model._fused_ctx, xd, yd, acts, logws, src, p0, p1, seed=SEED, want_choice=True)
    for pattern in PATTERNS:
        with contract(pattern) as c:
            c.frozen(xd, yd, src, p0, p1, *acts, *logws)
            got = c.expect_written(*ops.ratspn_topdown(2, dist, B, model._fused_ctx, xd, yd, acts, logws, src, p0, p1,
                                                       seed=SEED, want_choice=True))
        assert 'dpk_ratspn_topdown' in c.called
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_determinism_and_the_grid_stride_loop():
    """The same seed twice is the same batch bit for bit, another seed another batch; more rows than one pass of the grid
    (256 compute units x 16 work-groups x 4 rows): all finite, and a row's draws depend on (seed, row, its evidence) only."""
    from deeprob.spn.models import GaussianRatSpn
    model, x, y = make_case('classes')
    model.cuda()
    xd, yd = x.cuda(), y.cuda()
    first = model.sample_conditional(xd, y=yd, seed=7)
    assert torch.equal(first, model.sample_conditional(xd, y=yd, seed=7))
    assert not torch.equal(first, model.sample_conditional(xd, y=yd, seed=8))
    torch.manual_seed(1)
    small = GaussianRatSpn(40, out_classes=3, rg_depth=2, rg_repetitions=4, rg_batch=4, rg_sum=3, random_state=2).cuda().eval()
    n = 300000
    gen = torch.Generator(device='cuda').manual_seed(3)
    xb = torch.randn(n, 40, device='cuda', generator=gen)
    xb[torch.rand(n, 40, device='cuda', generator=gen) < 0.5] = float('nan')
    yb = torch.arange(n, device='cuda') % 3
    big = small.sample_conditional(xb, y=yb, seed=5)
    assert tuple(big.shape) == (n, 40) and torch.isfinite(big).all()
    assert torch.equal(big[:1000], small.sample_conditional(xb[:1000], y=yb[:1000], seed=5))
    obs = ~torch.isnan(xb)
    assert torch.equal(big[obs], xb[obs])


def test_edges():
    """An empty batch; nothing to draw (no NaN: the evidence as it is); labels of another integer dtype; a label given to a
    model with one root."""
    from deeprob.spn.models import GaussianRatSpn
    torch.manual_seed(1)
    model = GaussianRatSpn(40, out_classes=3, rg_depth=2, rg_repetitions=4, rg_batch=4, rg_sum=3, random_state=2).cuda().eval()
    for y in (None, torch.empty(0, dtype=torch.long, device='cuda')):
        empty = model.sample_conditional(torch.empty(0, 40, device='cuda'), y=y)
        assert tuple(empty.shape) == (0, 40) and empty.is_cuda
    x = torch.randn(9, 40, device='cuda')
    assert torch.equal(model.sample_conditional(x), x)
    assert torch.equal(model.sample_conditional(x, y=torch.arange(9, device='cuda') % 3, seed=1), x)
    x[:, ::2] = float('nan')
    y = torch.tensor([0, 1, 2, 1, 1, 0, 2, 2, 0], device='cuda')
    a = model.sample_conditional(x, y=y.to(torch.int32), seed=4)
    assert torch.equal(a, model.sample_conditional(x, y=y, seed=4)) and not torch.isnan(a).any()
    assert torch.equal(a[:, 1::2], x[:, 1::2])
    single = GaussianRatSpn(40, rg_depth=2, rg_repetitions=4, rg_batch=4, rg_sum=3, random_state=2).cuda().eval()
    b = single.sample_conditional(x, y=torch.full((9,), 2, device='cuda'), seed=4)
    assert torch.equal(b, single.sample_conditional(x, seed=4)) and not torch.isnan(b).any()
