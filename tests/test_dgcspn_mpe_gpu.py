"""DgcSpn.mpe_completion on the device (mode 3 of dpg_dgcspn_topdown, csrc/dgc/dgcspn_topdown.hip): replayed bit for bit
by the restatement of tests/dgcspn_mpe_ref.py from the device's own activations, checked at its degenerate nodes and its
ties, under the buffer contract (the guarded, poisoned allocations that tests/test_buffer_contract_gpu.py and
tests/test_dgcspn_topdown_gpu.py use, tests/buffer_contract.py), and against the sampler's most frequent root choice."""
import functools

import numpy as np
import pytest
import torch

from tests import dgcspn_mpe_ref as mref
from tests import dgcspn_topdown_ref as ref
from tests.buffer_contract import contract, PATTERNS
from tests.test_dgcspn_mpe_host import bare_weight_choices

pytestmark = pytest.mark.gpu

B = ref.B                     # 301: a ragged batch, one work-group a row
MODE_MPE = 3


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    """Bitwise equality (a pixel out of scope may be NaN in both)."""
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def logws_of(model):
    return [w.detach() for w in model._topdown_logw()]


def topdown(model, mode, x, y, acts, seed=0, logws=None):
    from deeprob.hip import dgc
    return dgc.dgcspn_topdown(mode, x.shape[0], model.in_features, dgc.product_geometry(model._product_layers()),
                              model.out_classes, x, y, acts, logws_of(model) if logws is None else logws,
                              model.base_layer.loc, model.base_layer.scale, seed, want_choice=True)


def restate(case, model, acts, x, y, logws=None):
    logws = logws_of(model) if logws is None else logws
    return mref.topdown_mpe(ref.case_geometry(case), ref.CASES[case]['in_features'], [a.cpu() for a in acts],
                            [w.cpu() for w in logws], model.base_layer.loc.detach().cpu(), x.cpu(),
                            None if y is None else y.cpu())


@functools.lru_cache(maxsize=None)
def device_case(case):
    """(model on the device, evidence, labels or None, the device's bottom-up activations, the restatement's (out, choice)
    from them): made once, shared by the tests, never written to."""
    model = ref.make_model(case)
    x, y = ref.make_evidence(model, case)
    model.cuda()
    xd, yd = x.cuda(), None if y is None else y.cuda()
    with torch.no_grad():
        acts = model._upward_for_sampling(xd)
    return model, xd, yd, acts, restate(case, model, acts, xd, yd)


def check_shape_of_the_result(case, xd, out, choice):
    """Observed entries bit for bit, pixels out of scope as given with choice -1, everything else filled with a number."""
    C, H, W = ref.CASES[case]['in_features']
    n = xd.shape[0]
    assert tuple(out.shape) == tuple(xd.shape) and out.is_cuda and out.dtype == torch.float32
    assert tuple(choice.shape) == (n, 1 + H * W) and choice.dtype == torch.int32 and choice.is_cuda
    scope = torch.ones(H, W, dtype=torch.bool)
    if case == 'odd5':
        scope[-1, :] = scope[:, -1] = False
    out, choice, x = out.cpu(), choice.cpu(), xd.cpu()
    obs = ~torch.isnan(x)
    assert torch.equal(bits(out[obs]), bits(x[obs]))
    assert not torch.isnan(out[:, :, scope]).any()
    comp = choice[:, 1:].view(n, H, W)
    assert (comp[:, scope] >= 0).all() and (comp[:, ~scope] == -1).all() and (choice[:, 0] >= 0).all()
    assert same_bits(out[:, :, ~scope], x[:, :, ~scope])


@pytest.mark.parametrize('case', list(ref.CASES))
def test_replays_the_restatement_bit_for_bit(case):
    """model.mpe_completion(x, y, return_choice=True) equals the restatement run on the device's own activations, `out`
    and `choice`, every row; the direct mode-3 call is the method's launch; the seed does not enter; a row's result does
    not depend on the batch around it."""
    model, xd, yd, acts, (want, want_choice) = device_case(case)
    out, choice = model.mpe_completion(xd, y=yd, return_choice=True)
    check_shape_of_the_result(case, xd, out, choice)
    assert torch.equal(choice.cpu(), want_choice), (choice.cpu() != want_choice).any(dim=1).nonzero().flatten().tolist()
    assert same_bits(out.cpu(), want)
    assert same_bits(model.mpe_completion(xd, y=yd), out)
    d_out, d_choice = topdown(model, MODE_MPE, xd, yd, acts, seed=1)
    assert same_bits(d_out, out) and torch.equal(d_choice, choice)
    s_out, s_choice = topdown(model, MODE_MPE, xd, yd, acts, seed=0xDEADBEEFCAFE)
    assert same_bits(s_out, out) and torch.equal(s_choice, choice)
    few, few_choice = model.mpe_completion(xd[:3], y=None if yd is None else yd[:3], return_choice=True)
    assert same_bits(few, out[:3]) and torch.equal(few_choice, choice[:3])


def test_without_labels_a_row_descends_from_its_best_class():
    """Three classes, no labels: the class of a row is the first maximum of its root outputs (class 0 for a row whose
    outputs hold a NaN or are all -inf), and the result is the restatement's with those labels, bit for bit."""
    from deeprob.hip import ops_spatial
    case = 'mixed6'
    model, xd, yd, acts, _ = device_case(case)
    with torch.no_grad():
        top = ops_spatial.spatial_prodroot(acts[-1], model.layers[-1], model.root_layer.weight, model.root_layer._ws2)
        if top is None:
            top = model.root_layer(model.layers[-1](acts[-1]))
    top = top.cpu().numpy()
    assert top.shape == (B, 3)
    cls = np.zeros(B, np.int64)
    for b in range(B):
        m = top[b].max()
        if m > -np.inf:
            cls[b] = int(np.flatnonzero(top[b] == m)[0])
    assert len(set(cls.tolist())) > 1, 'evidence that never changes the class tests nothing'
    out, choice = model.mpe_completion(xd, return_choice=True)
    check_shape_of_the_result(case, xd, out, choice)
    want, want_choice = restate(case, model, acts, xd, torch.from_numpy(cls))
    assert torch.equal(choice.cpu(), want_choice) and same_bits(out.cpu(), want)
    given = model.mpe_completion(xd, y=torch.from_numpy(cls).cuda())
    assert same_bits(given, out)
    # a model with one root ignores y
    one, xo, _, _, _ = device_case('dw4')
    assert same_bits(one.mpe_completion(xo, y=torch.full((B,), 7, device='cuda')), one.mpe_completion(xo))


@pytest.mark.parametrize('case', ['mixed6', 'wide3', 'odd5'])
def test_degenerate_activations_fall_to_the_weights(case):
    """Activations filled with -inf (no input of any node is possible) and with NaN: the first argmax of the bare
    log-weights at every node -- the float64 recursion over the weights alone, and the restatement -- and no NaN in any
    in-scope NaN entry."""
    model, xd, yd, acts, _ = device_case(case)
    logw = [w.cpu().numpy() for w in logws_of(model)]
    ycpu = torch.zeros(B, dtype=torch.long) if yd is None else yd.cpu()
    by_class = {c: bare_weight_choices(case, logw, c) for c in sorted(set(ycpu.tolist()))}
    want_choice = torch.from_numpy(np.stack([by_class[int(c)] for c in ycpu]))
    for fill in (float('-inf'), float('nan')):
        bad = [torch.full_like(a, fill) for a in acts]
        out, choice = topdown(model, MODE_MPE, xd, yd, bad)
        check_shape_of_the_result(case, xd, out, choice)
        assert torch.equal(choice.cpu(), want_choice)
        want, restated_choice = restate(case, model, bad, xd, yd)
        assert torch.equal(restated_choice, want_choice) and same_bits(out.cpu(), want)


@pytest.mark.parametrize('case', ['dw4', 'wide3'])
def test_ties_go_to_the_lowest_index(case):
    """Two equal best weights at the root and at every node of sum layer 1: the lower index, by the scores (activations of
    exactly log 1) and by the fallback (activations of -inf), at nodes of 2 inputs (one lane's loop) and of 81 and 1 296
    (a wave's scan: the pairs put the lower index in a later lane, in the same lane and in an earlier lane than the other)."""
    model, xd, _, acts, _ = device_case(case)
    logw = logws_of(model)
    count = logw[0].shape[1]
    assert count == (2 if case == 'dw4' else 81)
    nan = torch.full_like(xd[:5], float('nan'))
    pairs = [(0, 1)] if count == 2 else [(7, 70), (3, 67), (5, 80), (0, 64), (63, 64)]
    for lo, hi in pairs:
        tied = [w.clone() for w in logw]
        tied[0][:, lo] = 1.0
        tied[0][:, hi] = 1.0
        rlo, rhi = (lo, hi) if count == 2 else (lo + 64, hi + 128)
        tied[-1][:, rlo] = 1.0
        tied[-1][:, rhi] = 1.0
        for fill in (0.0, float('-inf')):
            flat = [torch.full_like(a[:5], fill) for a in acts]
            out, choice = topdown(model, MODE_MPE, nan, None, flat, logws=tied)
            assert (choice[:, 0] == rlo).all(), (lo, hi, fill, choice[:, 0].tolist())
            want = torch.from_numpy(bare_weight_choices(case, [w.cpu().numpy() for w in tied], 0))
            assert torch.equal(choice.cpu(), want.expand(5, -1)), (lo, hi, fill)
            w_out, w_choice = restate(case, model, flat, nan, None, logws=tied)
            assert torch.equal(choice.cpu(), w_choice) and same_bits(out.cpu(), w_out)


@pytest.mark.parametrize('case', ['odd5', 'wide3'])
def test_buffer_contract(case):
    """Poisoned, guard-banded out / choice (0xFF, 0x7F) for B = 1, 301 and 0: every element written, nothing outside them,
    and the evidence, the activations, the tables and the leaf parameters bitwise what they were.  (With pixels out of scope
    `choice` legitimately holds -1, the 0xFF poison itself: under that pattern `out` alone is expected written there.)"""
    from deeprob.hip import dgc
    model, xd, yd, acts, _ = device_case(case)
    logws = logws_of(model)
    geom = dgc.product_geometry(model._product_layers())
    loc, scale = model.base_layer.loc, model.base_layer.scale
    H, W = xd.shape[2], xd.shape[3]
    for b in (1, B, 0):
        xb, yb, ab = xd[:b], None if yd is None else yd[:b], [a[:b] for a in acts]
        args = (dgc.DPG_MODE_MPE, b, model.in_features, geom, model.out_classes, xb, yb, ab, logws, loc, scale, 0)
        want = dgc.dgcspn_topdown(*args, want_choice=True)
        for pattern in PATTERNS:
            with contract(pattern) as c:
                c.frozen(xb, yb, loc, scale, *ab, *logws)
                got = dgc.dgcspn_topdown(*args, want_choice=True)
                c.expect_written(got[0], None if case == 'odd5' and pattern == 0xFF else got[1])
            assert same_bits(got[0], want[0]) and torch.equal(got[1], want[1])
            assert tuple(got[0].shape) == (b,) + tuple(model.in_features) and tuple(got[1].shape) == (b, 1 + H * W)
    # B = 0 writes nothing: the method on an empty batch
    empty, empty_choice = model.mpe_completion(xd[:0], return_choice=True)
    assert tuple(empty.shape) == (0,) + tuple(model.in_features) and tuple(empty_choice.shape) == (0, 1 + H * W)


def test_argument_errors_on_the_device():
    model, xd, yd, acts, _ = device_case('mixed6')
    with pytest.raises(ValueError, match='expected inputs'):
        model.mpe_completion(xd[:, :1], y=yd)
    for bad in (3, -1):
        wrong = yd.clone()
        wrong[5] = bad
        with pytest.raises(ValueError, match='labels'):
            model.mpe_completion(xd, y=wrong)
    from deeprob.hip import dgc
    with pytest.raises(ValueError, match='activations'):
        topdown(model, dgc.DPG_MODE_MPE, xd, yd, None)
    full = torch.nan_to_num(xd, nan=0.5)
    assert torch.equal(model.mpe_completion(full, y=yd), full)


def test_the_sampler_most_often_takes_the_root_input_of_the_completion():
    """4 096 sample_conditional draws of one half-observed dw4 row: the root input drawn most often is choice[0] of
    mpe_completion.  The row is one whose exact float64 root posterior puts its two largest inputs at least 0.1 apart
    (asserted here, on the host): 14 standard errors of the difference of two frequencies among 4 096 draws."""
    case = 'dw4'
    model = device_case(case)[0]
    row = ref.half_observed_row(model, case, seed=mref.SANITY_ROW_SEED)
    host = ref.make_model(case)
    post = mref.root_posterior64(host, case, row)
    top = np.sort(post)[::-1]
    assert top[0] - top[1] >= 0.1, top[:3]
    n = 4096
    xd = row.cuda().expand(n, -1, -1, -1).contiguous()
    with torch.no_grad():
        acts = model._upward_for_sampling(xd)
    drawn, d_choice = topdown(model, 2, xd, None, acts, seed=ref.STAT_SEED)
    assert same_bits(drawn, model.sample_conditional(xd, seed=ref.STAT_SEED))
    counts = np.bincount(d_choice[:, 0].cpu().numpy(), minlength=len(post))
    out, choice = model.mpe_completion(xd[:1], return_choice=True)
    print('root posterior: top two %.4f %.4f; drawn %d and %d times of %d' % (top[0], top[1], np.sort(counts)[-1], np.sort(counts)[-2], n))
    assert int(np.argmax(counts)) == int(choice[0, 0]) == int(np.argmax(post))
    # and the completion's pixels are the chosen components' locations
    k = choice[0, 1:].long().view(1, 1, 4, 4)
    hid = torch.isnan(row[0]).cuda()
    mode = torch.gather(model.base_layer.loc.detach(), 0, k)[0]             # [C = 1, H, W]
    assert hid.any() and torch.equal(out[0][hid], mode[hid]) and torch.equal(out[0][~hid], xd[0][~hid])
