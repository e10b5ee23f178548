"""DgcSpn.mpe_completion without a device: the header's third mode, the argument errors raised before anything reaches the
device, and the restatement the GPU tests replay against (tests/dgcspn_mpe_ref.py) against a second, independent
formulation: float64, recursive, node by node over the dense product maps of the oracle's forward."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

from oracle import dgcspn_oracle as dorc
from tests import dgcspn_mpe_ref as mref
from tests import dgcspn_topdown_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = ref.B                                       # 301, as in the top-down tests
HOST_CASES = ['dw4', 'full3', 'odd5', 'mixed6']
# The seeds of the model and of the evidence (tests/dgcspn_topdown_ref.py: make_model, make_evidence), chosen so that the
# float32 restatement and the float64 formulation choose the same input at every node of every row: no row is exempt.
MODEL_SEED, EVIDENCE_SEED = 31, 32
MAX_EXEMPT = {'dw4': 0, 'full3': int(0.02 * B), 'odd5': int(0.02 * B), 'mixed6': int(0.02 * B)}


# ---- the header ----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_third_mode_and_no_new_entry_point():
    from deeprob import hip
    from deeprob.hip import dgc
    text = open(os.path.join(ROOT, 'include', 'deeprob_dgc.h')).read()
    sigs, consts, _ = hip.parse_header(text, prefix='dpg', header='deeprob_dgc.h')
    assert consts['DPG_MODE_MPE'] == 3 == dgc.DPG_MODE_MPE
    assert consts['DPG_MODE_PRIOR'] == 1 and consts['DPG_MODE_POSTERIOR'] == 2
    assert sorted(sigs) == ['dpg_abi_version', 'dpg_dgcspn_topdown', 'dpg_last_error'] and sigs == dgc.SIGNATURES
    assert len(sigs['dpg_dgcspn_topdown'][1]) == 19


# ---- the second formulation: float64, recursive, dense product maps ----------------------------------------------------------
def first_max64(s, lw):
    """The node rule on one node's float64 scores: the first maximum; the first maximum of the weights when no score is a
    number above -inf."""
    m = np.max(s)                                                        # (propagates NaN)
    if m > -np.inf:
        return int(np.flatnonzero(s == m)[0])
    return int(np.flatnonzero(lw == np.max(lw))[0])


class Circuit:
    """One case's levels from the oracle's plan: (pad, stride, dilation, depthwise, input shape) per product level, the
    channel combinations in itertools.product order, and which entry of the oracle's activations is which map."""

    def __init__(self, case):
        kw = ref.CASES[case]
        self.plan = ref.case_plan(case)
        self.prod_at = [i for i, step in enumerate(self.plan) if step[0] == 'prod']
        self.L = len(self.prod_at)
        self.in_features = kw['in_features']
        self.combos = {}

    def children(self, level, in_shape, oc, oh, ow):
        """[(channel, h, w)] of the taps of product (oc, oh, ow) of `level` that fall inside its input map."""
        _, pad, stride, dilation, dw = self.plan[self.prod_at[level]]
        cin, hin, win = in_shape
        if not dw and level not in self.combos:
            self.combos[level] = list(itertools.product(range(cin), repeat=4))
        out = []
        for th in range(2):
            for tw in range(2):
                h, w = oh * stride + th * dilation - pad[2], ow * stride + tw * dilation - pad[0]
                if 0 <= h < hin and 0 <= w < win:
                    out.append((oc if dw else self.combos[level][oc][2 * th + tw], h, w))
        return out


def descend(circ, score_fns, in_shapes, root_shape, on_node):
    """The recursion.  score_fns(node) -> (s64, lw64, s32) of the node's inputs; node = ('root',) or (t, o, h, w).
    on_node(node, pick64, pick32, s64) is called at every node reached through float64 picks; a node at which float32
    picks otherwise ends its branch (what lies below is another tree).  Returns (root index or -1, {pixel (h, w): k})."""
    comp = {}

    def visit(t, o, h, w):
        if t == 0:
            assert (h, w) not in comp, 'a pixel is reached twice'
            comp[(h, w)] = o
            return
        s64, lw64, s32 = score_fns((t, o, h, w))
        c, c32 = first_max64(s64, lw64), first_max64(s32.astype(np.float64), lw64)
        on_node((t, o, h, w), c, c32, s64)
        if c != c32:
            return
        for ch, hh, ww in circ.children(t - 1, in_shapes[t - 1], c, h, w):
            visit(t - 1, ch, hh, ww)

    s64, lw64, s32 = score_fns(('root',))
    i, i32 = first_max64(s64, lw64), first_max64(s32.astype(np.float64), lw64)
    on_node(('root',), i, i32, s64)
    if i != i32:
        return -1, comp
    oc, oh, ow = np.unravel_index(i, root_shape)
    for ch, hh, ww in circ.children(circ.L - 1, in_shapes[circ.L - 1], int(oc), int(oh), int(ow)):
        visit(circ.L - 1, ch, hh, ww)
    return i, comp


@functools.lru_cache(maxsize=None)
def host_case(case):
    """Everything a host test of `case` needs, made once and never written to: the model, the evidence and labels, the
    float32 and float64 states, activations and log-weights, and the restatement's (out, choice)."""
    model = ref.make_model(case, seed=MODEL_SEED)
    x, y = ref.make_evidence(model, case, seed=EVIDENCE_SEED)
    plan, geom = ref.case_plan(case), ref.case_geometry(case)
    sd32, sd64 = ref.state(model, torch.float32), ref.state(model, torch.float64)
    acts32 = ref.host_activations(sd32, x, plan)
    logw32, logw64 = ref.host_logws(sd32, plan), ref.host_logws(sd64, plan)
    _, all64 = dorc.dgcspn_forward(sd64, x.double(), plan, return_activations=True)
    got = mref.topdown_mpe(geom, ref.CASES[case]['in_features'], acts32, logw32, sd32['base_layer.loc'], x, y)
    return dict(model=model, x=x, y=y, plan=plan, geom=geom, sd32=sd32, acts32=acts32, logw32=logw32, logw64=logw64,
                all64=[a.numpy() for a in all64], got=got)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('case', HOST_CASES)
def test_restatement_against_the_float64_recursion(case):
    """Row by row.  eps is the largest |s32 - s64| over all scores of the row (every input of every sum node at every
    position, and of the root), computed here.  Where the two formulations choose differently at a node whose ancestors
    agree, each of the two scores has moved by at most eps, so the float64 gap between the float64 pick and the float32
    pick is at most 2 eps: asserted, and such a row is exempt.  Every other row matches bit for bit, `out` and `choice`.
    The exempt rows are counted: none on dw4, at most 2 % elsewhere -- with these seeds none anywhere."""
    d = host_case(case)
    circ = Circuit(case)
    C, H, W = circ.in_features
    geom, x, y = d['geom'], d['x'], d['y']
    L = circ.L
    loc32 = d['sd32']['base_layer.loc'].numpy()
    out, choice = d['got']
    assert tuple(out.shape) == (B, C, H, W) and tuple(choice.shape) == (B, 1 + H * W) and choice.dtype == torch.int32
    # dense maps: the float64 product maps are the oracle's (F.pad and strided slices), the float32 ones the kernel's order
    P64 = [d['all64'][i + 1] for i in circ.prod_at]
    P32 = [ref.product_map(geom[j], d['acts32'][j].numpy()) for j in range(L)]
    in_shapes = [d['all64'][i].shape[1:] for i in circ.prod_at]
    lw32 = [w.numpy() for w in d['logw32']]
    lw64 = [w.numpy() for w in d['logw64']]
    exempt = []
    for b in range(B):
        cls = 0 if y is None else int(y[b])
        eps = 0.0
        with np.errstate(invalid='ignore'):
            for t in range(1, L + 1):
                if t == L:
                    a = P64[L - 1][b].reshape(-1) + lw64[L - 1][cls]
                    c = (P32[L - 1][b].reshape(-1) + lw32[L - 1][cls]).astype(np.float32)
                else:
                    a = P64[t - 1][b][None] + lw64[t - 1]
                    c = (P32[t - 1][b][None] + lw32[t - 1]).astype(np.float32)
                both = np.isfinite(a) & np.isfinite(c)
                assert both.any()
                eps = max(eps, float(np.abs(a - c.astype(np.float64))[both].max()))

        def scores(node):
            if node == ('root',):
                return (P64[L - 1][b].reshape(-1) + lw64[L - 1][cls], lw64[L - 1][cls],
                        (P32[L - 1][b].reshape(-1) + lw32[L - 1][cls]).astype(np.float32))
            t, o, h, w = node
            return (P64[t - 1][b][:, h, w] + lw64[t - 1][o, :, h, w], lw64[t - 1][o, :, h, w],
                    (P32[t - 1][b][:, h, w] + lw32[t - 1][o, :, h, w]).astype(np.float32))

        differs = []

        def on_node(node, pick64, pick32, s64):
            if pick64 != pick32:
                gap = float(s64[pick64] - s64[pick32])
                assert 0.0 <= gap <= 2.0 * eps, (case, b, node, gap, eps)
                differs.append(node)

        root, comp = descend(circ, scores, in_shapes, P64[L - 1][b].shape, on_node)
        if differs:
            exempt.append(b)
            continue
        want_choice = np.full(1 + H * W, -1, np.int32)
        want_choice[0] = root
        want = x[b].numpy().copy()
        for (h, w), k in comp.items():
            want_choice[1 + h * W + w] = k
            hide = np.isnan(want[:, h, w])
            want[hide, h, w] = loc32[k, hide, h, w]
        assert np.array_equal(choice[b].numpy(), want_choice), (case, b)
        assert np.array_equal(out[b].numpy().view(np.int32), want.view(np.int32)), (case, b)
    print('%s: %d of %d rows exempt' % (case, len(exempt), B))
    assert len(exempt) <= MAX_EXEMPT[case], exempt
    assert not exempt, 'the seeds were chosen so that no row is exempt'


@pytest.mark.parametrize('case', HOST_CASES)
def test_observed_entries_and_scope(case):
    """A fully observed x comes back bit for bit with every in-scope choice >= 0; on odd5 the last row and column have
    choice -1 and come back as given, NaN included; elsewhere every NaN of a pixel in scope is filled with a number."""
    d = host_case(case)
    C, H, W = ref.CASES[case]['in_features']
    scope = torch.ones(H, W, dtype=torch.bool)
    if case == 'odd5':
        scope[-1, :] = scope[:, -1] = False
    out, choice = d['got']
    comp = choice[:, 1:].view(B, H, W)
    assert (comp[:, scope] >= 0).all() and (comp[:, ~scope] == -1).all() and (choice[:, 0] >= 0).all()
    assert torch.equal(bits(out[:, :, ~scope]), bits(d['x'][:, :, ~scope]))
    assert case != 'odd5' or torch.isnan(out[:, :, ~scope]).any()
    assert not torch.isnan(out[:, :, scope]).any()
    obs = ~torch.isnan(d['x'])
    assert torch.equal(bits(out[obs]), bits(d['x'][obs]))
    # filled entries are locations of the chosen component
    loc = d['sd32']['base_layer.loc']
    k = comp.clamp(min=0)[:, None].expand(B, C, H, W)
    mode = torch.gather(loc[None].expand(B, -1, -1, -1, -1), 1, k[:, None]).squeeze(1)
    fill = torch.isnan(d['x']) & scope
    assert torch.equal(bits(out[fill]), bits(mode[fill]))
    full = torch.nan_to_num(d['x'], nan=0.25)
    acts = ref.host_activations(d['sd32'], full, d['plan'])
    o2, c2 = mref.topdown_mpe(d['geom'], (C, H, W), acts, d['logw32'], loc, full, d['y'])
    assert torch.equal(bits(o2), bits(full)) and (c2[:, 1:].view(B, H, W)[:, scope] >= 0).all() and (c2[:, 0] >= 0).all()


def bare_weight_choices(case, logw, cls):
    """The first argmax of the bare log-weights, node by node: the float64 recursion with every product value 0."""
    circ = Circuit(case)
    geom = ref.case_geometry(case)
    L = circ.L
    lw = [np.asarray(w, dtype=np.float64) for w in logw]
    in_shapes = [tuple(g[0:3]) for g in geom]

    def scores(node):
        if node == ('root',):
            return lw[L - 1][cls], lw[L - 1][cls], lw[L - 1][cls].astype(np.float32)
        t, o, h, w = node
        v = lw[t - 1][o, :, h, w]
        return v, v, v.astype(np.float32)

    root, comp = descend(circ, scores, in_shapes, tuple(geom[-1][3:6]), lambda *a: None)
    C, H, W = circ.in_features
    want = np.full(1 + H * W, -1, np.int32)
    want[0] = root
    for (h, w), k in comp.items():
        want[1 + h * W + w] = k
    return want


@pytest.mark.parametrize('case', ['dw4', 'odd5', 'mixed6', 'wide3'])
def test_activations_of_log_one_select_by_the_bare_weights(case):
    """All-NaN x with every activation exactly log 1 = 0: every score is its weight, the choices are the first argmax of
    the bare log-weights (per class), and every pixel in scope is the location of its component."""
    d_model = ref.make_model(case, seed=MODEL_SEED)
    plan, geom = ref.case_plan(case), ref.case_geometry(case)
    sd = ref.state(d_model)
    logw = ref.host_logws(sd, plan)
    C, H, W = ref.CASES[case]['in_features']
    classes = ref.CASES[case].get('out_classes', 1)
    n = 2 * classes
    x = torch.full((n, C, H, W), float('nan'))
    y = torch.arange(n) % classes
    acts = [torch.zeros((n,) + tuple(g[0:3])) for g in geom]
    out, choice = mref.topdown_mpe(geom, (C, H, W), acts, logw, sd['base_layer.loc'], x, y if classes > 1 else None)
    for b in range(n):
        assert np.array_equal(choice[b].numpy(), bare_weight_choices(case, [w.numpy() for w in logw], int(y[b]))), (case, b)
    # the fallback takes the same inputs: activations of -inf, and of NaN
    for fill in (float('-inf'), float('nan')):
        o2, c2 = mref.topdown_mpe(geom, (C, H, W), [torch.full_like(a, fill) for a in acts], logw, sd['base_layer.loc'], x,
                                  y if classes > 1 else None)
        assert torch.equal(c2, choice) and torch.equal(bits(o2), bits(out))


@pytest.mark.parametrize('case,count', [('dw4', 2), ('wide3', 81)])
def test_ties_go_to_the_lowest_index(case, count):
    """A table with two equal best weights at every node: the lower index is taken, at a node of 2 inputs (one lane's loop
    in the kernel) and at a node of 81 (more than a wave's 64 lanes), whichever of the two comes first in a lane's stride."""
    geom = ref.case_geometry(case)
    C, H, W = ref.CASES[case]['in_features']
    assert geom[0][3] == count and len(geom) >= 2
    sd = ref.state(ref.make_model(case, seed=MODEL_SEED))
    logw = [w.clone() for w in ref.host_logws(sd, ref.case_plan(case))]
    assert logw[0].shape[1] == count
    x = torch.full((1, C, H, W), float('nan'))
    acts = [torch.zeros((1,) + tuple(g[0:3])) for g in geom]
    # (lo, hi): hi in an earlier lane than lo (70 -> lane 6, 7 -> lane 7), in the same lane (3, 67), in a later one
    pairs = [(0, 1)] if count == 2 else [(7, 70), (3, 67), (5, 80), (0, 64), (63, 64)]
    root_n = logw[-1].shape[1]
    for lo, hi in pairs:
        tied = [w.clone() for w in logw]
        tied[0][:, lo] = tied[0][:, hi] = 1.0                                # above every log-softmax weight
        rlo, rhi = (lo, hi) if count == 2 else (lo + 64, hi + 128)
        assert rhi < root_n
        tied[-1][:, rlo] = tied[-1][:, rhi] = 1.0
        for fill in (0.0, float('-inf')):                                     # by the scores, and by the fallback
            out, choice = mref.topdown_mpe(geom, (C, H, W), [torch.full_like(a, fill) for a in acts], tied,
                                           sd['base_layer.loc'], x, None)
            assert int(choice[0, 0]) == rlo
            want = bare_weight_choices(case, [w.numpy() for w in tied], 0)
            assert np.array_equal(choice[0].numpy(), want)
        # sum layer 1 picks product `lo` of level 0 wherever it is reached: its taps carry lo's channels
        below = mref.tap_channel(geom[0], lo, 0)
        assert (choice[0, 1:] >= 0).all() and below in choice[0, 1:].tolist()


# ---- methods and errors ------------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_device(monkeypatch):
    """A CPU model raises HipError (no silent fallback); training-mode dropout is not built and says so.  The shape and the
    labels are checked before the bottom-up pass: with the device check stood in for, a wrong shape and a label out of
    range raise ValueError on the host (the GPU test raises them on the real path)."""
    from deeprob.hip import HipError, ops
    from deeprob.spn.models import DgcSpn
    model = ref.make_model('dw4')
    assert callable(DgcSpn.mpe_completion)
    with pytest.raises(HipError) as info:
        model.mpe_completion(torch.randn(3, 1, 4, 4))
    assert not isinstance(info.value, NotImplementedError)
    with pytest.raises(HipError):
        model.mpe_completion(torch.randn(3, 1, 4, 4), return_choice=True)
    for kw in (dict(in_dropout=0.2), dict(sum_dropout=0.2)):
        drop = DgcSpn((1, 4, 4), n_batch=2, sum_channels=2, depthwise=True, **kw).train()
        with pytest.raises(NotImplementedError, match='dropout'):
            drop.mpe_completion(torch.randn(3, 1, 4, 4))
        with pytest.raises(HipError):
            drop.eval().mpe_completion(torch.randn(3, 1, 4, 4))
    monkeypatch.setattr(DgcSpn, '_check_topdown', lambda self, what: torch.device('cpu'))
    monkeypatch.setattr(ops, 'require_device_f32', lambda t, name: t)
    for shape in ((3, 1, 4, 5), (3, 2, 4, 4), (1, 4, 4), (3, 16)):
        with pytest.raises(ValueError, match='expected inputs'):
            model.mpe_completion(torch.randn(*shape))
    many = ref.make_model('mixed6')
    x = torch.randn(4, 2, 6, 6)
    for bad in ([0, 1, 3, 2], [0, -1, 1, 2]):
        with pytest.raises(ValueError, match='labels'):
            many.mpe_completion(x, y=torch.tensor(bad))
    with pytest.raises(ValueError, match='shape'):
        many.mpe_completion(x, y=torch.tensor([0, 1, 2]))


def test_the_sanity_row_of_the_device_test_has_a_clear_root():
    """The half-observed dw4 row that the device test draws 4 096 times: its exact float64 root posterior puts the two
    largest inputs at least 0.1 apart (14 standard errors of a difference of two frequencies among 4 096 draws), and the
    restatement's root choice is that posterior's mode."""
    model = ref.make_model('dw4')
    row = ref.half_observed_row(model, 'dw4', seed=mref.SANITY_ROW_SEED)
    post = mref.root_posterior64(model, 'dw4', row)
    top = np.sort(post)[::-1]
    assert abs(post.sum() - 1.0) <= 1e-12 and top[0] - top[1] >= 0.1, top[:3]
    sd = ref.state(model)
    plan = ref.case_plan('dw4')
    _, choice = mref.topdown_mpe(ref.case_geometry('dw4'), (1, 4, 4), ref.host_activations(sd, row, plan),
                                 ref.host_logws(sd, plan), sd['base_layer.loc'], row, None)
    assert int(choice[0, 0]) == int(np.argmax(post))
