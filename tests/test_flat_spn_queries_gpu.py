"""The node-graph SPN queries on the HIP path (mpe, sample, eval_backward, expectation_maximization) against the
reference's goldens (tools/gen_golden_spn_queries.py) and the CPU restatement (tests/flat_spn_query_ref.py).

Measured on an MI355X (the figures the tests print; bars in the test bodies): see DESIGN.md section 13."""
import ctypes
import io
import json
import os

import numpy as np
import pytest
import torch

from tests import flat_spn_query_ref as qref
from tests.flat_spn_cases import random_circuit
from tests.flat_spn_query_cases import support_inputs, RANDOM_CASES
from tests.test_flat_spn_queries_host import eligible_rows
from tests.util import rel_err, grad_err, report_measured

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
FLOOR = np.float32(-1e31)
LL_TOL = 1e-5
EM_KW = dict(num_iter=30, batch_perc=0.5, step_size=0.5, random_state=42, verbose=False)


def _json(name):
    with open(os.path.join(GOLD, 'spn_%s.json' % name)) as f:
        return json.load(f)


def _load(name):
    from deeprob.spn.structure.io import load_spn_json
    return load_spn_json(os.path.join(GOLD, 'spn_%s.json' % name))


def _check_mpe(name, spn, st, x, want, near):
    """Exact equality of the whole output outside the near-tie rows (at most 1 %); evidence bit-identical; no NaN left
    inside the scope; the workspace route gives the same bits."""
    from deeprob.spn.algorithms.inference import mpe
    got = mpe(spn, x)
    share = float(near.mean())
    print('mpe %-24s rows %5d set aside %d (%.2f %%)' % (name, len(x), int(near.sum()), 100 * share))
    report_measured('flat_spn_queries mpe set-aside share ' + name, share, 0.01)
    assert near.sum() <= 0.01 * len(x)
    assert got.dtype == np.float32 and got.shape == x.shape
    given = ~np.isnan(x)
    assert np.array_equal(got.view(np.uint32)[given], x.view(np.uint32)[given])
    assert not np.isnan(got[:, :spn.n_features]).any()
    assert np.array_equal(got[~near], want[~near], equal_nan=True)
    slots = spn.n_slots
    spn.n_slots = 0
    try:
        again = mpe(spn, x)
    finally:
        spn.n_slots = slots
    assert np.array_equal(again, got, equal_nan=True)
    return got


@pytest.mark.parametrize('circuit,vectors', [('binary16', 'binary16_nan'), ('mixed4', 'mixed4')])
def test_mpe_golden(circuit, vectors):
    g = np.load(os.path.join(GOLD, 'spn_%s.npz' % vectors))
    q = np.load(os.path.join(GOLD, 'spn_queries_%s.npz' % vectors))
    st = qref.State(_json(circuit))
    _, near = qref.mpe(st, g['x'], g['per_node'])
    _check_mpe(vectors, _load(circuit), st, g['x'], q['mpe'], near)


@pytest.mark.parametrize('n_features,seed,B', RANDOM_CASES)
def test_mpe_random_circuits(n_features, seed, B):
    from deeprob.spn.structure.io import digraph_to_spn
    from deeprob.hip import load_library
    d, family = random_circuit(n_features, seed)
    x = support_inputs(d, family, B, seed + 100)
    st = qref.State(d)
    want, near = qref.mpe(st, x)
    spn = digraph_to_spn(d)
    if n_features >= 12:
        rec = spn.circuit(torch.device('cuda', torch.cuda.current_device()))
        assert spn.n_nodes > 256
        assert load_library().dpk_flat_spn_topdown_workspace_bytes(B, ctypes.addressof(rec)) > 0     # workspace route
    _check_mpe('random %d' % n_features, spn, st, x, want, near)


def test_mpe_tensor_inplace_and_extra_columns():
    from deeprob.spn.algorithms.inference import mpe
    from deeprob.hip import HipError
    spn = _load('mixed4')
    x = np.load(os.path.join(GOLD, 'spn_mixed4.npz'))['x']
    base = mpe(spn, x)
    wide = np.full((len(x), 7), np.nan, np.float32)
    wide[:, :4] = x
    wide[:, 5] = 3.25
    out = mpe(spn, wide)
    assert np.array_equal(out[:, :4], base) and np.isnan(out[:, 4]).all() and np.isnan(out[:, 6]).all()
    assert np.array_equal(out[:, 5], wide[:, 5])
    t = torch.from_numpy(x).cuda()
    keep = t.clone()
    res = mpe(spn, t)
    assert isinstance(res, torch.Tensor) and res.is_cuda and res.data_ptr() != t.data_ptr()
    assert torch.equal(torch.isnan(t), torch.isnan(keep))                     # the input is untouched
    assert np.array_equal(res.cpu().numpy(), base)
    res2 = mpe(spn, t, inplace=True)
    assert res2.data_ptr() == t.data_ptr() and np.array_equal(t.cpu().numpy(), base)
    xin = x.copy()
    assert mpe(spn, xin, inplace=True) is xin and np.array_equal(xin, base)
    assert mpe(spn, np.zeros((0, 4), np.float32)).shape == (0, 4)
    with pytest.raises(ValueError):
        mpe(spn, np.zeros((3, 2), np.float32))
    with pytest.raises(HipError):
        mpe(spn, torch.zeros(3, 4))


@pytest.mark.parametrize('circuit,vectors', [('binary16', 'binary16'), ('binary16', 'binary16_nan'), ('mixed4', 'mixed4')])
def test_eval_backward_golden(circuit, vectors):
    from deeprob.spn.algorithms.gradient import eval_backward
    g = np.load(os.path.join(GOLD, 'spn_%s.npz' % vectors))
    q = np.load(os.path.join(GOLD, 'spn_queries_%s.npz' % vectors))
    table = np.ascontiguousarray(g['per_node'][:, :int(q['n_rows'])])
    spn = _load(circuit)
    grads = eval_backward(spn, table)
    assert grads.dtype == np.float32 and grads.shape == table.shape
    assert not np.isnan(grads).any()
    ok, floored, tail = eligible_rows(table)
    assert floored.mean() <= 0.05 and tail.mean() <= 0.01
    err = rel_err(grads[:, ok], q['grads'][:, ok])
    print('eval_backward %-14s rel_err %.3e on %d of %d rows' % (vectors, err, int(ok.sum()), len(ok)))
    report_measured('flat_spn_queries eval_backward ' + vectors, err, LL_TOL)
    assert err <= LL_TOL
    t = eval_backward(spn, torch.from_numpy(table).cuda())
    assert isinstance(t, torch.Tensor) and np.array_equal(t.cpu().numpy(), grads)
    with pytest.raises(ValueError):
        eval_backward(spn, table[:-1])


# Circuits without Uniform leaves: a Uniform leaf whose interval misses the input sits on the -1e31 floor, and with many
# such leaves per variable nearly every row has a node below -1e3, which leaves nothing to hold a bar on.
@pytest.mark.parametrize('n_features,seed,B', [(5, 0, 1), (7, 1, 63), (9, 2, 65), (12, 3, 300)])
def test_eval_backward_random_circuits(n_features, seed, B):
    from deeprob.spn.structure.io import digraph_to_spn
    from deeprob.spn.algorithms.inference import log_likelihood
    from deeprob.spn.algorithms.gradient import eval_backward
    d, family = random_circuit(n_features, seed, kinds=('Gaussian', 'Bernoulli', 'Categorical'))
    x = support_inputs(d, family, B, seed + 100)
    st = qref.State(d)
    table = qref.forward(st, x)
    want = qref.backward(st, table)
    spn = digraph_to_spn(d)
    grads = eval_backward(spn, table)
    assert not np.isnan(grads).any()
    ok, floored, tail = eligible_rows(table)
    assert floored.sum() <= 0.05 * B and tail.sum() <= 0.01 * B
    err = rel_err(grads[:, ok], want[:, ok])
    print('eval_backward random %2d rel_err %.3e on %d of %d rows' % (n_features, err, int(ok.sum()), B))
    report_measured('flat_spn_queries eval_backward random %d' % n_features, err, LL_TOL)
    assert err <= LL_TOL
    # on the device's own table too (log_likelihood -> eval_backward), all rows: no exception, no NaN
    _, own = log_likelihood(spn, x, return_results=True)
    assert not np.isnan(eval_backward(spn, own)).any()


def _em_errors(name, tag, got, g, key, bars):
    worst = 0.0
    for k, bar in zip(qref.GROUPS, bars):
        want = g['%s.%s' % (key, k)]
        if not len(want):
            continue
        err = grad_err(got[k], want)
        print('EM %-9s %-5s %-4s %-10s grad_err %.3e (bar %.1e)' % (name, tag, key, k, err, bar))
        report_measured('flat_spn_queries EM %s %s %s %s' % (name, tag, key, k), err, bar)
        worst = max(worst, err / bar)
    return worst


@pytest.mark.parametrize('name', ['binary16', 'mixed4'])
@pytest.mark.parametrize('tag', ['cold', 'rand'])
def test_em_one_iteration(name, tag):
    from deeprob.spn.learning import expectation_maximization
    g = np.load(os.path.join(GOLD, 'spn_em_%s.npz' % name))
    spn = _load(name)
    kw = dict(EM_KW, num_iter=1, random_init=(tag == 'rand'))
    assert expectation_maximization(spn, g['data'], **kw) is spn
    assert _em_errors(name, tag, qref.flat_params(spn), g, tag + '1', [1e-4] * 5) <= 1.0


@pytest.mark.parametrize('name', ['binary16', 'mixed4'])
@pytest.mark.parametrize('tag', ['cold', 'rand'])
def test_em_thirty_iterations(name, tag, tmp_path):
    from deeprob.spn.learning import expectation_maximization
    from deeprob.spn.algorithms.inference import log_likelihood
    from deeprob.spn.structure.io import load_spn_json, save_spn_json
    g = np.load(os.path.join(GOLD, 'spn_em_%s.npz' % name))
    spn = _load(name)
    kw = dict(EM_KW, random_init=(tag == 'rand'))
    expectation_maximization(spn, g['data'], **kw)
    got = qref.flat_params(spn)
    bars = [max(1e-4, 4.0 * float(dr)) for dr in g['dref_' + tag]]
    assert _em_errors(name, tag, got, g, tag + '30', bars) <= 1.0
    ll = log_likelihood(spn, g['data'])
    if name == 'binary16':
        gain, ref_gain = float(np.mean(ll)) - float(g['ll_start']), float(g['ll_' + tag]) - float(g['ll_start'])
        print('EM binary16 %s mean LL %.4f -> %.4f (reference -> %.4f)' % (tag, float(g['ll_start']), float(np.mean(ll)),
                                                                         float(g['ll_' + tag])))
        assert ref_gain > 0 and gain >= 0.5 * ref_gain
    # bitwise reproducible
    twin = _load(name)
    expectation_maximization(twin, g['data'], **kw)
    for k, v in qref.flat_params(twin).items():
        assert np.array_equal(v, got[k]), k
    # the new parameters are what every later call sees: a device tensor, and the circuit written and read back
    ll_t = log_likelihood(spn, torch.from_numpy(g['data']).cuda()).cpu().numpy()
    assert np.array_equal(ll_t, ll)
    path = str(tmp_path / 'learned.json')
    save_spn_json(spn, path)
    assert rel_err(log_likelihood(load_spn_json(path), g['data']), ll) <= LL_TOL
    # ... and they are the helper's view of the same circuit
    st = qref.State(json.load(open(path)))
    assert rel_err(ll, qref.forward(st, g['data'])[0]) <= LL_TOL


def test_em_rejects_nan_and_verbose_runs(capsys):
    from deeprob.spn.learning import expectation_maximization
    g = np.load(os.path.join(GOLD, 'spn_em_binary16.npz'))
    bad = g['data'].copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError):
        expectation_maximization(_load('binary16'), bad, **EM_KW)
    a, b = _load('binary16'), _load('binary16')
    expectation_maximization(a, g['data'], **dict(EM_KW, num_iter=3, verbose=True))
    expectation_maximization(b, torch.from_numpy(g['data']).cuda(), **dict(EM_KW, num_iter=3))
    for k, v in qref.flat_params(a).items():
        assert np.array_equal(v, qref.flat_params(b)[k]), k
    assert a.em_mean_ll.shape == (3,) and bool(torch.isfinite(a.em_mean_ll).all())


@pytest.mark.parametrize('case', ['mixed4', 'random7', 'random12'])
def test_sample_replay(case):
    """The helper, fed the seed and the documented counters, reproduces the draws."""
    from deeprob.spn.structure.io import digraph_to_spn
    from deeprob.spn.algorithms.sampling import sample
    if case == 'mixed4':
        d = _json('mixed4')
        x = np.load(os.path.join(GOLD, 'spn_mixed4.npz'))['x'].copy()
        x[2, 0] = np.nan
        family = ['Gaussian', 'Gaussian', 'Categorical', 'Bernoulli']
    else:
        nf, seed, B = {'random7': (7, 1, 1000), 'random12': (12, 3, 500)}[case]
        d, family = random_circuit(nf, seed)
        x = support_inputs(d, family, B, seed + 100)
    spn = digraph_to_spn(d)
    got = sample(spn, x, seed=1234)
    want, near = qref.sample_replay(qref.State(d), x, 1234, spn.n_features)
    share = float(near.mean())
    print('sample replay %-9s rows %5d set aside %d (%.2f %%)' % (case, len(x), int(near.sum()), 100 * share))
    report_measured('flat_spn_queries sample replay set-aside share ' + case, share, 0.01)
    assert near.sum() <= 0.01 * len(x)
    assert not np.isnan(got[:, :spn.n_features]).any()
    given = ~np.isnan(x)
    assert np.array_equal(got.view(np.uint32)[given], x.view(np.uint32)[given])
    discrete = np.array([f in ('Bernoulli', 'Categorical') for f in family])
    keep = ~near
    assert np.array_equal(got[keep][:, discrete], want[keep][:, discrete])
    err = rel_err(got[keep][:, ~discrete], want[keep][:, ~discrete])
    print('sample replay %-9s continuous rel_err %.3e' % (case, err))
    assert err <= LL_TOL
    slots = spn.n_slots
    spn.n_slots = 0
    try:
        assert np.array_equal(sample(spn, x, seed=1234), got)
    finally:
        spn.n_slots = slots


def _marginal(spn, assign):
    from deeprob.spn.algorithms.inference import log_likelihood
    x = np.full((1, spn.n_features), np.nan, np.float32)
    for v, val in assign.items():
        x[0, v] = val
    return float(np.exp(np.float64(log_likelihood(spn, x)[0])))


def test_sample_distribution():
    from deeprob.spn.algorithms.sampling import sample
    N = 1 << 18
    spn = _load('binary16')
    s = sample(spn, torch.full((N, 16), float('nan'), device='cuda'), seed=2024).cpu().numpy()
    assert np.isin(s, (0.0, 1.0)).all()
    worst = 0.0
    for v in range(16):
        p = _marginal(spn, {v: 1.0})
        worst = max(worst, abs(float(s[:, v].mean()) - p) / np.sqrt(p * (1 - p) / N))
    for a, b in [(0, 1), (2, 9), (3, 4), (5, 15), (6, 7), (8, 12), (10, 11), (13, 14)]:
        p = _marginal(spn, {a: 1.0, b: 1.0})
        worst = max(worst, abs(float((s[:, a] * s[:, b]).mean()) - p) / np.sqrt(p * (1 - p) / N))
    mixed = _load('mixed4')
    m = sample(mixed, torch.full((N, 4), float('nan'), device='cuda'), seed=2025).cpu().numpy()
    p = _marginal(mixed, {3: 1.0})
    assert abs(p - 0.44375) < 1e-6
    z3 = abs(float(m[:, 3].mean()) - p) / np.sqrt(p * (1 - p) / N)
    print('sample distribution: worst deviation %.2f sigma (binary16), %.2f sigma (mixed4 variable 3)' % (worst, z3))
    assert worst <= 5.0 and z3 <= 5.0


def test_sample_conditional_and_seeds():
    from deeprob.spn.structure.io import digraph_to_spn
    from deeprob.spn.algorithms.sampling import sample
    d, family = random_circuit(9, 2)
    spn = digraph_to_spn(d)
    x = support_inputs(d, family, 2000, 77, nan_rate=0.0)
    x[:, ::2] = np.nan                       # half the columns given
    x[0, :] = np.nan                         # (and one row with nothing given)
    out = sample(spn, x, seed=5)
    given = ~np.isnan(x)
    assert given[1:, 1::2].all() and not given[:, ::2].any()
    assert np.array_equal(out.view(np.uint32)[given], x.view(np.uint32)[given])
    assert not np.isnan(out).any()
    lo, hi = {}, {}
    for n in d['nodes']:
        if n['class'] == 'Uniform':
            v, p = n['scope'][0], n['params']
            lo[v] = min(lo.get(v, np.inf), p['start'])
            hi[v] = max(hi.get(v, -np.inf), p['start'] + p['width'])
    for v, f in enumerate(family):
        if v % 2:
            continue
        assert not np.isnan(out[:, v]).any()
        if f == 'Categorical':
            assert np.isin(out[:, v], (0, 1, 2, 3, 4)).all()
        elif f == 'Bernoulli':
            assert np.isin(out[:, v], (0, 1)).all()
        elif f == 'Uniform':
            assert (out[:, v] >= np.float32(lo[v])).all() and (out[:, v] <= np.float32(hi[v]) + 1e-6).all()
    assert np.array_equal(sample(spn, x, seed=5), out)
    assert not np.array_equal(sample(spn, x, seed=6), out)
    torch.manual_seed(11)
    a = sample(spn, x)
    torch.manual_seed(11)
    assert np.array_equal(sample(spn, x), a)
    t = torch.from_numpy(x).cuda()
    r = sample(spn, t, inplace=True, seed=5)
    assert r.data_ptr() == t.data_ptr() and np.array_equal(t.cpu().numpy(), out)


def test_abi_errors():
    """Null pointers, bad sizes, short workspaces and empty batches of the new entry points."""
    from deeprob.hip import load_library
    from deeprob.spn.structure.io import digraph_to_spn
    lib = load_library()
    dev = torch.device('cuda', torch.cuda.current_device())
    EINVAL, EWORKSPACE = -1, -2
    spn = _load('mixed4')
    rec = spn.circuit(dev)
    c = ctypes.addressof(rec)
    x = torch.full((8, 4), float('nan'), device=dev)
    lls = torch.zeros((spn.n_nodes, 8), device=dev)
    grads = torch.empty_like(lls)
    idx = torch.arange(8, dtype=torch.int32, device=dev)
    data = torch.zeros((8, 4), device=dev)

    def bad(**kw):
        r = spn.circuit(dev)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    # top-down
    assert lib.dpk_flat_spn_topdown(None, 8, 4, c, 0, 0, None, 0, None) == EINVAL
    assert b'null' in lib.dpk_last_error()
    assert lib.dpk_flat_spn_topdown(x.data_ptr(), 8, 4, None, 0, 0, None, 0, None) == EINVAL
    assert lib.dpk_flat_spn_topdown(x.data_ptr(), 8, 4, c, 2, 0, None, 0, None) == EINVAL
    assert lib.dpk_flat_spn_topdown(x.data_ptr(), 8, 2, c, 0, 0, None, 0, None) == EINVAL          # D < n_vars
    assert lib.dpk_flat_spn_topdown(x.data_ptr(), -1, 4, c, 0, 0, None, 0, None) == EINVAL
    r = bad(n_nodes=0)
    assert lib.dpk_flat_spn_topdown(x.data_ptr(), 8, 4, ctypes.addressof(r), 0, 0, None, 0, None) == EINVAL
    assert lib.dpk_flat_spn_topdown_workspace_bytes(8, ctypes.addressof(r)) == EINVAL
    r = bad(order=None)
    assert lib.dpk_flat_spn_topdown(x.data_ptr(), 8, 4, ctypes.addressof(r), 0, 0, None, 0, None) == EINVAL
    assert lib.dpk_flat_spn_topdown(None, 0, 4, c, 0, 0, None, 0, None) == 0                        # B == 0: no launch
    assert lib.dpk_flat_spn_topdown_workspace_bytes(8, c) == 0                                      # on-chip route
    r = bad(n_slots=0)
    need = lib.dpk_flat_spn_topdown_workspace_bytes(8, ctypes.addressof(r))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    assert lib.dpk_flat_spn_topdown(x.data_ptr(), 8, 4, ctypes.addressof(r), 0, 0, ws.data_ptr(), need - 1, None) == EWORKSPACE
    assert b'workspace' in lib.dpk_last_error()
    assert lib.dpk_flat_spn_topdown(x.data_ptr(), 8, 4, ctypes.addressof(r), 0, 0, None, 0, None) == EWORKSPACE
    # backward
    assert lib.dpk_flat_spn_backward(None, grads.data_ptr(), 8, c, None) == EINVAL
    assert lib.dpk_flat_spn_backward(lls.data_ptr(), None, 8, c, None) == EINVAL
    assert lib.dpk_flat_spn_backward(lls.data_ptr(), grads.data_ptr(), 8, None, None) == EINVAL
    assert lib.dpk_flat_spn_backward(lls.data_ptr(), grads.data_ptr(), -1, c, None) == EINVAL
    r = bad(n_nodes=-3)
    assert lib.dpk_flat_spn_backward(lls.data_ptr(), grads.data_ptr(), 8, ctypes.addressof(r), None) == EINVAL
    assert lib.dpk_flat_spn_backward(None, None, 0, c, None) == 0
    # EM step
    need = lib.dpk_flat_spn_em_step_workspace_bytes(8, c)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    args = (data.data_ptr(), 8, 4, idx.data_ptr(), 8, c, 0.5, None, ws.data_ptr(), need, None)

    def em(**kw):
        names = ('x', 'N', 'D', 'index', 'B', 'c', 'step', 'mean', 'ws', 'ws_bytes', 'stream')
        a = dict(zip(names, args))
        a.update(kw)
        return lib.dpk_flat_spn_em_step(*[a[k] for k in names])

    assert em(x=None) == EINVAL and em(index=None) == EINVAL and em(c=None) == EINVAL
    assert em(step=0.0) == EINVAL and em(step=1.0) == EINVAL and em(D=2) == EINVAL and em(B=-1) == EINVAL
    r = bad(n_nodes=0)
    assert em(c=ctypes.addressof(r)) == EINVAL
    assert lib.dpk_flat_spn_em_step_workspace_bytes(8, ctypes.addressof(r)) == EINVAL
    assert em(ws_bytes=need - 1) == EWORKSPACE and em(ws=None) == EWORKSPACE
    assert em(B=0, x=None, index=None, ws=None, ws_bytes=0) == 0
    # a sum node with more than 255 children is outside the top-down kernel
    r = bad(max_children=300)
    assert lib.dpk_flat_spn_topdown(x.data_ptr(), 8, 4, ctypes.addressof(r), 0, 0, None, 0, None) == -4
    torch.cuda.synchronize()
