"""Mixtures of Chow-Liu trees on the device: the two ``dpc_mix_*`` entry points on poisoned, guard-banded memory
(tests/buffer_contract.py) against the float64 restatement (tests/clt_mixture_ref.py), ``BinaryCLT.em_step`` and
``BinaryCLTMixture`` (``em``, ``fit``, ``to_pc``, ``expectation_maximization``) against the reference's golden run.

Bounds.  ``comp_ll`` is bitwise ``BinaryCLT.log_likelihood``.  ``|ll - want| <= 2^-23 (max_k |a_k| + K + 4)`` with ``want`` the
float64 mixing of the device's own ``comp_ll`` (derived in tests/clt_mixture_ref.ll_bound, checked on the host).  A row of
``resp`` sums to 1 within ``K 2^-22``; an entry is within ``2^-25 max_k |a_k| + 2^-21`` of the float64 one (the rounding of
the a_k themselves through the softmax's derivative, then a few relative ulp of numbers <= 1:
tests/clt_mixture_ref.resp_bound).  ``stats``: every
entry within ``(nb + 8) nb 2^-53`` of the float64 sums of the device's ``resp`` (the worst case of any order over nb terms
<= 1, as tests/test_learn_cont_gpu.py bounds its sums), and bitwise equal on a second run.  EM: every probability within 1e-4
of the reference's after one iteration and within max(1e-4, 4 dref) after 30."""
import numpy as np
import pytest
import torch

from tests import clt_mixture_ref as mref
from tests import clt_ref
from tests.buffer_contract import PATTERNS, contract

pytestmark = pytest.mark.gpu
B_ROWS = 900
EM_KW = dict(batch_perc=0.5, step_size=0.5, random_state=42, verbose=False)
_cache = {}


def bar(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def random_trees(d, k, seed):
    """``k`` random trees over ``d`` positions with random CPTs: ``[(bfs, tree, params)]`` (bfs: the package's order)."""
    from deeprob.utils.graph import compute_bfs_ordering
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(k):
        order = rs.permutation(d)
        tree = np.full(d, -1, np.int32)
        for i in range(1, d):
            tree[order[i]] = order[rs.randint(0, i)]
        probs = 0.05 + 0.9 * rs.rand(d, 2)
        probs[order[0], 0] = probs[order[0], 1]
        params = np.log(np.stack([1.0 - probs, probs], axis=2)).astype(np.float32)
        out.append((np.asarray(compute_bfs_ordering(tree), np.int32), tree, params))
    return out


def case(d, k):
    """``(trees, logw, rows x with 30 % NaN and an all-NaN row, complete rows, a shuffled batch index)``; once per (d, k)."""
    if (d, k) not in _cache:
        rs = np.random.RandomState(100 * d + k)
        complete = (rs.rand(B_ROWS, d) < 0.5).astype(np.float32)
        x = complete.copy()
        x[rs.rand(B_ROWS, d) < 0.3] = np.nan
        x[5] = np.nan
        x[6] = complete[6]
        logw = np.log(rs.dirichlet(np.ones(k))).astype(np.float32)
        _cache[(d, k)] = (random_trees(d, k, d + k), logw, x, complete, rs.permutation(B_ROWS).astype(np.int32))
    return _cache[(d, k)]


def device_mixture(trees, logw):
    from deeprob.hip import clt as C
    return C.DeviceMixture(trees, logw, torch.device('cuda', torch.cuda.current_device()))


def check_likelihood(trees, logw, x, rows):
    """One ``dpc_mix_log_likelihood`` under both poisons against the restatement; returns the device's ``resp``."""
    from deeprob.hip import clt as C
    from deeprob.spn.structure.cltree import BinaryCLT
    k, d = len(trees), x.shape[1]
    mix = device_mixture(trees, logw)
    xd = torch.from_numpy(x).cuda()
    rd = None if rows is None else torch.from_numpy(rows).cuda()
    picked = x if rows is None else x[rows]
    for pattern in PATTERNS:
        with contract(pattern) as c:
            codes = C.pack_query(xd)
            c.check()
            c.frozen(codes, rd, mix._buf)
            ll, comp_ll, resp = c.expect_written(*C.mixture_codes_log_likelihood(mix, codes, rd))
        comp_ll, ll, resp = comp_ll.cpu().numpy(), ll.cpu().numpy(), resp.cpu().numpy()
        assert comp_ll.shape == (len(picked), k) and ll.shape == (len(picked),) and resp.shape == comp_ll.shape
        for j, (bfs, tree, params) in enumerate(trees):         # bit for bit the tree's own query
            alone = BinaryCLT(list(range(d)), tree=tree.copy(), params=params.copy()).log_likelihood(picked)[:, 0]
            assert np.array_equal(comp_ll[:, j], alone), j
        want_ll, want_resp = mref.mix(comp_ll, logw)
        err, bound = np.abs(ll.astype(np.float64) - want_ll), mref.ll_bound(comp_ll, logw)
        print('mix ll d %d K %d nb %d: worst |ll - want| / bound %.3f' % (d, k, len(picked), float(np.max(err / bound))))
        assert (err <= bound).all()
        assert (np.abs(resp.astype(np.float64).sum(axis=1) - 1.0) <= k * 2.0 ** -22).all()
        assert (np.abs(resp.astype(np.float64) - want_resp) <= mref.resp_bound(comp_ll, logw)[:, None]).all()
        # ... and the restatement's tree pass gives the same component values at the project's bar
        assert bar(comp_ll, mref.component_lls([(b, t) for b, t, _ in trees], [p for _, _, p in trees], picked)) <= 1e-5
    return resp


# ---- dpc_mix_log_likelihood ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb', [1, 255, 256, 257, 700])
@pytest.mark.parametrize('d,k', [(1, 1), (2, 2), (7, 3), (65, 2)])
def test_mix_log_likelihood(d, k, nb):
    trees, logw, x, _, perm = case(d, k)
    check_likelihood(trees, logw, x, perm[:nb].copy())


@pytest.mark.parametrize('d,k', [(1, 2), (7, 1), (65, 3)])
def test_mix_log_likelihood_all_rows_in_order(d, k):
    trees, logw, x, _, _ = case(d, k)
    check_likelihood(trees, logw, x, None)


def test_mix_log_likelihood_excluded_component_and_impossible_row():
    """A component with logw = -inf has no share; a row impossible under every component gets ll = -inf, resp = 0."""
    from deeprob.hip import clt as C
    trees, _, x, complete, _ = case(7, 3)
    logw = np.asarray([np.log(0.25), -np.inf, np.log(0.75)], np.float32)
    resp = check_likelihood(trees, logw, complete[:64], None)
    assert (resp[:, 1] == 0).all()
    # every tree: position 0 is never 1 under any parent value
    hard = []
    for bfs, tree, params in trees:
        p = params.copy()
        p[0, :, 1], p[0, :, 0] = -np.inf, 0.0
        hard.append((bfs, tree, p))
    rows = complete[:64].copy()
    rows[:, 0] = 1.0
    rows[1, 0] = 0.0
    rows[2, 0] = np.nan
    mix = device_mixture(hard, np.log(np.asarray([0.2, 0.3, 0.5], np.float32)))
    ll, comp_ll, resp = (t.cpu().numpy() for t in C.mixture_codes_log_likelihood(mix, C.pack_query(torch.from_numpy(rows).cuda())))
    possible = np.zeros(64, bool)
    possible[[1, 2]] = True
    assert (ll[~possible] == -np.inf).all() and (resp[~possible] == 0).all() and (comp_ll[~possible] == -np.inf).all()
    assert np.isfinite(ll[possible]).all() and np.allclose(resp[possible].sum(axis=1), 1.0, atol=3 * 2.0 ** -22)


def test_mix_log_likelihood_in_pieces_and_a_bad_row_index(monkeypatch):
    from deeprob.hip import clt as C
    trees, logw, x, _, _ = case(7, 3)
    mix = device_mixture(trees, logw)
    xd = torch.from_numpy(x).cuda()
    whole = C.mixture_log_likelihood(mix, xd, want_resp=True)
    monkeypatch.setattr(C, 'query_rows', lambda d: 256)
    for a, b in zip(whole, C.mixture_log_likelihood(mix, xd, want_resp=True)):
        assert torch.equal(a, b)
    # an index outside the rows reads nothing: NaN there, the other positions as they are
    rows = torch.tensor([3, -1, B_ROWS, 4], dtype=torch.int32, device='cuda')
    ll = C.mixture_log_likelihood(mix, xd, rows).cpu().numpy()
    assert np.isnan(ll[1:3]).all() and np.array_equal(ll[[0, 3]], whole[0].cpu().numpy()[[3, 4]])


def test_mix_log_likelihood_without_scratch():
    """``work`` = NULL, what EM passes for rows it has checked: complete rows get the same bits, a row with NaN gets NaN, and
    nothing is written anywhere else (the outputs sit between guard bands)."""
    from deeprob.hip import clt as C
    trees, logw, x, complete, perm = case(65, 2)
    mix = device_mixture(trees, logw)
    rows = torch.from_numpy(perm[:300].copy()).cuda()
    codes = C.pack_query(torch.from_numpy(complete).cuda())
    with_work = C.mixture_codes_log_likelihood(mix, codes, rows)
    for pattern in PATTERNS:
        with contract(pattern) as c:
            c.frozen(codes, rows, mix._buf)
            without = c.expect_written(*C.mixture_codes_log_likelihood(mix, codes, rows, complete=True))
        for a, b in zip(with_work, without):
            assert torch.equal(a, b)
    mixed = complete[:64].copy()
    mixed[3, 7] = np.nan
    ll, comp_ll, resp = (t.cpu().numpy() for t in C.mixture_codes_log_likelihood(
        mix, C.pack_query(torch.from_numpy(mixed).cuda()), complete=True))
    holds_nan = np.arange(64) == 3
    assert np.isnan(ll[holds_nan]).all() and np.isnan(comp_ll[holds_nan]).all() and np.isnan(resp[holds_nan]).all()
    assert np.isfinite(ll[~holds_nan]).all() and np.isfinite(resp[~holds_nan]).all()


# ---- dpc_mix_em_stats ----------------------------------------------------------------------------------------------------------
def check_stats(trees, logw, complete, rows):
    from deeprob.hip import clt as C
    k, d = len(trees), complete.shape[1]
    mix = device_mixture(trees, logw)
    codes = C.pack_query(torch.from_numpy(complete).cuda())
    rd = None if rows is None else torch.from_numpy(rows).cuda()
    picked = complete if rows is None else complete[rows]
    nb = len(picked)
    resp = C.mixture_codes_log_likelihood(mix, codes, rd)[2]
    want = mref.em_stats(picked, resp.cpu().numpy(), [t for _, t, _ in trees])
    runs = []
    for pattern in PATTERNS:
        with contract(pattern) as c:
            c.frozen(codes, rd, resp, mix._buf)
            stats = c.expect_written(C.mixture_em_stats(mix, codes, rd, resp))
        runs.append(stats.cpu().numpy())
    got = runs[0]
    assert got.shape == (k, 1 + 2 * d) and got.dtype == np.float64
    assert np.array_equal(runs[0], runs[1])                             # a second run: the same bits
    err = float(np.max(np.abs(got - want)))
    print('em stats d %d K %d nb %d: worst error %.3e (bound %.3e)' % (d, k, nb, err, (nb + 8) * nb * 2.0 ** -53))
    assert err <= (nb + 8) * nb * 2.0 ** -53
    for j, (bfs, tree, _) in enumerate(trees):
        assert got[j, 1 + d + int(bfs[0])] == 0.0                        # the root has no parent
    assert np.allclose(got[:, 0].sum(), nb, atol=1e-3)
    return got


@pytest.mark.parametrize('nb', [1, 255, 256, 257, 700])
@pytest.mark.parametrize('d,k', [(1, 1), (2, 2), (7, 3), (65, 2)])
def test_mix_em_stats(d, k, nb):
    trees, logw, _, complete, perm = case(d, k)
    check_stats(trees, logw, complete, perm[:nb].copy())


@pytest.mark.parametrize('d,k', [(2, 3), (65, 1)])
def test_mix_em_stats_all_rows_in_order(d, k):
    trees, logw, _, complete, _ = case(d, k)
    check_stats(trees, logw, complete, None)


def test_mix_em_stats_more_than_one_chunk_and_missing_codes():
    """Past DPC_MIX_CHUNK positions the chunk sums are added in chunk order; a DPC_MISSING code counts as 0."""
    from deeprob.hip import clt as C
    trees, logw, x, complete, _ = case(7, 3)
    rows = np.random.RandomState(0).randint(0, B_ROWS, size=2 * C.DPC_MIX_CHUNK + 77).astype(np.int32)
    check_stats(trees, logw, complete, rows)
    mix = device_mixture(trees, logw)
    resp = torch.rand((B_ROWS, 3), generator=torch.Generator().manual_seed(1)).cuda()
    with_nan = C.mixture_em_stats(mix, C.pack_query(torch.from_numpy(x).cuda()), None, resp).cpu().numpy()
    as_zero = C.mixture_em_stats(mix, C.pack_query(torch.from_numpy(np.nan_to_num(x)).cuda()), None, resp).cpu().numpy()
    assert np.array_equal(with_nan, as_zero)


# ---- the golden run ------------------------------------------------------------------------------------------------------------
def given():
    g = mref.golden()
    data = clt_ref.unpack(g['data'], int(g['n_rows']), int(g['n_vars']))
    return g, data


def mixture(g):
    from deeprob.spn.structure import BinaryCLTMixture
    from deeprob.spn.structure.cltree import BinaryCLT
    scope = list(range(int(g['n_vars'])))
    return BinaryCLTMixture(scope, [BinaryCLT(scope, tree=t.copy(), params=p.copy()) for t, p in zip(g['tree'], g['params'])],
                            g['weights'].copy())


def test_em_step_of_one_tree():
    from deeprob.spn.structure.cltree import BinaryCLT
    g, data = given()
    for as_tensor in (False, True):
        clt = BinaryCLT(list(range(16)), tree=g['tree'][0].copy(), params=g['params'][0].copy())
        x, stats = data[g['step_rows']], g['step_stats']
        if as_tensor:
            x, stats = torch.from_numpy(x).cuda(), torch.from_numpy(stats).cuda()
        clt.em_step(stats, x, 0.5)
        assert clt.params.dtype == np.float32 and clt.params.shape == (16, 2, 2)
        assert np.max(np.abs(np.exp(clt.params.astype(np.float64)) - np.exp(g['step_params'].astype(np.float64)))) <= 1e-4
    with pytest.raises(ValueError, match='NaN'):
        clt.em_step(g['step_stats'], np.where(np.arange(16) == 3, np.nan, data[g['step_rows']]).astype(np.float32), 0.5)


@pytest.mark.parametrize('tag', ['cold', 'rand'])
def test_em_one_iteration(tag):
    g, data = given()
    m = mixture(g)
    assert m.em(data, num_iter=1, random_init=(tag == 'rand'), **EM_KW) is m
    errs = mref.prob_err(m.weights, np.stack([c.params for c in m.components]), g[tag + '1.weights'], g[tag + '1.params'])
    print('EM %s 1 iteration: weights %.3e CPTs %.3e (bar 1e-4)' % (tag, errs[0], errs[1]))
    assert m.weights.dtype == np.float32 and max(errs) <= 1e-4


@pytest.mark.parametrize('tag', ['cold', 'rand'])
def test_em_thirty_iterations(tag):
    from deeprob.spn.algorithms.inference import log_likelihood
    from deeprob.spn.learning import expectation_maximization
    g, data = given()
    kw = dict(EM_KW, num_iter=30, random_init=(tag == 'rand'))
    m = mixture(g)
    before = m.log_likelihood(data)
    assert abs(float(np.mean(before)) - float(g['ll_start'])) <= 1e-4
    m.em(data, **kw)
    got_p = np.stack([c.params for c in m.components])
    errs = mref.prob_err(m.weights, got_p, g[tag + '30.weights'], g[tag + '30.params'])
    bars = [max(1e-4, 4.0 * float(d)) for d in g['dref_' + tag]]
    print('EM %s 30 iterations: weights %.3e (bar %.1e) CPTs %.3e (bar %.1e)' % (tag, errs[0], bars[0], errs[1], bars[1]))
    assert errs[0] <= bars[0] and errs[1] <= bars[1]
    ll = m.log_likelihood(data)
    gain, ref_gain = float(np.mean(ll)) - float(g['ll_start']), float(g['ll_' + tag]) - float(g['ll_start'])
    assert ref_gain > 0 and gain >= 0.5 * ref_gain
    assert m.em_mean_ll.shape == (30,) and bool(torch.isfinite(m.em_mean_ll).all())
    # bitwise reproducible on a twin; the same through expectation_maximization; the same from a device tensor
    for run in (lambda t: t.em(data, **kw), lambda t: expectation_maximization(t, data, **kw),
                lambda t: t.em(torch.from_numpy(data).cuda(), **kw)):
        twin = mixture(g)
        assert run(twin) is twin
        assert np.array_equal(twin.weights, m.weights)
        assert np.array_equal(np.stack([c.params for c in twin.components]), got_p)
    assert np.array_equal(m.log_likelihood(torch.from_numpy(data).cuda()).cpu().numpy(), ll)
    # the circuit of the trained mixture, on rows with NaN (the untrained one: test_to_pc_and_queries)
    q = data[:200].copy()
    q[np.random.RandomState(2).rand(*q.shape) < 0.3] = np.nan
    assert bar(np.asarray(log_likelihood(m.to_pc(), q)), m.log_likelihood(q)) <= 1e-5


def test_em_rejects_nan_and_verbose_runs(capsys):
    g, data = given()
    bad = data.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match='NaN'):
        mixture(g).em(bad, num_iter=1, **EM_KW)
    mixture(g).em(data, num_iter=2, **dict(EM_KW, verbose=True))


def test_to_pc_and_queries():
    from deeprob.spn.algorithms.inference import log_likelihood
    g, data = given()
    m = mixture(g)
    q = data[:300].copy()
    q[np.random.RandomState(1).rand(*q.shape) < 0.3] = np.nan
    q[0] = np.nan
    ll = m.log_likelihood(q)
    assert ll.shape == (300, 1) and ll.dtype == np.float32 and abs(float(ll[0, 0])) <= 1e-5
    assert bar(np.asarray(log_likelihood(m.to_pc(), q)), ll) <= 1e-5
    assert np.allclose(m.likelihood(q), np.exp(ll))
    resp = m.responsibilities(q)
    assert resp.shape == (300, 2) and np.allclose(resp.sum(axis=1), 1.0, atol=1e-6)
    assert np.allclose(resp[0], m.weights, atol=1e-6)                   # the all-NaN row: the prior of the components
    trees = [(clt_ref.bfs_order(t), t) for t in g['tree']]
    want_ll, want_resp = mref.mix(mref.component_lls(trees, g['params'], q), np.log(g['weights']))
    assert bar(ll, want_ll) <= 1e-5 and np.max(np.abs(resp - want_resp)) <= 1e-5
    assert m.params_count() == 2 + sum(c.params_count() for c in m.components)
    as_tensor = m.log_likelihood(torch.from_numpy(q).cuda())
    assert as_tensor.is_cuda and np.array_equal(as_tensor.cpu().numpy(), ll)


@pytest.mark.parametrize('how', ['kmeans', 'clusters'])
def test_fit(how):
    from deeprob.spn.structure import BinaryCLTMixture
    from deeprob.spn.structure.cltree import BinaryCLT
    g, data = given()
    scope, domain = list(range(16)), [[0, 1]] * 16
    m = BinaryCLTMixture(scope)
    draws = np.random.RandomState(5)
    if how == 'clusters':
        # the two clusters by their distance to the first row's pattern; label values need not be 0 .. K-1
        given_labels = np.where((data != data[0]).sum(axis=1) > 8, 7, 3)
        assert m.fit(data, domain, random_state=5, clusters=given_labels) is m
        assert np.array_equal(m.labels, given_labels)
    else:
        assert m.fit(data, domain, n_components=2, random_state=5) is m
        for _ in range(5):                                              # the seeds of the five restarts come first
            draws.choice(600, 2, replace=False)
    labels = m.labels
    present = np.unique(labels)
    assert len(present) == 2 and len(m.components) == 2 and m.weights.dtype == np.float32
    sizes = np.asarray([(labels == v).sum() for v in present])
    assert np.array_equal(m.weights, (sizes / 600.0).astype(np.float32)) and sizes.min() >= 150    # (a 40 / 60 split)
    # the k-means finds the two clusters the rows were drawn from: the split by distance to the first row's pattern
    far = (data != data[0]).sum(axis=1) > 8
    agree = np.mean((labels == present[0]) == far)
    assert max(agree, 1.0 - agree) >= 0.98
    for c, value in zip(m.components, present):                          # each tree: BinaryCLT.fit on its slice
        root = int(draws.choice(16))
        alone = BinaryCLT(scope, root=scope[root])
        alone.fit(data[labels == value], domain, alpha=0.1)
        assert c.root == root and np.array_equal(alone.tree, c.tree) and np.array_equal(alone.params, c.params)
    assert np.isfinite(m.log_likelihood(data)).all()
