"""BinaryCLT on the device: the counting kernels against integer numpy, ``fit`` against the reference's goldens, the
three queries against the goldens and the numpy restatement (tests/clt_ref.py), and every entry point of
include/deeprob_clt.h on poisoned, guard-banded memory (tests/buffer_contract.py).

Tolerances: counts and trees are exact; ``params`` within 1e-6 in log space (the tolerance test_classifier uses for
weights); log likelihoods at the project's bar |got - want| / max(1, |want|) <= 1e-5."""
import numpy as np
import pytest
import torch

from tests import clt_ref as ref
from tests.buffer_contract import PATTERNS, contract

pytestmark = pytest.mark.gpu
_models = {}


def bar(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def fitted(name):
    """The package's model fitted on a fixture's training rows (numpy input); once."""
    from deeprob.spn.structure.cltree import BinaryCLT
    if name not in _models:
        g = ref.golden(name)
        d = int(g['n_vars'])
        clt = BinaryCLT(list(range(d)), root=None if int(g['root']) < 0 else int(g['root']))
        clt.fit(g['x'], [[0, 1]] * d, alpha=float(g['alpha']),
                random_state=None if int(g['random_state']) < 0 else int(g['random_state']))
        _models[name] = clt
    return _models[name]


def device_tree(name):
    from deeprob.hip import clt as C
    m = fitted(name)
    return C.DeviceTree(m.bfs, m.tree, m.params, torch.device('cuda', torch.cuda.current_device()))


# ---- packing and counting ------------------------------------------------------------------------------------------------
def planes_of(x):
    """[D, W] uint64: bit r % 64 of word r // 64 of column c is x[r, c]; the bits past the last row are zero."""
    n, d = x.shape
    w = (n + 63) // 64
    bits = np.zeros((d, w * 64), np.uint64)
    bits[:, :n] = x.T
    return (bits.reshape(d, w, 64) << np.arange(64, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


@pytest.mark.parametrize('d', [1, 2, 33, 65, 130])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 4097])
def test_pack_bits_and_pair_counts_are_exact(n, d):
    from deeprob.hip import clt as C
    x = (np.random.RandomState(1000 * d + n).rand(n, d) < 0.3).astype(np.float32)
    want = x.astype(np.int64).T @ x.astype(np.int64)
    xd = torch.from_numpy(x).cuda()
    for pattern in PATTERNS:
        with contract(pattern) as c:
            c.frozen(xd)
            planes = c.expect_written(C.pack_bits(xd))
            c.check()
            c.frozen(planes)
            ones = c.expect_written(C.pair_counts(planes))
        assert planes.shape == (d, (n + 63) // 64) and ones.dtype == torch.int32
        assert np.array_equal(planes.cpu().numpy().view(np.uint64), planes_of(x))        # (tail bits zero included)
        assert np.array_equal(ones.cpu().numpy().astype(np.int64), want)


@pytest.mark.parametrize('b,d', [(1, 1), (63, 33), (65, 65), (257, 130)])
def test_pack_query_codes(b, d):
    from deeprob.hip import clt as C
    rs = np.random.RandomState(b + d)
    x = (rs.rand(b, d) < 0.5).astype(np.float32)
    x[rs.rand(b, d) < 0.4] = np.nan
    xd = torch.from_numpy(x).cuda()
    for pattern in PATTERNS:
        with contract(pattern) as c:
            c.frozen(xd)
            codes = c.expect_written(C.pack_query(xd))
        assert np.array_equal(codes.cpu().numpy(), ref.codes(x).T.astype(np.uint8))


def test_entry_points_reject_what_the_header_excludes():
    from deeprob.hip import HipError, clt as C
    lib = C.load_library()
    x = torch.zeros((4, 4), device='cuda')
    out = torch.empty(64, dtype=torch.int64, device='cuda')
    assert C.DPC_MAX_D >= 1024
    for args in ((x.data_ptr(), 4, C.DPC_MAX_D + 1, out.data_ptr(), None), (x.data_ptr(), 0, 4, out.data_ptr(), None),
                 (None, 4, 4, out.data_ptr(), None)):
        assert lib.dpc_pack_bits(*args) == C.DPC_EINVAL and lib.dpc_last_error()
    assert lib.dpc_pair_counts(out.data_ptr(), 1, C.DPC_MAX_D + 1, out.data_ptr(), None) == C.DPC_EINVAL
    with pytest.raises(HipError):
        C.call(lib.dpc_pack_query, x.data_ptr(), 4, 0, out.data_ptr(), None)
    torch.cuda.synchronize()


# ---- fit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ref.CONFIGS)
def test_fit_reproduces_the_reference(name):
    from deeprob.spn.structure.cltree import BinaryCLT
    g, m = ref.golden(name), fitted(name)
    assert m.root == int(g['ref_root'])                      # (drawn24: random_state.choice as the reference draws it)
    assert np.array_equal(m.tree, g['tree']) and np.array_equal(m.bfs, ref.restated(name)[0])
    assert m.params.dtype == np.float32 and np.max(np.abs(m.params - g['params'])) <= 1e-6
    d = int(g['n_vars'])
    on_device = BinaryCLT(list(range(d)), root=int(g['ref_root']))
    on_device.fit(torch.from_numpy(g['x']).cuda(), [[0, 1]] * d, alpha=float(g['alpha']))
    assert np.array_equal(on_device.tree, m.tree) and np.array_equal(on_device.params, m.params)


def test_fit_with_a_given_tree_keeps_it():
    from deeprob.spn.structure.cltree import BinaryCLT
    g = ref.golden('d16')
    chain = [-1] + list(range(15))
    m = BinaryCLT(list(range(16)), tree=chain)
    m.fit(g['x'], [[0, 1]] * 16, alpha=float(g['alpha']))
    assert m.tree.tolist() == chain and m.root == 0 and np.allclose(np.exp(m.params).sum(axis=2), 1.0)
    priors, joints = ref.priors_joints(ref.counts(g['x']), len(g['x']), float(g['alpha']))
    assert np.max(np.abs(m.params - ref.cpts(m.bfs, m.tree, priors, joints))) <= 1e-6


# ---- log likelihood ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ref.CONFIGS)
def test_log_likelihood_matches_the_reference(name):
    g, m = ref.golden(name), fitted(name)
    ll = m.log_likelihood(g['x'])
    assert isinstance(ll, np.ndarray) and ll.shape == (len(g['x']), 1) and ll.dtype == np.float32
    assert bar(ll, g['ll']) <= 1e-5
    ll_mar = m.log_likelihood(g['q'])
    assert bar(ll_mar, g['ll_mar']) <= 1e-5
    assert abs(float(ll_mar[0, 0])) <= 1e-5                  # the all-NaN row
    on_device = m.log_likelihood(torch.from_numpy(g['q']).cuda())
    assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and on_device.shape == (len(g['q']), 1)
    assert np.array_equal(on_device.cpu().numpy(), ll_mar)
    bfs, tree, params = ref.restated(name)
    assert bar(ll_mar, ref.log_likelihood(bfs, tree, params, g['q'])) <= 1e-5
    assert np.array_equal(m.likelihood(g['q']), np.exp(ll_mar))
    assert torch.equal(m.likelihood(torch.from_numpy(g['q']).cuda()), on_device.exp())


@pytest.mark.parametrize('b', [1, 63, 65])
def test_log_likelihood_does_not_depend_on_the_batch(b):
    g, m = ref.golden('d130'), fitted('d130')
    full = m.log_likelihood(g['q'])
    for start in (0, 2, 200):
        assert np.array_equal(m.log_likelihood(g['q'][start:start + b]), full[start:start + b])


def test_a_long_batch_in_pieces_gives_the_same_bytes(monkeypatch):
    from deeprob.hip import clt as C
    g, m = ref.golden('d16'), fitted('d16')
    q = np.concatenate([g['q'], g['q'], g['q'][:100]])
    whole = m.log_likelihood(q), m.mpe(q), m.sample(q, seed=3)
    monkeypatch.setattr(C, 'WORK_FLOATS', 0)
    assert C.query_rows(16) == 1024 < len(q)
    pieces = m.log_likelihood(q), m.mpe(q), m.sample(q, seed=3)
    for a, b in zip(whole, pieces):
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize('name', ref.CONFIGS)
def test_to_pc_evaluates_to_the_same_likelihoods(name):
    from deeprob.spn.algorithms.inference import log_likelihood
    g, m = ref.golden(name), fitted(name)
    pc = m.to_pc()
    for rows in (g['x'][:300], g['q']):
        assert bar(log_likelihood(pc, rows), m.log_likelihood(rows)) <= 1e-5


# ---- mpe -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ref.CONFIGS)
def test_mpe_is_no_less_likely_than_the_reference(name):
    g, m = ref.golden(name), fitted(name)
    q = g['q']
    got = m.mpe(q)
    obs = ~np.isnan(q)
    assert got.shape == q.shape and got.dtype == np.float32
    assert np.array_equal(got[obs], q[obs]) and set(np.unique(got)) <= {0.0, 1.0}
    mine = ref.log_likelihood64(m.tree, m.params, got)
    theirs = ref.log_likelihood64(m.tree, m.params, g['mpe_rows'])
    assert (mine >= theirs - 1e-5 * np.maximum(1.0, np.abs(theirs))).all()          # every row
    if name in ref.EXACT_MPE:
        assert np.array_equal(got, g['mpe_rows'])
    on_device = m.mpe(torch.from_numpy(q).cuda())
    assert on_device.is_cuda and np.array_equal(on_device.cpu().numpy(), got)


def test_mpe_is_optimal_by_enumeration():
    g, m = ref.golden('d10'), fitted('d10')
    q = g['q']
    best = ref.log_likelihood64(m.tree, m.params, m.mpe(q))
    every = np.array([[(v >> i) & 1 for i in range(10)] for v in range(1024)], np.float32)
    ll_every = ref.log_likelihood64(m.tree, m.params, every)
    for r, row in enumerate(q):
        obs = ~np.isnan(row)
        agrees = (every[:, obs] == row[obs]).all(axis=1)
        assert best[r] >= ll_every[agrees].max() - 1e-5


# ---- sample --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ref.CONFIGS)
def test_sample_replays(name):
    g, m = ref.golden(name), fitted(name)
    q = g['q']
    got = m.sample(q, seed=11)
    obs = ~np.isnan(q)
    assert got.shape == q.shape and np.array_equal(got[obs], q[obs]) and set(np.unique(got)) <= {0.0, 1.0}
    assert m.sample(q, seed=11).tobytes() == got.tobytes()
    assert m.sample(q, seed=12).tobytes() != got.tobytes()
    on_device = m.sample(torch.from_numpy(q).cuda(), seed=11)
    assert on_device.is_cuda and np.array_equal(on_device.cpu().numpy(), got)
    want, near = ref.sample_replay(m.bfs, m.tree, m.params, q, 11)
    assert near.mean() <= 0.02
    assert np.array_equal(got[~near], want[~near])


def test_sample_without_a_seed_draws_one():
    g, m = ref.golden('d10'), fitted('d10')
    np.random.seed(7)
    a = m.sample(g['q'])
    np.random.seed(7)
    b = m.sample(g['q'])
    c = m.sample(g['q'])
    assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_unconditional_samples_follow_the_model():
    """200 000 samples of the 10-variable model: the empirical joint of every tree edge within 4 binomial standard errors
    of the model's."""
    m = fitted('d10')
    n = 200000
    s = m.sample(torch.full((n, 10), float('nan'), device='cuda'), seed=2024).cpu().numpy().astype(np.int64)
    p = np.exp(m.params.astype(np.float64))
    marginal = np.zeros((10, 2))
    for j in m.bfs:
        pa = m.tree[j]
        marginal[j] = p[j, 0] if pa < 0 else marginal[pa] @ p[j]
    for j in m.bfs[1:]:
        pa = m.tree[j]
        for l in range(2):
            for k in range(2):
                model = marginal[pa, l] * p[j, l, k]
                seen = np.mean((s[:, pa] == l) & (s[:, j] == k))
                assert abs(seen - model) <= 4.0 * np.sqrt(model * (1.0 - model) / n), (j, pa, l, k, seen, model)


# ---- the buffer contract of the queries ------------------------------------------------------------------------------------
def test_queries_keep_the_buffer_contract():
    from deeprob.hip import clt as C
    g = ref.golden('d33')
    tree = device_tree('d33')
    x = torch.from_numpy(g['q']).cuda()
    plain = C.log_likelihood(tree, x), C.mpe(tree, x), C.sample(tree, x, 5)
    for pattern in PATTERNS:
        with contract(pattern) as c:
            c.frozen(x, tree._buf)
            got = (c.expect_written(C.log_likelihood(tree, x)), c.expect_written(C.mpe(tree, x)),
                   c.expect_written(C.sample(tree, x, 5)))
        for a, b in zip(got, plain):
            assert torch.equal(a, b)            # nothing depends on what outputs and scratch held
