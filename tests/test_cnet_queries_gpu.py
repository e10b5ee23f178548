"""Sampling and MPE of cutset networks on the device (``dpc_cnq_sample`` / ``dpc_cnq_mpe``, ``deeprob.hip.cnet.sample`` / ``mpe``,
``BinaryCNet.sample``) against the numpy restatement (tests/cnet_queries_ref.py) and against enumeration, on poisoned,
guard-banded memory (tests/buffer_contract.py).

Tolerances.  The sampler is replayed draw by draw: rows in which a draw lies within 1e-5 of its probability (``near``; at
most 2 % of the rows) may fall either way and are left out, every other row is equal in every entry and in its leaf.
Frequencies lie within 4 binomial standard errors of the exact posterior.  MPE is compared by the likelihood of the
completion (``cnet_ref._path_values``, float64) at the project's bar 1e-5 * max(1, |want|): two completions that tie to
float32 rounding are both right."""
import numpy as np
import pytest
import torch

from tests import cnet_queries_ref as qref
from tests import cnet_ref as ref
from tests.buffer_contract import PATTERNS, contract
from tests.test_cnet_gpu import fitted, guarded

PATTERNS_D5, N_DRAWS = qref.PATTERNS_D5, qref.N_DRAWS

pytestmark = pytest.mark.gpu
NAMES = list(ref.CONFIGS)
_cache = {}


def as_ref_model(m):
    """The package's model as tests/cnet_ref.py holds one."""
    nodes = m._nodes()
    number = {id(n): k for k, n in enumerate(nodes)}
    return [dict(or_id=n.or_id, weights=[float(w) for w in n.weights], children=[number[id(c)] for c in n.children],
                 scope=list(n.scope))
            if n.clt is None else
            dict(or_id=-1, weights=None, children=None, scope=list(n.scope), bfs=n.clt.bfs, tree=n.clt.tree, params=n.clt.params)
            for n in nodes]


def pair(name):
    """``(the fitted model, the same as the restatement holds it)``; once per fixture."""
    if name not in _cache:
        _cache[name] = (fitted(name), as_ref_model(fitted(name)))
    return _cache[name]


def tables(m):
    return m._on_device(torch.device('cuda', torch.cuda.current_device()))


def device(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def run(m, x, seed=None):
    """``(out, choice)`` as numpy from the binding, under both poison patterns, x and the model's buffer frozen, every
    element of both outputs written."""
    from deeprob.hip import cnet
    xd, t = device(x), tables(m)
    results = []
    for pattern in PATTERNS:
        with contract(pattern) as c:
            c.frozen(xd, t._buf)
            if seed is None:
                out, choice = cnet.mpe(t, xd, return_choice=True)
            else:
                out, choice = cnet.sample(t, xd, seed, return_choice=True)
            c.expect_written(out, choice)
        results.append((out.cpu().numpy(), choice.cpu().numpy()))
    assert results[0][0].tobytes() == results[1][0].tobytes() and results[0][1].tobytes() == results[1][1].tobytes()
    assert results[0][0].shape == x.shape and results[0][0].dtype == np.float32 and results[0][1].dtype == np.int32
    return results[0]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def bar(got, want):
    return (want - got) / np.maximum(1.0, np.abs(want))


# ---- the sampler, replayed ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_sampler_replays_the_restatement(name):
    m, model = pair(name)
    q = ref.queries(name)
    obs = ~np.isnan(q)
    out, choice = run(m, q, 11)
    assert same_bits(out[obs], q[obs]) and set(np.unique(out)) <= {0.0, 1.0}
    again, again_choice = run(m, q, 11)
    assert out.tobytes() == again.tobytes() and choice.tobytes() == again_choice.tobytes()
    assert run(m, q, 12)[0].tobytes() != out.tobytes()
    public = guarded(lambda: m.sample(q, seed=11))
    assert isinstance(public, np.ndarray) and public.tobytes() == out.tobytes()
    on_device = guarded(lambda: m.sample(device(q), seed=11))
    assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and on_device.cpu().numpy().tobytes() == out.tobytes()
    want, leaf, near = qref.sample_replay(model, q, 11)
    print('%s: near %.4f' % (name, near.mean()))
    assert near.mean() <= 0.02
    assert np.array_equal(out[~near], want[~near]) and np.array_equal(choice[~near], leaf[~near])
    is_leaf = np.array([node['or_id'] < 0 for node in model])
    assert is_leaf[choice].all() and np.array_equal(choice, ref.leaf_of_rows(model, out))
    complete = obs.all(axis=1)
    assert complete[1] and np.array_equal(choice[complete], ref.leaf_of_rows(model, q[complete]))


def test_unseeded_sampling_draws_its_seed_from_numpy():
    m, _ = pair('d10')
    q = np.full((64, 10), np.nan, np.float32)
    np.random.seed(3)
    first = m.sample(q)
    np.random.seed(3)
    assert m.sample(q).tobytes() == first.tobytes() and set(np.unique(first)) <= {0.0, 1.0}
    assert m.sample(q).tobytes() != first.tobytes()


# ---- the sampler, its distribution -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pattern', range(3))
def test_sampler_draws_from_the_posterior_by_enumeration(pattern):
    m, model = pair('d5')
    row = np.asarray(PATTERNS_D5[pattern], np.float32)
    x = np.tile(row, (N_DRAWS, 1))
    out, choice = run(m, x, 2024)
    obs = ~np.isnan(row)
    assert same_bits(out[:, obs], x[:, obs]) and set(np.unique(out)) <= {0.0, 1.0}
    worst, outside = qref.deviations(model, row, out)
    print('pattern %d: worst deviation %.2f s.e., mass outside the support %g' % (pattern, worst, outside))
    assert outside == 0.0 and worst <= 4.0


def test_leaf_frequencies_match_the_posterior_over_leaves():
    m, model = pair('d10')
    cuts = [node['or_id'] for node in model if node['or_id'] >= 0]
    row = ref.golden('d10')['fresh'][3].copy()
    row[[model[0]['or_id'], model[1]['or_id'], model[2]['or_id']]] = np.nan          # the root's cut and both below it
    row[[c for c in range(10) if c not in cuts][:1]] = np.nan                        # and a column only leaves hold
    assert np.isnan(row[list(set(cuts))]).sum() >= 2 and not np.isnan(row).all()
    x = np.tile(row, (N_DRAWS, 1))
    out, choice = run(m, x, 2024)
    groups = ref.leaf_of_rows(model, qref.every_row(10))
    worst, outside = qref.deviations(model, row, choice, groups)
    reached = len(np.unique(choice))
    print('leaf frequencies on d10: %d leaves drawn, worst deviation %.2f s.e.' % (reached, worst))
    assert reached >= 3 and outside == 0.0 and worst <= 4.0


# ---- MPE ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_mpe_is_no_less_likely_than_the_restatement_and_optimal_by_enumeration(name):
    m, model = pair(name)
    q = ref.queries(name)
    obs = ~np.isnan(q)
    out, choice = run(m, q)
    assert same_bits(out[obs], q[obs]) and set(np.unique(out)) <= {0.0, 1.0}
    is_leaf = np.array([node['or_id'] < 0 for node in model])
    assert is_leaf[choice].all() and np.array_equal(choice, ref.leaf_of_rows(model, out))
    got = ref._path_values(model, out.astype(np.int64))
    want = ref._path_values(model, qref.mpe(model, q)[0].astype(np.int64))
    print('%s: largest shortfall against the restatement %.3g' % (name, float(np.max(bar(got, want)))))
    assert (bar(got, want) <= 1e-5).all()
    d = q.shape[1]
    if d <= 10:
        every = qref.every_row(d)
        ll_every = ref._path_values(model, every)
        best = np.array([ll_every[(every[:, obs[r]] == q[r, obs[r]]).all(axis=1)].max() for r in range(len(q))])
        print('%s: largest shortfall against enumeration %.3g' % (name, float(np.max(bar(got, best)))))
        assert (bar(got, best) <= 1e-5).all()


# ---- the batch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b', [1, 63, 65])
def test_rows_do_not_depend_on_the_batch(b):
    m, _ = pair('d33')
    q = ref.queries('d33')
    full, full_choice = run(m, q, 11)
    part, part_choice = run(m, q[:b], 11)
    assert part.tobytes() == full[:b].tobytes() and part_choice.tobytes() == full_choice[:b].tobytes()
    full, full_choice = run(m, q)
    part, part_choice = run(m, q[:b])
    assert part.tobytes() == full[:b].tobytes() and part_choice.tobytes() == full_choice[:b].tobytes()


def test_a_long_batch_in_pieces_gives_the_same_bytes(monkeypatch):
    from deeprob.hip import cnet
    m, _ = pair('d24')
    q = np.concatenate([ref.queries('d24', n=512, seed=s) for s in (5, 6, 7, 8)] + [ref.queries('d24', n=52, seed=9)])
    assert len(q) == 2100
    whole = run(m, q, 11), run(m, q)
    monkeypatch.setattr(cnet, 'WORK_BYTES', 0)
    assert cnet.query_rows(tables(m).query_row_bytes) == 1024 < len(q)
    pieces = run(m, q, 11), run(m, q)
    for a, b in zip(whole, pieces):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- the smallest shapes -----------------------------------------------------------------------------------------------------
def test_a_lone_leaf_and_a_one_variable_leaf():
    from deeprob.hip import cnet
    dev = torch.device('cuda', torch.cuda.current_device())
    # M = 1: a Chow-Liu tree over two columns, no OR draw; column 1 follows column 0 with probability 0.9
    params = np.log(np.array([[[0.3, 0.7], [0.3, 0.7]], [[0.9, 0.1], [0.1, 0.9]]], np.float32))
    lone = cnet.DeviceCNet(2, [-1], [[0, -1]], [[0.0, 0.0]], [([0, 1], [0, 1], [-1, 0], params)], dev)
    assert (lone.n_nodes, lone.levels) == (1, 1)
    model = [dict(or_id=-1, weights=None, children=None, scope=[0, 1], bfs=np.array([0, 1]), tree=np.array([-1, 0]), params=params)]
    x = np.tile(np.array([[np.nan, np.nan], [np.nan, 1.0], [0.0, np.nan], [1.0, 0.0]], np.float32), (2000, 1))
    out, choice = cnet.sample(lone, device(x), 7, return_choice=True)
    out, choice = out.cpu().numpy(), choice.cpu().numpy()
    want, _, near = qref.sample_replay(model, x, 7)
    assert near.mean() <= 0.02 and np.array_equal(out[~near], want[~near]) and not choice.any()
    for k in range(3):
        worst, outside = qref.deviations(model, x[k], out[k::4])
        assert outside == 0.0 and worst <= 4.0, k
    best, choice = cnet.mpe(lone, device(x[:4]), return_choice=True)
    assert best.cpu().numpy().tolist() == [[1.0, 1.0], [1.0, 1.0], [0.0, 0.0], [1.0, 0.0]] and not choice.cpu().numpy().any()
    # one-variable leaves under one cut; column 2 is in no scope: returned as given
    half = np.full((1, 2, 2), np.log(0.5), np.float32)
    skew = np.log(np.array([[[0.2, 0.8], [0.2, 0.8]]], np.float32))
    net = cnet.DeviceCNet(3, [0, -1, -1], [[1, 2], [0, -1], [1, -1]], np.log([[0.4, 0.6], [0.5, 0.5], [0.5, 0.5]]),
                          [([1], [0], [-1], half), ([1], [0], [-1], skew)], dev)
    x = np.tile(np.array([[np.nan, np.nan, np.nan], [np.nan, 0.0, 5.0]], np.float32), (4000, 1))
    out, choice = cnet.sample(net, device(x), 9, return_choice=True)
    out, choice = out.cpu().numpy(), choice.cpu().numpy()
    assert np.isnan(out[0::2, 2]).all() and (out[1::2, 2] == 5.0).all() and (out[1::2, 1] == 0.0).all()
    assert np.array_equal(choice, 1 + out[:, 0].astype(np.int32)) and set(np.unique(out[:, :2])) <= {0.0, 1.0}
    for draws, p in ((out[0::2, 0], 0.6), (out[0::2, 1][out[0::2, 0] == 1], 0.8),
                     (out[1::2, 0], 0.6 * 0.2 / (0.6 * 0.2 + 0.4 * 0.5))):
        assert abs(draws.mean() - p) <= 4.0 * np.sqrt(p * (1 - p) / len(draws)), (draws.mean(), p, len(draws))
    best = cnet.mpe(net, device(x[:2])).cpu().numpy()
    assert best[0, :2].tolist() == [1.0, 1.0] and np.isnan(best[0, 2]) and best[1].tolist() == [0.0, 0.0, 5.0]


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_what_the_header_excludes():
    from deeprob.hip import clt as C
    lib = C.load_library()
    buf = torch.zeros(64, dtype=torch.int64, device='cuda')
    p = buf.data_ptr()

    def args(x=p, codes=p, b=4, d=4, n_nodes=1, parent=p, levels=1, max_leaf_d=1, work=p, out=p, row0=0):
        head = (x, codes, b, d, n_nodes, p, p, parent, p, p, p, p, levels, max_leaf_d)
        return head + (work, out, None, None), head + (1, row0, work, out, None, None)

    cases = [dict(d=0), dict(d=C.DPC_MAX_D + 1), dict(levels=6), dict(levels=0), dict(max_leaf_d=5), dict(max_leaf_d=0),
             dict(work=p + 4), dict(x=None), dict(codes=None), dict(parent=None), dict(work=None), dict(out=None), dict(b=-1)]
    for case in cases:
        for fn, a in zip((lib.dpc_cnq_mpe, lib.dpc_cnq_sample), args(**case)):
            assert fn(*a) == C.DPC_EINVAL and fn.__name__.encode() in lib.dpc_last_error(), case
    assert lib.dpc_cnq_sample(*args(row0=-1)[1]) == C.DPC_EINVAL and b'row0' in lib.dpc_last_error()
    before = buf.clone()
    for fn, a in zip((lib.dpc_cnq_mpe, lib.dpc_cnq_sample), args(b=0)):
        assert fn(*a) == C.DPC_OK
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
