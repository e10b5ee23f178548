"""BinaryCNet on the device: the learning kernels against integer and float64 numpy, ``fit`` against the reference's
goldens, ``log_likelihood`` against the goldens, the numpy restatement (tests/cnet_ref.py) and a brute-force marginal, and
every ``dpc_cnet_*`` entry point on poisoned, guard-banded memory (tests/buffer_contract.py): every call that reaches one
runs inside a contract context, under both poison patterns, and must give the same bytes under both.

Tolerances: counts, partitions and the OR tree are exact; OR weights within 1e-12 (Python floats on both sides); scores
within 1e-12 relative; log likelihoods at the project's bar |got - want| / max(1, |want|) <= 1e-5.  The leaves' trees: see
``cnet_ref.assert_leaf_trees``."""
import copy

import numpy as np
import pytest
import torch

from tests import clt_ref
from tests import cnet_ref as ref
from tests.buffer_contract import PATTERNS, contract

pytestmark = pytest.mark.gpu
NAMES = list(ref.CONFIGS)
_models = {}


def bar(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def guarded(fn, same=None):
    """``fn()`` under every poison pattern; the results (numpy arrays or device tensors, or tuples of them) must agree
    byte for byte.  Returns the first."""
    results = []
    for pattern in PATTERNS:
        with contract(pattern):
            results.append(fn())
    as_bytes = same or (lambda r: [np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t).tobytes()
                                   for t in (r if isinstance(r, tuple) else (r,))])
    assert as_bytes(results[0]) == as_bytes(results[1])
    return results[0]


def nodes_of(model):
    return model._nodes()


def fit_model(name, data=None, random_state=7):
    from deeprob.spn.structure.cnet import BinaryCNet
    g = ref.golden(name)
    m = BinaryCNet(list(range(int(g['n_vars']))))
    m.fit(g['x'] if data is None else data, random_state=random_state, **ref.hyper(g))
    return m


def model_bytes(m):
    out = []
    for node in nodes_of(m):
        out.append(repr((node.scope, node.or_id, node.weights)).encode())
        if node.clt is not None:
            out += [repr((node.clt.scope, node.clt.root)).encode(), node.clt.tree.tobytes(), node.clt.bfs.tobytes(),
                    node.clt.params.tobytes()]
    return out


def fitted(name):
    """The package's model of a fixture's training rows (numpy input, random_state=7), fitted under both poison patterns
    to the same bytes; once."""
    if name not in _models:
        _models[name] = guarded(lambda: fit_model(name), same=model_bytes)
    return _models[name]


def with_reference_trees(name):
    """A copy of the fitted model whose leaves hold the reference's undirected trees (rooted where the model's are) with
    parameters fitted by the package to the leaf's partition; once."""
    from deeprob.spn.structure.cltree import BinaryCLT
    key = (name, 'reference trees')
    if key not in _models:
        g, m = ref.golden(name), copy.deepcopy(fitted(name))
        edges, base = ref.golden_structure(g)[3], ref.restated(name)
        for k, node in enumerate(nodes_of(m)):
            if node.clt is not None:
                tree = ref.rooted(node.scope, edges[k], node.clt.root)
                node.clt = BinaryCLT(node.scope, tree=tree)
                node.clt.fit(g['x'][base[k]['rows']][:, node.scope], [[0, 1]] * len(node.scope), alpha=float(g['alpha']))
        _models[key] = m
    return _models[key]


def as_ref_model(m):
    """The package's model in the restatement's form (tests/cnet_ref.py)."""
    nodes = nodes_of(m)
    number = {id(n): k for k, n in enumerate(nodes)}
    out = []
    for n in nodes:
        if n.clt is None:
            out.append(dict(or_id=n.or_id, weights=list(n.weights), children=[number[id(c)] for c in n.children],
                            scope=list(n.scope)))
        else:
            out.append(dict(or_id=-1, weights=None, children=None, scope=list(n.scope), bfs=n.clt.bfs, tree=n.clt.tree,
                            params=n.clt.params))
    return out


def structure(m):
    nodes = nodes_of(m)
    or_id = np.array([-1 if n.clt is not None else n.or_id for n in nodes], np.int64)
    weights = np.array([[np.nan, np.nan] if n.clt is not None else n.weights for n in nodes], np.float64)
    scopes = [list(n.scope) if n.clt is not None else None for n in nodes]
    edges = [ref.edge_set(n.clt.scope, n.clt.tree) if n.clt is not None else None for n in nodes]
    return or_id, weights, scopes, edges


# ---- gather-pack and segmented counts ------------------------------------------------------------------------------------
def planes_of(x, sizes, rows):
    """[D, n_words] uint64 by the header's definition."""
    d = x.shape[1]
    words = [(n + 63) // 64 for n in sizes]
    bits = np.zeros((d, sum(words) * 64), np.uint64)
    at = w = 0
    for n, nw in zip(sizes, words):
        bits[:, w * 64:w * 64 + n] = x[rows[at:at + n]].T
        at, w = at + n, w + nw
    return (bits.reshape(d, -1, 64) << np.arange(64, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


@pytest.mark.parametrize('d', [2, 33, 130])
@pytest.mark.parametrize('sizes', [(0, 1, 63), (64, 0, 65), (257, 65, 0)])
def test_gather_pack_and_segmented_counts_are_exact(sizes, d):
    from deeprob.hip import cnet
    rs = np.random.RandomState(1000 * d + sum(sizes))
    x = (rs.rand(400, d) < 0.3).astype(np.float32)
    rows = rs.permutation(400)[:sum(sizes)].astype(np.int32)            # a shuffled row index
    xd, rows_d = torch.from_numpy(x).cuda(), torch.from_numpy(rows).cuda()
    xi = x.astype(np.int64)
    at, want = 0, []
    for n in sizes:
        part = xi[rows[at:at + n]]
        want.append(part.T @ part)
        at += n
    assert not want[sizes.index(0)].any()
    for pattern in PATTERNS:
        with contract(pattern) as c:
            c.frozen(xd, rows_d)
            gen = cnet.Generation(xd, rows_d, sizes)
            planes = c.expect_written(gen.pack())
            c.check()
            c.frozen(planes)
            ones = c.expect_written(gen.counts(0, 3))
            tail = c.expect_written(gen.counts(1, 2))                 # a chunk that does not start at task 0
        assert planes.shape == (d, sum((n + 63) // 64 for n in sizes)) and ones.dtype == torch.int32
        assert np.array_equal(planes.cpu().numpy().view(np.uint64), planes_of(x, sizes, rows))     # (pad bits zero included)
        assert np.array_equal(ones.cpu().numpy().astype(np.int64), np.stack(want))
        assert torch.equal(tail, ones[1:])


# ---- scores --------------------------------------------------------------------------------------------------------------
def test_scores_match_the_restatement_on_the_partitions_of_the_24_variable_fixture():
    """Every node of the restated model whose partition the learner scores (more rows than min_n_samples) is one task;
    its cut variables are inactive columns."""
    from deeprob.hip import cnet
    g = ref.golden('d24')
    alpha, d = float(g['alpha']), 24
    trace = []
    ref.learn(g['x'], random_state=np.random.RandomState(0), trace=trace, **ref.hyper(g))
    assert len(trace) >= 111
    rows = np.concatenate([r for r, _, _, _ in trace]).astype(np.int32)
    active = np.zeros((len(trace), d), np.uint8)
    for t, (_, scope, _, _) in enumerate(trace):
        active[t, scope] = 1
    xd, rows_d = torch.from_numpy(g['x']).cuda(), torch.from_numpy(rows).cuda()

    def run():
        gen = cnet.Generation(xd, rows_d, [len(r) for r, _, _, _ in trace])
        gen.pack()
        ones = gen.counts(0, len(trace))
        return gen.scores(ones, 0, active, alpha) + (ones,)
    gains, stats, best, ones = (t.cpu().numpy() for t in guarded(run))
    worst_gain = worst_entropy = 0.0
    for t, (r, scope, mean_entropy, want) in enumerate(trace):
        got = gains[t, scope]
        worst_gain = max(worst_gain, float(np.max(np.abs(got - want) / np.abs(want))))
        worst_entropy = max(worst_entropy, abs(stats[t, 0] - mean_entropy) / abs(mean_entropy))
        assert np.isneginf(np.delete(gains[t], scope)).all()
        assert best[t, 0] == scope[int(np.argmax(want))] and best[t, 1] == ones[t, best[t, 0], best[t, 0]]
        assert stats[t, 1] == got.max()
    print('scores: worst relative error of a gain %.3g, of a mean entropy %.3g' % (worst_gain, worst_entropy))
    assert worst_entropy <= 1e-12 and worst_gain <= 1e-12


# ---- partition -----------------------------------------------------------------------------------------------------------
def test_partition_is_stable_counts_and_tiles():
    from deeprob.hip import cnet
    rs = np.random.RandomState(3)
    d = 33
    x = (rs.rand(5000, d) < 0.4).astype(np.float32)
    x[:, 7] = 1.0                                   # constant columns: one child is empty
    x[:, 8] = 0.0
    sizes = [300, 0, 65, 4097, 64, 1, 129]
    cut = np.array([5, 3, 7, 32, -1, 8, 0])
    rows = rs.permutation(5000)[:sum(sizes)].astype(np.int32)
    xd, rows_d = torch.from_numpy(x).cuda(), torch.from_numpy(rows).cuda()
    for pattern in PATTERNS:
        with contract(pattern) as c:
            c.frozen(xd, rows_d)
            gen = cnet.Generation(xd, rows_d, sizes)
            c.frozen(gen.pack())
            rows_out, child_n = c.expect_written(*gen.partition(cut))
        rows_out, child_n = rows_out.cpu().numpy(), child_n.cpu().numpy()
        at, want, want_n = 0, [], []
        for n, col in zip(sizes, cut):
            seg = rows[at:at + n]
            at += n
            if col < 0:
                want_n.append([0, 0])
                continue
            bit = x[seg, col] == 1
            want += [seg[~bit], seg[bit]]                                # zeros first, each in its order
            want_n.append([int((~bit).sum()), int(bit.sum())])
        assert np.array_equal(child_n, want_n) and child_n[2].tolist() == [0, 65] and child_n[5].tolist() == [1, 0]
        assert rows_out.shape == (sum(sizes) - 64,) and np.array_equal(rows_out, np.concatenate(want))


# ---- fit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_fit_reproduces_the_reference(name):
    g, m = ref.golden(name), fitted(name)
    or_id, weights, scopes, edges = structure(m)
    want_or_id, want_weights, want_scopes, _, _ = ref.golden_structure(g)
    assert np.array_equal(or_id, want_or_id) and scopes == want_scopes
    inner = or_id >= 0
    assert np.max(np.abs(weights[inner] - want_weights[inner])) <= 1e-12
    ref.assert_leaf_trees(name, edges)
    base = ref.restated(name)
    assert np.array_equal(weights[inner], ref.structure(base)[1][inner])        # the same Python-float expression
    assert m.scope == list(range(int(g['n_vars']))) and m.children[0] is nodes_of(m)[1] and m.or_id == or_id[0]
    assert m.params_count() == sum(2 if n.clt is None else n.clt.params_count() for n in nodes_of(m))
    assert m.fit_profile_['generations'] == max(len(n.scope) for n in nodes_of(m)) - min(len(n.scope) for n in nodes_of(m)) + 1


def test_fit_is_reproducible_and_takes_device_tensors():
    g = ref.golden('d33')
    first = model_bytes(fitted('d33'))
    again = guarded(lambda: fit_model('d33'), same=model_bytes)
    on_device = guarded(lambda: fit_model('d33', torch.from_numpy(g['x']).cuda()), same=model_bytes)
    assert model_bytes(again) == first and model_bytes(on_device) == first
    assert model_bytes(guarded(lambda: fit_model('d33', random_state=8), same=model_bytes)) != first        # other roots
    roots = np.random.RandomState(7)
    for node in nodes_of(fitted('d33')):
        if node.clt is not None:
            assert node.clt.root == int(roots.choice(len(node.scope)))        # drawn breadth first, left before right


def test_fit_in_chunks_of_one_task_gives_the_same_model(monkeypatch):
    from deeprob.hip import cnet
    first = model_bytes(fitted('d24'))
    monkeypatch.setattr(cnet, 'COUNT_INTS', 0)
    assert cnet.chunk_tasks(24) == 1
    assert model_bytes(guarded(lambda: fit_model('d24'), same=model_bytes)) == first


@pytest.mark.parametrize('name', NAMES)
def test_every_leaf_is_the_binary_clt_of_its_partition(name):
    from deeprob.spn.structure.cltree import BinaryCLT
    g, m, base = ref.golden(name), fitted(name), ref.restated(name)
    for k, node in enumerate(nodes_of(m)):
        if node.clt is None:
            continue
        scope = node.scope
        assert isinstance(node.clt, BinaryCLT) and node.clt.scope == scope
        own = BinaryCLT(scope, root=scope[node.clt.root])
        own.fit(g['x'][base[k]['rows']][:, scope], [[0, 1]] * len(scope), alpha=float(g['alpha']))
        assert np.array_equal(own.tree, node.clt.tree) and np.array_equal(own.bfs, node.clt.bfs)
        assert own.params.tobytes() == node.clt.params.tobytes()


# ---- log likelihood, complete rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_log_likelihood_matches_the_reference(name):
    g, m = ref.golden(name), with_reference_trees(name)
    ll = guarded(lambda: m.log_likelihood(g['x']))
    assert isinstance(ll, np.ndarray) and ll.shape == (len(g['x']),) and ll.dtype == np.float32
    assert bar(ll, g['ll_train']) <= 1e-5
    fresh = guarded(lambda: m.log_likelihood(g['fresh']))
    assert bar(fresh, g['ll_fresh']) <= 1e-5
    assert bar(fresh, ref.log_likelihood(ref.restated(name, reference_trees=True), g['fresh'])) <= 1e-5


@pytest.mark.parametrize('name', NAMES)
def test_log_likelihood_matches_the_restatement(name):
    g, m = ref.golden(name), fitted(name)
    ll = guarded(lambda: m.log_likelihood(g['fresh']))
    assert bar(ll, ref.log_likelihood(as_ref_model(m), g['fresh'])) <= 1e-5
    on_device = guarded(lambda: m.log_likelihood(torch.from_numpy(g['fresh']).cuda()))
    assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and on_device.shape == (ref.N_FRESH,)
    assert np.array_equal(on_device.cpu().numpy(), ll)
    assert np.array_equal(m.likelihood(g['fresh'][:50]), np.exp(ll[:50]))
    assert torch.equal(m.likelihood(torch.from_numpy(g['fresh']).cuda()), on_device.exp())


@pytest.mark.parametrize('b', [1, 63, 65])
def test_log_likelihood_does_not_depend_on_the_batch(b):
    g, m = ref.golden('d130'), fitted('d130')
    q = np.concatenate([g['fresh'][:256], ref.queries('d130')])
    full = guarded(lambda: m.log_likelihood(q))
    for start in (0, 2, 200, 300):
        assert np.array_equal(guarded(lambda: m.log_likelihood(q[start:start + b])), full[start:start + b])


def test_a_long_batch_in_pieces_gives_the_same_bytes(monkeypatch):
    from deeprob.hip import cnet
    g, m = ref.golden('d33'), fitted('d33')
    q = np.concatenate([g['x'], ref.queries('d33')])
    whole = guarded(lambda: m.log_likelihood(q))
    monkeypatch.setattr(cnet, 'WORK_BYTES', 0)
    assert cnet.query_rows(100) == 1024 < len(q)
    assert np.array_equal(guarded(lambda: m.log_likelihood(q)), whole)


# ---- log likelihood, rows with NaN ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_marginal_log_likelihood_matches_the_restatement(name):
    m = fitted(name)
    q = ref.queries(name)
    assert np.isnan(q[0]).all() and not np.isnan(q[1]).any() and 0.3 < np.isnan(q).mean() < 0.5
    ll = guarded(lambda: m.log_likelihood(q))
    assert ll.shape == (len(q),) and ll.dtype == np.float32
    assert bar(ll, ref.log_likelihood(as_ref_model(m), q)) <= 1e-5
    assert abs(float(ll[0])) <= 1e-5                         # the all-NaN row


def test_marginal_log_likelihood_is_the_sum_over_completions():
    m = fitted('d10')
    q = ref.queries('d10')
    ll = guarded(lambda: m.log_likelihood(q))
    assert bar(ll, ref.brute_marginal(as_ref_model(m), q)) <= 1e-5


@pytest.mark.parametrize('name', ['d33', 'd24'])
def test_nan_outside_the_cut_variables_agrees_with_the_path_formula(name):
    """log P = the log weights along the row's path + the leaf tree's marginal of the leaf's observed entries."""
    g, m = ref.golden(name), fitted(name)
    model = as_ref_model(m)
    q = g['fresh'][:200].copy()
    leaf = ref.leaf_of_rows(model, q)
    rs = np.random.RandomState(9)
    want = np.empty(len(q))
    parent = {c: (k, v) for k, n in enumerate(model) if n['or_id'] >= 0 for v, c in enumerate(n['children'])}
    for r in range(len(q)):
        node = model[leaf[r]]
        hide = [v for v in node['scope'] if rs.rand() < 0.5] or node['scope'][:1]
        q[r, hide] = np.nan
        s, k = 0.0, int(leaf[r])
        while k in parent:
            k, v = parent[k]
            s += float(np.log(np.float64(model[k]['weights'][v])))
        want[r] = s + float(clt_ref.log_likelihood(node['bfs'], node['tree'], node['params'], q[r:r + 1, node['scope']])[0])
    assert np.isnan(q).any(axis=1).all()
    assert bar(guarded(lambda: m.log_likelihood(q)), want) <= 1e-5


# ---- errors --------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_what_the_header_excludes():
    from deeprob.hip import clt as C
    lib = C.load_library()
    buf = torch.zeros(64, dtype=torch.int64, device='cuda')
    p = buf.data_ptr()
    assert lib.dpc_cnet_gather_pack(p, 4, C.DPC_MAX_D + 1, p, p, p, 1, 1, p, None) == C.DPC_EINVAL and lib.dpc_last_error()
    assert lib.dpc_cnet_gather_pack(p, 4, 4, None, p, p, 1, 1, p, None) == C.DPC_EINVAL
    assert lib.dpc_cnet_pair_counts(p, 1, 4, p, 65536, p, None) == C.DPC_EINVAL
    assert lib.dpc_cnet_scores(p, p, p, 1, 4, -1.0, p, p, p, None) == C.DPC_EINVAL
    assert lib.dpc_cnet_partition(p, 1, p, p, p, p, p, 0, p, p, None) == C.DPC_EINVAL
    assert lib.dpc_cnet_log_likelihood(p, 4, 4, 1, p, p, p, p, p, p, 6, 1, p, p, None) == C.DPC_EINVAL       # levels > d + 1
    assert lib.dpc_cnet_log_likelihood(p, 4, 4, 1, p, p, p, p, p, p, 1, 1, p + 4, p, None) == C.DPC_EINVAL   # work alignment
    torch.cuda.synchronize()


def test_missing_library_and_cpu_tensor_raise_hip_error(monkeypatch):
    import os
    from deeprob.hip import HipError, clt
    from deeprob.spn.structure.cnet import BinaryCNet
    g, m = ref.golden('d5'), fitted('d5')
    with pytest.raises(HipError):
        BinaryCNet(list(range(5))).fit(torch.from_numpy(g['x']))
    for query in (m.log_likelihood, m.likelihood):
        with pytest.raises(HipError) as e:
            query(torch.from_numpy(g['fresh']))
        assert 'make -C deeprob-kit_amd/csrc' in str(e.value)
    monkeypatch.setattr(clt, '_lib', None)
    monkeypatch.setattr(clt, 'LIB_PATH', os.path.join(os.path.dirname(clt.LIB_PATH), 'no', 'such', 'libdeeprob_clt.so'))
    for call in (lambda: m.log_likelihood(g['fresh']), lambda: BinaryCNet(list(range(5))).fit(g['x'])):
        with pytest.raises(HipError) as e:
            call()
        assert 'make -C deeprob-kit_amd/csrc' in str(e.value)
