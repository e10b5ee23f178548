"""The scored cutset learners on the device: ``dpc_cut_pair_counts`` against integer numpy on poisoned, guard-banded
memory (tests/buffer_contract.py), the reference's helpers and both learners against the reference's goldens
(tools/gen_golden_cnet_scored.py) and against the numpy restatement (tests/cnet_scored_ref.py).

Tolerances.  Counts, index sets, the OR tree and row counts are exact; OR weights within 1e-12 of the reference's (the
same Python-float expression); a helper's score within 4 x the deviation the generator measured between the reference and
float64 (``helper_deviation``); scores against the restatement within 1e-12 relative (float64 sums of the same terms from
the same integers, ``math.fsum`` on both sides); tables within 1e-6; log likelihoods at the project's bar
|got - want| / max(1, |want|) <= 1e-5.  The leaves' trees follow the rule of ``cnet_ref.assert_leaf_trees``: the
reference's edge set where it is the only maximum spanning tree, a tree of the same sorted edge weights (2^-23) elsewhere."""
import copy

import numpy as np
import pytest
import torch

from tests import cnet_ref
from tests import cnet_scored_ref as ref
from tests.buffer_contract import PATTERNS, contract

pytestmark = pytest.mark.gpu
NAMES = list(ref.CONFIGS)
_models = {}


def bar(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def rel(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape
    return float(np.max(np.abs(got - want) / np.abs(want))) if len(want) else 0.0


def learn(name, data=None, random_state=7, n_cand_cuts=None):
    from deeprob.spn.learning import learn_cnet_bd, learn_cnet_bic
    _, kind, par, k = ref.CONFIGS[name]
    data = ref.golden(name)['x'] if data is None else data
    k = k if n_cand_cuts is None else n_cand_cuts
    if kind == 'bd':
        return learn_cnet_bd(data, ess=par, n_cand_cuts=k, random_state=random_state)
    return learn_cnet_bic(data, alpha=par, n_cand_cuts=k, random_state=random_state)


def model_bytes(m):
    out = []
    for node in m._nodes():
        out.append(repr((node.scope, node.or_id, node.weights, node.n_rows_, node.score_, node.candidates_)).encode())
        if node.clt is not None:
            out += [repr((node.clt.scope, node.clt.root)).encode(), node.clt.tree.tobytes(), node.clt.bfs.tobytes(),
                    node.clt.params.tobytes()]
    return out


def guarded(fn, same=None):
    """``fn()`` under every poison pattern; the results must agree byte for byte.  Returns the first."""
    results = []
    for pattern in PATTERNS:
        with contract(pattern):
            results.append(fn())
    as_bytes = same or (lambda r: [np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t).tobytes()
                                   for t in (r if isinstance(r, tuple) else (r,))])
    assert as_bytes(results[0]) == as_bytes(results[1])
    return results[0]


def fitted(name):
    """The package's model of a fixture (numpy input, random_state=7), learned under both poison patterns to the same
    bytes; once."""
    if name not in _models:
        _models[name] = guarded(lambda: learn(name), same=model_bytes)
    return _models[name]


def leaf_alpha(name, depth):
    _, kind, par, _ = ref.CONFIGS[name]
    return par / 2.0 ** depth / 4 if kind == 'bd' else par


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [1, 2, 31, 32, 33, 65])
def test_cut_pair_counts_are_exact(d):
    """One launch: tasks of 1, 63, 0, 64, 65 and 2049 rows (one word past a full step of 32 words), several entries per
    task with the tasks interleaved, a cut column that is constant 0 and one that is constant 1; every cut column is also
    a row i and a column j of its output."""
    from deeprob.hip import cnet
    sizes = [1, 63, 0, 64, 65, 2049]
    rs = np.random.RandomState(100 + d)
    x = (rs.rand(2400, d) < 0.4).astype(np.float32)
    cut_cols = [0]
    if d >= 2:
        x[:, d - 1] = 1.0
        cut_cols.append(d - 1)
    if d >= 3:
        x[:, d - 2] = 0.0
        cut_cols += [d - 2, d // 2]
    rows = rs.permutation(2400)[:sum(sizes)].astype(np.int32)
    entries = [(t, c) for c in cut_cols for t in range(len(sizes))] + [(5, 0), (1, cut_cols[-1])]
    xi = x.astype(np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    want = []
    for t, c in entries:
        part = xi[rows[off[t]:off[t + 1]]]
        part = part[part[:, c] == 1]
        want.append(part.T @ part)
    want = np.stack(want)
    assert not want[[e for e, (t, _) in enumerate(entries) if t == 2]].any()
    if d >= 3:
        assert not want[[e for e, (_, c) in enumerate(entries) if c == d - 2]].any()      # the empty side
    xd, rows_d = torch.from_numpy(x).cuda(), torch.from_numpy(rows).cuda()
    for pattern in PATTERNS:
        with contract(pattern) as c:
            c.frozen(xd, rows_d)
            gen = cnet.Generation(xd, rows_d, sizes)
            planes = gen.pack()
            ones = gen.counts(0, len(sizes))
            c.check()
            c.frozen(planes, gen._word, gen._seg)
            ones1 = c.expect_written(gen.cut_counts([t for t, _ in entries], [col for _, col in entries]))
        assert ones1.dtype == torch.int32 and ones1.shape == (len(entries), d, d)
        got = ones1.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, want) and np.array_equal(got, got.transpose(0, 2, 1))
        # the other side is the task's counts minus these; a cut on a constant-1 column leaves it empty
        full = ones.cpu().numpy().astype(np.int64)
        for e, (t, col) in enumerate(entries):
            part = xi[rows[off[t]:off[t + 1]]]
            part = part[part[:, col] == 0]
            assert np.array_equal(full[t] - got[e], part.T @ part)


def test_cut_pair_counts_rejects_what_the_header_excludes():
    from deeprob.hip import clt as C
    lib = C.load_library()
    buf = torch.zeros(64, dtype=torch.int64, device='cuda')
    p = buf.data_ptr()
    assert lib.dpc_cut_pair_counts(p, 1, C.DPC_MAX_D + 1, p, 1, p, p, 1, p, None) == C.DPC_EINVAL and lib.dpc_last_error()
    assert lib.dpc_cut_pair_counts(p, 1, 4, p, 1, p, p, 65536, p, None) == C.DPC_EINVAL
    assert lib.dpc_cut_pair_counts(p, 1, 4, p, 1, p, p, 0, p, None) == C.DPC_EINVAL
    assert lib.dpc_cut_pair_counts(p, 1, 4, p, 0, p, p, 1, p, None) == C.DPC_EINVAL
    assert lib.dpc_cut_pair_counts(p, 1, 4, p, 1, None, p, 1, p, None) == C.DPC_EINVAL
    assert lib.dpc_cut_pair_counts(p, -1, 4, p, 1, p, p, 1, p, None) == C.DPC_EINVAL
    torch.cuda.synchronize()


# ---- 2. the reference's helpers --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_helpers_match_the_reference(name):
    from deeprob.spn.learning import cnet_bayesian as cb
    g = ref.golden(name)
    _, kind, par, k = ref.CONFIGS[name]
    x, d = g['x'], int(g['n_vars'])
    smoothing = par if kind == 'bd' else 4 * par
    bound = 4 * float(g['helper_deviation'])
    cands = guarded(lambda: cb.select_cand_cuts(x, ess=smoothing, n_cand_cuts=k))
    assert sorted(cands.tolist()) == g['helper_cands'].tolist()
    assert cands.tolist() == ref.candidates(x, smoothing / 4, min(k, d))[0]              # and in the order §17 defines
    got_or = guarded(lambda: cb.compute_or_bd_scores(x, ess=smoothing))
    got_clt = guarded(lambda: cb.compute_clt_bd_scores(torch.from_numpy(x).cuda(), ess=smoothing))
    pairs = ~np.eye(d, dtype=bool)
    print(name, 'helpers: or scores', rel(got_or, g['helper_or_scores']), 'pairwise', rel(got_clt[pairs], g['helper_clt_scores'][pairs]),
          'bound', bound)
    assert got_or.dtype == np.float64 and got_or.shape == (d,) and got_clt.shape == (d, d)
    assert rel(got_or, g['helper_or_scores']) <= bound and rel(got_clt[pairs], g['helper_clt_scores'][pairs]) <= bound
    assert rel(got_or, ref.or_bd_scores(x, smoothing)) <= 1e-12 and rel(got_clt, ref.clt_bd_scores(x, smoothing)) <= 1e-12
    tree = ref.restated(name)[0]['tree0']
    assert abs(cb.eval_tree_score(tree, got_clt, got_or) - ref.tree_score(tree, got_clt, got_or)) <= 1e-9


# ---- 3. both learners against the reference --------------------------------------------------------------------------------
def structure(m):
    nodes = m._nodes()
    or_id = np.array([-1 if n.clt is not None else n.or_id for n in nodes], np.int64)
    weights = np.array([[np.nan, np.nan] if n.clt is not None else n.weights for n in nodes], np.float64)
    scopes = [list(n.scope) if n.clt is not None else None for n in nodes]
    edges = [cnet_ref.edge_set(n.clt.scope, n.clt.tree) if n.clt is not None else None for n in nodes]
    return or_id, weights, scopes, edges, np.array([n.n_rows_ for n in nodes], np.int64)


def with_reference_trees(name):
    """A copy of the learned model whose leaves hold the reference's undirected trees (rooted where the model's are)
    with tables fitted by the package to the leaf's rows at the leaf's smoothing; once."""
    from deeprob.spn.structure.cltree import BinaryCLT
    key = (name, 'reference trees')
    if key not in _models:
        g, m = ref.golden(name), copy.deepcopy(fitted(name))
        edges, base = cnet_ref.golden_structure(g)[3], ref.restated(name)
        for k, node in enumerate(m._nodes()):
            if node.clt is not None and cnet_ref.edge_set(node.clt.scope, node.clt.tree) != edges[k]:
                tree = cnet_ref.rooted(node.scope, edges[k], node.clt.root)
                node.clt = BinaryCLT(node.scope, tree=tree)
                node.clt.fit(g['x'][base[k]['rows']][:, node.scope], [[0, 1]] * len(node.scope),
                             alpha=leaf_alpha(name, base[k]['depth']))
        _models[key] = m
    return _models[key]


@pytest.mark.parametrize('name', NAMES)
def test_learners_reproduce_the_reference(name):
    from deeprob.spn.structure.cnet import BinaryCNet
    g, m = ref.golden(name), fitted(name)
    _, kind, par, _ = ref.CONFIGS[name]
    assert isinstance(m, BinaryCNet) and m.scope == list(range(int(g['n_vars'])))
    or_id, weights, scopes, edges, rows = structure(m)
    want_or_id, want_weights, want_scopes, want_edges, want_rows = cnet_ref.golden_structure(g)
    assert np.array_equal(or_id, want_or_id) and scopes == want_scopes and np.array_equal(rows, want_rows)
    inner = or_id >= 0
    if inner.any():
        assert np.max(np.abs(weights[inner] - want_weights[inner])) <= 1e-12
    base = ref.restated(name)
    for k, (got, want) in enumerate(zip(edges, want_edges)):
        if want is None:
            assert got is None, k
        elif g['leaf_unique'][k]:
            assert got == want, k
        else:
            mi = cnet_ref.leaf_mutual_information(g['x'], base[k], ref.BD_TREE_ALPHA if kind == 'bd' else par)
            a, b = cnet_ref.edge_weights(mi, scopes[k], got), cnet_ref.edge_weights(mi, scopes[k], want)
            assert a.shape == b.shape and (len(a) == 0 or np.max(np.abs(a - b)) <= 2.0 ** -23), k
    bound = 4 * float(g['score_deviation'])
    nodes = m._nodes()
    assert rel([n.score_ for n in nodes], g['node_score']) <= bound
    for k, node in enumerate(nodes):
        lo, hi = g['cand_off'][k], g['cand_off'][k + 1]
        got = dict(node.candidates_)
        assert sorted(got) == g['cand_vars'][lo:hi].tolist(), k
        assert rel([got[v] for v in g['cand_vars'][lo:hi]], g['cand_scores'][lo:hi]) <= bound, k
    assert m.params_count() == sum(2 if n.clt is None else n.clt.params_count() for n in nodes)


@pytest.mark.parametrize('name', NAMES)
def test_log_likelihood_matches_the_reference(name):
    g, m = ref.golden(name), with_reference_trees(name)
    ll = guarded(lambda: m.log_likelihood(g['x']))
    fresh = guarded(lambda: m.log_likelihood(g['fresh']))
    print(name, 'log likelihood against the reference: training rows', bar(ll, g['ll_train']), 'fresh rows',
          bar(fresh, g['ll_fresh']))
    assert ll.shape == (len(g['x']),) and ll.dtype == np.float32 and np.isfinite(ll).all()
    assert bar(ll, g['ll_train']) <= 1e-5
    assert bar(fresh, g['ll_fresh']) <= 1e-5


# ---- 4. against the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_learners_match_the_restatement(name):
    g, m, base = ref.golden(name), fitted(name), ref.restated(name)
    nodes = m._nodes()
    assert len(nodes) == len(base)
    roots = np.random.RandomState(7)
    worst = 0.0
    for k, (node, want) in enumerate(zip(nodes, base)):
        assert (node.or_id if node.clt is None else -1) == want['or_id'] and node.scope == want['scope'], k
        assert node.n_rows_ == len(want['rows'])
        assert abs(node.score_ - want['score']) <= 1e-12 * abs(want['score']), k
        assert [v for v, _ in node.candidates_] == [v for v, _ in want['candidates']], k        # the order they were tried
        worst = max(worst, rel([s for _, s in node.candidates_], [s for _, s in want['candidates']]))
        if node.clt is None:
            assert list(node.weights) == want['weights'] and [nodes.index(c) for c in node.children] == want['children']
            continue
        assert node.clt.root == int(roots.choice(len(node.scope))), k                           # breadth first, left before right
        assert np.array_equal(node.clt.tree, want['tree']) and np.array_equal(node.clt.bfs, want['bfs']), k
        assert node.clt.params.dtype == np.float32 and np.max(np.abs(node.clt.params - want['params'])) <= 1e-6, k
    print(name, 'worst relative difference of a candidate score from the restatement', worst)
    assert worst <= 1e-12
    ll = m.log_likelihood(g['fresh'])
    assert bar(ll, cnet_ref.log_likelihood(base, g['fresh'])) <= 1e-5


# ---- 5, 6. reproducible; device tensors ------------------------------------------------------------------------------------
def test_learning_is_reproducible_and_takes_device_tensors():
    g = ref.golden('bic_d33')
    first = model_bytes(fitted('bic_d33'))
    assert model_bytes(learn('bic_d33')) == first
    assert model_bytes(guarded(lambda: learn('bic_d33', torch.from_numpy(g['x']).cuda()), same=model_bytes)) == first
    assert model_bytes(learn('bic_d33', g['x'].astype(np.float64))) == first
    other = learn('bic_d33', random_state=8)
    assert model_bytes(other) != first and np.array_equal(structure(other)[0], structure(fitted('bic_d33'))[0])   # other roots
    assert structure(other)[3] == structure(fitted('bic_d33'))[3]                              # the same undirected trees
    bd = model_bytes(fitted('bd_d24'))
    assert model_bytes(learn('bd_d24', torch.from_numpy(g_x('bd_d24')).cuda())) == bd


def g_x(name):
    return ref.golden(name)['x']


def test_learning_in_chunks_of_one_gives_the_same_model(monkeypatch):
    from deeprob.hip import cnet
    first = model_bytes(fitted('bic_d24'))
    monkeypatch.setattr(cnet, 'COUNT_INTS', 0)
    assert cnet.chunk_tasks(24) == 1
    again = guarded(lambda: learn('bic_d24'), same=model_bytes)
    assert model_bytes(again) == first
    assert again.fit_profile_['launches'] > fitted('bic_d24').fit_profile_['launches']


# ---- 7, 8. the number of candidates; one variable --------------------------------------------------------------------------
@pytest.mark.parametrize('name, k', [('bic_d10', 1), ('bic_d10', 50), ('bd_d24', 1), ('bd_d5', 50)])
def test_one_candidate_and_more_candidates_than_variables(name, k):
    _, kind, par, _ = ref.CONFIGS[name]
    m = guarded(lambda: learn(name, n_cand_cuts=k), same=model_bytes)
    base = ref.learn(g_x(name), kind, par, k, random_state=np.random.RandomState(7))
    nodes = m._nodes()
    assert [(-1 if n.clt is not None else n.or_id) for n in nodes] == [b['or_id'] for b in base]
    for node, want in zip(nodes, base):
        assert [v for v, _ in node.candidates_] == [v for v, _ in want['candidates']]
        assert len(node.candidates_) <= min(k, len(node.scope))
        assert rel([s for _, s in node.candidates_], [s for _, s in want['candidates']]) <= 1e-12
        if node.clt is not None:
            assert np.array_equal(node.clt.tree, want['tree'])
    assert np.isfinite(m.log_likelihood(ref.golden(name)['fresh'])).all()


@pytest.mark.parametrize('kind', ['bd', 'bic'])
def test_one_variable_gives_a_lone_leaf(kind):
    from deeprob.spn.learning import learn_cnet_bd, learn_cnet_bic
    x = g_x('bd_d5')[:, 2:3]
    m = guarded(lambda: (learn_cnet_bd if kind == 'bd' else learn_cnet_bic)(x, random_state=0), same=model_bytes)
    assert m.clt is not None and m.children == [] and m.or_id is None and m.scope == [0] and m.candidates_ == []
    assert m.clt.tree.tolist() == [-1] and m.fit_profile_['generations'] == 0
    smoothing = 0.1 / 4 if kind == 'bd' else 0.01
    p1 = (x.sum() + 2 * smoothing) / (len(x) + 4 * smoothing)
    assert bar(m.log_likelihood(np.array([[1.0], [0.0], [np.nan]], np.float32)), np.log([p1, 1 - p1, 1.0])) <= 1e-5


# ---- 9. launches -----------------------------------------------------------------------------------------------------------
def test_launches_do_not_grow_with_the_tasks_of_a_generation():
    """Two fixtures whose generations have different widths under one bound: the root's two counting calls, then per
    generation gather-pack, pair counts, scores (two kernels), conditioned counts and partition (the last generation
    has nothing to partition)."""
    from deeprob.spn.learning import cnet_bayesian as cb
    infos = {name: fitted(name).fit_profile_ for name in ('bic_d24', 'bic_d33', 'bd_d24')}
    for name, info in infos.items():
        print(name, info)
        deepest = int(ref.golden(name)['node_depth'].max())
        assert info['generations'] == len(info['tasks_per_generation']) and deepest <= info['generations'] <= deepest + 1
        assert info['launches'] <= 2 + cb.LAUNCHES_PER_GENERATION * info['generations']
        assert info['gathers'] <= 1 + info['generations']
        assert 0.0 <= info['host_tree_seconds'] <= info['seconds']
    assert max(infos['bic_d24']['tasks_per_generation']) > max(infos['bd_d24']['tasks_per_generation'])
    assert infos['bic_d24']['tasks_per_generation'] != infos['bic_d33']['tasks_per_generation']
    assert cb.last_profile()['learner'] in ('bd', 'bic')
