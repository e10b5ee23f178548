"""The Gaussian-mixture row split on the HIP device: ``dpl_gmm_estep`` and ``dpl_gmm_mstats`` alone against the numpy
restatement (tests/learn_gmm_ref.py) on poisoned, guard-banded memory with several tasks in one launch, then ``gmm`` /
``kmeans`` stand-alone, ``learn_spn(split_rows=gmm)`` against the restated task loops, and the seeding of a mixture of
Chow-Liu trees."""
import numpy as np
import pytest
import torch

from tests import learn_gmm_ref as ref
from tests.buffer_contract import PATTERNS, contract

pytestmark = pytest.mark.gpu

N_ROWS = 700
#: discrete columns 0-11 have K = 3, columns 12 and 13 K = 2, column 14 K = 5
DISC_KS = [3] * 12 + [2, 2, 5]
#: (rows, columns) of the tasks of a generation for C components: n = C (the smallest legal), the sizes around one 256-row
#: block and 300; every segment but the first starts past offset 0 and the scopes differ.  Discrete: one binary column alone
#: (F = 1), 12 columns of K = 3 (F = 36: a full 32-feature tile and a ragged second one), K = 2, 3 and 5 together (F = 9) and
#: F = 38.  Float: column 2 is constant, column 3 is 1000 + randn, and it also stands alone.
TASKS = {'disc': lambda C: [(C, [12, 0]), (255, [12]), (256, list(range(12))), (257, [13, 14, 1]), (300, list(range(14)))],
         'float': lambda C: [(C, [0, 1]), (255, [3]), (256, [0, 1, 2, 3, 4]), (257, [3, 0]), (300, [4, 2, 1])]}
N_INIT = 3

#: the largest deviations from the restatement measured on the MI355X (relative; the denominators of the responsibilities
#: are floored at 1e-280, those of a row's lse at 1), printed by the E-step test; the test asserts ten times each.  numpy's exp and log against the
#: device's, on arguments that agree to the last bits: the quadratic form itself is restated in the device's order.
ESTEP_MEASURED = {'resp': 7.2e-15, 'lse': 2.5e-16, 'lse_sum': 3.1e-16}

_cache = {}


def case(kind, C):
    """(host matrix, device data, device row index, GmmBatch task tuples, per task the [n, F] float64 features), built once."""
    key = (kind, C)
    if key not in _cache:
        from deeprob.hip import learn as L
        rs = np.random.RandomState(11)
        if kind == 'disc':
            x = np.stack([rs.randint(0, k, size=N_ROWS) for k in DISC_KS], axis=1).astype(np.uint8)
            x[:, 1] = np.where(rs.rand(N_ROWS) < 0.7, x[:, 0], x[:, 1])          # some dependence
        else:
            x = np.stack([rs.randn(N_ROWS), np.round(rs.randn(N_ROWS), 1), np.full(N_ROWS, 0.1), 1000.0 + rs.randn(N_ROWS),
                          rs.rand(N_ROWS)], axis=1).astype(np.float32)
        tasks = TASKS[kind](C)
        segs = [np.sort(rs.permutation(N_ROWS)[:n]) if i % 2 else rs.permutation(N_ROWS)[:n] for i, (n, _) in enumerate(tasks)]
        offs = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
        data = L.DeviceData(torch.from_numpy(np.ascontiguousarray(x.T)).cuda().reshape(-1), N_ROWS, x.shape[1])
        row_index = torch.from_numpy(np.concatenate(segs).astype(np.int32)).cuda()
        batch_tasks, feats = [], []
        for t, (n, cols) in enumerate(tasks):
            ks = [DISC_KS[c] for c in cols] if kind == 'disc' else None
            seeds = np.stack([rs.choice(n, C, replace=False) for _ in range(N_INIT)])
            batch_tasks.append((int(offs[t]), n, cols, ks, seeds))
            feats.append(ref.features(x[segs[t]][:, cols], ks))
        _cache[key] = (x, data, row_index, batch_tasks, feats)
    return _cache[key]


def parameters(kind, C):
    """Per (task, init): responsibilities [n, C] (a Dirichlet draw per row; hard 0/1 rows for init 2) and the parameters
    ``ref.pack(ref.m_step(...))`` of them, computed once."""
    key = ('par', kind, C)
    if key not in _cache:
        _, _, _, tasks, feats = case(kind, C)
        rs = np.random.RandomState(5)
        resp, par = {}, {}
        for t, X in enumerate(feats):
            for i in range(N_INIT):
                r = rs.dirichlet([0.7] * C, size=len(X))
                if i == 2:
                    r = ref.one_hot(np.argmax(r, axis=1), C)
                    r[:C] = np.eye(C)                                  # (no component is empty)
                resp[(t, i)] = r
                par[(t, i)] = ref.pack(*ref.m_step(X, r))
        _cache[key] = (resp, par)
    return _cache[key]


def new_batch(kind, C):
    from deeprob.hip import learn as L
    _, data, row_index, tasks, _ = case(kind, C)
    return L.GmmBatch(data, row_index, tasks, C, max(DISC_KS) if kind == 'disc' else None)


def rel(got, want, floor=0.0):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / np.maximum(np.where(want == 0.0, 1.0, np.abs(want)), floor)


# ---- the entries alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('C', [1, 2, 3])
@pytest.mark.parametrize('kind', ['disc', 'float'])
def test_estep_against_the_restatement(kind, C, pattern):
    _, data, row_index, tasks, feats = case(kind, C)
    _, par = parameters(kind, C)
    pairs = sorted(par)
    with contract(pattern, record=False) as c:
        c.frozen(data.x, row_index)
        batch = new_batch(kind, C)
        out, _, _ = batch.launch(pairs, [], par)
        c.expect_written(out, batch.resp, batch.labels, batch.lse)
        c.check()
        again, _, _ = batch.launch(pairs, [], par)
        assert torch.equal(out, again), 'a run repeats bit for bit'
    lse_sum, resp, labels, lse = out.cpu().numpy(), batch.resp.cpu().numpy(), batch.labels.cpu().numpy(), batch.lse.cpu().numpy()
    worst = {'resp': 0.0, 'lse': 0.0, 'lse_sum': 0.0}
    decided = total = 0
    for k, (t, i) in enumerate(pairs):
        n, rows = tasks[t][1], slice(batch.lab_off[t], batch.lab_off[t] + tasks[t][1])
        w_lp, w_resp, w_labels, w_lse, w_sum = ref.estep_entry(feats[t], par[(t, i)])
        if C > 1:
            two = np.sort(w_lp, axis=1)[:, -2:]
            clear = (two[:, 1] - two[:, 0]) >= 1e-6
        else:
            clear = np.ones(n, bool)
        assert np.array_equal(labels[i, rows][clear], w_labels[clear]), (t, i)
        decided, total = decided + int(clear.sum()), total + n
        worst['resp'] = max(worst['resp'], float(rel(resp[i, rows], w_resp, 1e-280).max()))
        worst['lse'] = max(worst['lse'], float(rel(lse[i, rows], w_lse, 1.0).max()))
        worst['lse_sum'] = max(worst['lse_sum'], float(rel(lse_sum[k], w_sum)))
    print(kind, 'C', C, 'labels compared', decided, 'of', total, 'measured relative deviations', worst)
    assert decided >= 0.9 * total
    for key, v in worst.items():
        assert v <= 10.0 * ESTEP_MEASURED[key], (key, v)


def test_estep_leaves_unlisted_pairs_alone():
    kind, C = 'float', 2
    _, par = parameters(kind, C)
    pairs = sorted(par)
    batch = new_batch(kind, C)
    batch.launch(pairs, [], par)
    before = [t.clone() for t in (batch.resp, batch.labels, batch.lse)]
    listed = [a for a in pairs if a[1] != 1]
    shifted = {a: np.concatenate([par[a][:, :1], par[a][:, 1:1 + batch.fs[a[0]]] + 0.25, par[a][:, 1 + batch.fs[a[0]]:]], axis=1)
               for a in pairs}
    batch.launch(listed, [], shifted)
    assert torch.equal(batch.labels[1], before[1][1]) and torch.equal(batch.resp[1], before[0][1])
    assert torch.equal(batch.lse[1], before[2][1]) and not torch.equal(batch.lse[0], before[2][0])


#: (rows of a unit, units of a call): one unit per group in one call; several units per group; several calls
PARTITIONS = {'whole': (1024, None), 'row_chunked': (64, None), 'multi_call': (96, 7)}


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('mfma', [False, True], ids=['valu', 'matrix_core'])
@pytest.mark.parametrize('C', [1, 2, 3])
@pytest.mark.parametrize('kind', ['disc', 'float'])
def test_mstats_within_the_bound_of_any_summation_order(kind, C, mfma, pattern):
    from deeprob.hip import learn as L
    _, data, row_index, tasks, feats = case(kind, C)
    resp, par = parameters(kind, C)
    pairs = sorted(par)
    key = ('mstats_want', kind, C)
    if key not in _cache:
        _cache[key] = {(a, c): ref.mstats_entry(feats[a[0]], resp[a][:, c], par[a][c, 1:1 + feats[a[0]].shape[1]])
                       for a in pairs for c in range(C)}
    want = _cache[key]
    results = {}
    with contract(pattern, record=False) as c:
        c.frozen(data.x, row_index)
        batch = new_batch(kind, C)
        host = np.zeros((N_INIT, batch.n_lab, C))
        for (t, i), r in resp.items():
            host[i, batch.lab_off[t]:batch.lab_off[t] + len(r)] = r
        batch.resp.copy_(torch.from_numpy(host))
        c.frozen(batch.resp)
        for name, (row_chunk, max_units) in PARTITIONS.items():
            out, stat_off, partials = batch.launch([], pairs, par, row_chunk=row_chunk, mfma=mfma,
                                                   max_units=L.GMM_MAX_UNITS if max_units is None else max_units)
            c.expect_written(out, *partials)
            c.check()
            assert (len(partials) > 1) == (name == 'multi_call')
            results[name] = (out, stat_off)
        again, _, _ = batch.launch([], pairs, par, row_chunk=PARTITIONS['row_chunked'][0], mfma=mfma)
        assert torch.equal(again, results['row_chunked'][0]), 'a run repeats bit for bit'
    worst = 0.0
    for name, (out, stat_off) in results.items():
        out = out.cpu().numpy()
        for k, a in enumerate(pairs):
            n, F = feats[a[0]].shape
            per = 1 + F + F * F
            for comp in range(C):
                got = out[stat_off[k] + comp * per:stat_off[k] + (comp + 1) * per]
                w, terms = want[(a, comp)]
                slack = (n + 8) * 2.0 ** -53 * terms
                bad = np.abs(got - w) > slack
                assert not bad.any(), (name, a, comp, int(np.flatnonzero(bad)[0]), float(np.abs(got - w)[bad].max()))
                worst = max(worst, float(np.max(np.abs(got - w) / np.where(slack > 0, slack, 1.0))))
                low = got[1 + F:].reshape(F, F)
                assert np.all(np.abs(low - low.T) <= 2.0 * slack[1 + F:].reshape(F, F)), 'the mirror image is written'
    print(kind, 'C', C, 'matrix core' if mfma else 'VALU', 'largest |got - want| as a share of the bound', worst)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def spec(which):
    from deeprob.spn.structure.leaf import Bernoulli, Gaussian
    data, ks = ref.standalone(which)[:2]
    if ks is None:
        return data, [Gaussian] * data.shape[1], [(-100.0, 100.0)] * data.shape[1]
    return data, [Bernoulli] * len(ks), [[0, 1]] * len(ks)


@pytest.mark.parametrize('which', ['float', 'binary'])
def test_gmm_and_kmeans_standalone_give_the_restated_labels(which):
    from deeprob.spn.learning.splitting import gmm, kmeans
    _, _, want_gmm, want_km, stats = ref.standalone(which)
    assert ref.preconditions(stats), 'the preconditions of the comparison, on the restatement alone'
    data, dists, doms = spec(which)
    cfg = ref.STANDALONE[which]
    for fn, want in ((gmm, want_gmm), (kmeans, want_km)):
        got = fn(data, dists, doms, np.random.RandomState(cfg['seed']), n=cfg['n'])
        assert got.dtype == np.int64 and got.shape == (len(data),) and np.array_equal(got, want), fn.__name__
        tensor = torch.from_numpy(data.astype(np.float32)).cuda()
        assert np.array_equal(fn(tensor, dists, doms, np.random.RandomState(cfg['seed']), n=cfg['n']), want), fn.__name__


def test_learn_spn_with_gmm_gives_the_restated_circuit_on_gaussian_columns():
    from deeprob.spn.learning import learn_spn, learn_estimator, learnspn
    from deeprob.spn.learning.splitting import gmm, kmeans, rdc_cols
    from deeprob.spn.structure.leaf import Gaussian
    from tests import learn_cont_ref as cont
    from tests.test_learn_cont_gpu import circuits_differ
    root, stats = ref.e2e_cont()
    assert ref.preconditions(stats) and stats['margin'] >= 1e-3, 'the preconditions of the comparison, on the restatement alone'
    x, kw = cont.two_blocks(), dict(ref.E2E_CONT, split_cols=rdc_cols, verbose=False)
    flat = learn_spn(x, [Gaussian] * 6, [(-100.0, 100.0)] * 6, split_rows=gmm, **kw)
    info = learnspn.last_info()
    print(info)
    assert circuits_differ(flat, root) is None
    # (the restatement adds the iterations of every task, a generation's tasks advance together here)
    assert 2 <= info['gmm_iterations'] <= stats['iterations'] and info['gmm_kernels'] > 0 and info['gmm_reads'] > 0
    assert info['gmm_uploads'] > 0 and info['launches'] == info['kernels'] + info['reads'] + info['uploads']
    # one upload and one read per EM pass (the label pass included), and per batch the tables, the centroids and the labels
    assert info['gmm_reads'] <= info['gmm_iterations'] + 4 * info['generations']
    assert info['gmm_uploads'] <= info['gmm_iterations'] + 3 * info['generations']
    assert learn_estimator(x, [Gaussian] * 6, [(-100.0, 100.0)] * 6, split_rows=gmm, **kw).n_nodes > 3
    # the function kmeans is the string 'kmeans'
    by_name = learn_spn(x, [Gaussian] * 6, [(-100.0, 100.0)] * 6, split_rows='kmeans', **kw)
    by_function = learn_spn(x, [Gaussian] * 6, [(-100.0, 100.0)] * 6, split_rows=kmeans, **kw)
    assert by_name.classes == by_function.classes and by_name.children == by_function.children
    assert np.array_equal(by_name.raw0, by_function.raw0) and np.array_equal(by_name.child_weight, by_function.child_weight)
    assert learnspn.last_info()['gmm_kernels'] == 0


def test_learn_spn_with_gmm_gives_the_restated_circuit_on_binary_columns():
    from deeprob.spn.learning import learn_spn, learnspn
    from deeprob.spn.learning.splitting import gmm
    from deeprob.spn.structure.io import spn_to_digraph
    from deeprob.spn.structure.leaf import Bernoulli
    root, stats = ref.e2e_disc()
    assert ref.preconditions(stats), 'the preconditions of the comparison, on the restatement alone'
    flat = learn_spn(ref.binary16_e2e().astype(np.float32), [Bernoulli] * 16, [[0, 1]] * 16, split_rows=gmm, verbose=False,
                     **ref.E2E_DISC)
    info = learnspn.last_info()
    print(info)
    assert ref.disc.graphs_differ(spn_to_digraph(flat), ref.disc.to_digraph(root)) is None
    assert 2 <= info['gmm_iterations'] <= stats['iterations']
    # the EM is counted apart: what `launches` counted before keeps its per-generation bound
    assert info['launches'] <= info['launches_per_generation'] * info['generations']


def test_a_mixture_of_chow_liu_trees_seeded_by_gmm():
    from deeprob.spn.learning.splitting import gmm
    from deeprob.spn.structure.cltmix import BinaryCLTMixture
    from deeprob.spn.structure.leaf import Bernoulli
    data = ref.binary16()
    labels = gmm(data, [Bernoulli] * 16, [[0, 1]] * 16, np.random.RandomState(ref.STANDALONE['binary']['seed']), n=2)
    m = BinaryCLTMixture(list(range(16)))
    assert m.fit(data, [[0, 1]] * 16, random_state=0, clusters=labels) is m
    shares = np.bincount(labels, minlength=2) / float(len(data))
    assert len(m.components) == 2 and np.array_equal(m.weights, shares.astype(np.float32))
    assert np.isfinite(np.asarray(m.log_likelihood(data))).all()
