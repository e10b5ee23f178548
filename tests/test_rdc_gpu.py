"""RDC column splits on the HIP device: ``dpl_pair_maxcorr`` alone against the two restatements of tests/rdc_ref.py on
poisoned, guard-banded outputs, ``rdc_scores`` against the reference's scores, and ``learn_spn`` / ``learn_estimator`` /
``learn_classifier`` with ``split_cols=rdc_cols`` against the reference's golden graphs and the numpy restatement."""
import io
import json
import os

import numpy as np
import pytest
import torch

from tests import learnspn_ref as ref
from tests import rdc_cases as cases
from tests import rdc_ref
from tests.buffer_contract import contract

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CONFIGS = ['binary16', 'mixed10', 'cat3x12', 'wide16']
LAUNCHES_PER_GENERATION = 14          # DESIGN.md, "LearnSPN on the device"

_cache = {}


def golden(name):
    if name not in _cache:
        g = np.load(os.path.join(GOLDEN, 'rdc_%s.npz' % name))
        _cache[name] = {k: g[k] for k in g.files}
    return _cache[name]


def spec(ks):
    from deeprob.spn.structure.leaf import Bernoulli, Categorical
    ks = [int(k) for k in ks]
    return ([Bernoulli if k == 2 else Categorical for k in ks], [list(range(k)) for k in ks],
            ['Bernoulli' if k == 2 else 'Categorical' for k in ks], ks)


def learned(name, estimator):
    """The circuit learned on a golden configuration with the golden's settings (learned once)."""
    key = ('learned', name, estimator)
    if key not in _cache:
        from deeprob.spn.learning import learn_spn, learn_estimator
        from deeprob.spn.learning.splitting.rdc import rdc_cols
        g = golden(name)
        dists, doms, _, _ = spec(g['ks'])
        fn = learn_estimator if estimator else learn_spn
        _cache[key] = fn(g['data'].astype(np.float32), dists, doms, split_rows='random', split_cols=rdc_cols,
                         min_rows_slice=int(g['min_rows_slice']), random_state=int(g['seed']), verbose=False)
    return _cache[key]


def digraph(flat):
    from deeprob.spn.structure.io import spn_to_digraph
    return spn_to_digraph(flat)


def text_of(flat):
    from deeprob.spn.structure.io import save_spn_json
    buf = io.StringIO()
    save_spn_json(flat, buf)
    return buf.getvalue()


def maxcorr_on_device(x, row_index, pairs, pattern):
    """``pairs``: (column i, column j, row offset, rows, ki, kj) records, one launch under the buffer contract."""
    from deeprob.hip import learn as L
    data = L.DeviceData(torch.from_numpy(np.ascontiguousarray(x.T)).cuda().reshape(-1), x.shape[0], x.shape[1])
    index = torch.from_numpy(np.asarray(row_index, np.int32)).cuda()
    ci, cj, off, n, ki, kj = (list(v) for v in zip(*pairs))
    with contract(pattern, record=False) as c:
        c.frozen(data.x, index)
        before = L.COUNTERS['kernels']
        score = c.expect_written(L.pair_maxcorr(data, index, ci, cj, off, n, ki, kj))
        assert L.COUNTERS['kernels'] == before + 1
        c.check()
    assert score.dtype == torch.float64 and tuple(score.shape) == (len(pairs),)
    return score.cpu().numpy()


# ---- the kernel alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pattern', [0xFF, 0x7F])
def test_maxcorr_against_the_restatements(pattern):
    """Segments of 1, 2, 63, 64, 65, 257 and 1000 rows through a shuffled index, all column pairs of tests/rdc_cases.py in
    ONE launch: |device - SVD| <= 1e-12 (Jacobi is accurate to a few K eps and the scores are <= 1) and
    |device - the header's order in Python floats| <= 1e-13."""
    k = cases.kernel_case()
    offs = np.concatenate([[0], np.cumsum([len(s) for s in k['segs']])])
    pairs = [(ci, cj, offs[t], len(k['segs'][t]), ki, kj) for ci, cj, t, ki, kj in k['pairs']]
    got = maxcorr_on_device(k['x'], np.concatenate(k['segs']), pairs, pattern)
    svd = np.array([rdc_ref.maxcorr_svd(t) for t in k['tables']])
    jac = np.array([rdc_ref.maxcorr_jacobi(t) for t in k['tables']])
    print('pairs', len(pairs), 'max |device - svd|', float(np.abs(got - svd).max()), 'max |device - jacobi order|',
          float(np.abs(got - jac).max()))
    assert np.all((got >= 0.0) & (got <= 1.0))
    assert np.all(np.abs(got - svd) <= 1e-12), int(np.abs(got - svd).argmax())
    assert np.all(np.abs(got - jac) <= 1e-13), int(np.abs(got - jac).argmax())
    per_pair = got.reshape(len(cases.SEGMENTS), len(cases.PAIRS))
    assert np.all(per_pair[0] == 0.0), 'one row: every column is constant'
    assert np.all(per_pair[:, 7] == 0.0), 'a constant column'
    assert np.all(np.abs(per_pair[2:, 5] - 1.0) <= 1e-12), 'duplicate columns'


@pytest.mark.parametrize('pattern', [0xFF, 0x7F])
def test_maxcorr_of_hand_tables(pattern):
    """Each hand table as a row segment of two columns with the stated K = 16 (absent values drop out)."""
    tables = cases.hand_tables()
    rows = [cases.rows_of(t) for _, t, _ in tables]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    x = np.concatenate(rows)
    pairs = [(0, 1, offs[i], len(rows[i]), 16, 16) for i in range(len(tables))]
    pairs += [(1, 0, offs[i], len(rows[i]), 16, 16) for i in range(len(tables))]
    got = maxcorr_on_device(x, np.arange(len(x)), pairs, pattern)
    want = np.array([w for _, _, w in tables] * 2)
    print('hand tables: max |device - known|', float(np.abs(got - want).max()))
    assert np.all(np.abs(got - want) <= 1e-12)
    for i, (name, _, w) in enumerate(tables):
        if w == 0.0 and name.startswith('one present'):
            assert got[i] == 0.0 and got[i + len(tables)] == 0.0


# ---- rdc_scores ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CONFIGS)
def test_scores_against_the_reference(name):
    from deeprob.spn.learning.splitting.rdc import rdc_scores
    g = golden(name)
    dists, doms, _, ks = spec(g['ks'])
    rs, want_rs = np.random.RandomState(0), np.random.RandomState(0)
    got = rdc_scores(g['data'].astype(np.float32), dists, doms, rs)
    for K in ks:                                        # rdc.py:170-176
        want_rs.randn(K, 20)
        want_rs.randn(20)
    assert rs.randint(0, 2 ** 31 - 1, size=4).tolist() == want_rs.randint(0, 2 ** 31 - 1, size=4).tolist()
    assert got.dtype == np.float64 and np.array_equal(np.diag(got), np.ones(len(ks))) and np.array_equal(got, got.T)
    err = float(np.abs(got - g['scores_ref']).max())
    exact = float(np.abs(got - rdc_ref.rdc_scores(g['data'], ks, np.random.RandomState(0))).max())
    print(name, 'max |device - reference|', err, 'max |device - svd|', exact)
    assert err <= (1e-6 if max(ks) == 2 else 1e-4) and exact <= 1e-12
    on_device = rdc_scores(torch.from_numpy(g['data'].astype(np.float32)).cuda(), dists, doms, np.random.RandomState(0))
    assert np.array_equal(on_device, got)


def test_cols_labels():
    from deeprob.spn.learning.splitting.rdc import rdc_cols
    g = golden('mixed10')
    dists, doms, _, ks = spec(g['ks'])
    labels = rdc_cols(g['data'].astype(np.float32), dists, doms, np.random.RandomState(0), d=0.3)
    want = rdc_ref.rdc_cols(g['data'], ks, np.random.RandomState(0), d=0.3)
    assert labels.dtype == np.int32 and labels.tolist() == want.tolist()


# ---- the learned graphs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('estimator', [False, True], ids=['learn_spn', 'learn_estimator'])
@pytest.mark.parametrize('name', CONFIGS)
def test_structure_against_the_reference(name, estimator):
    want = json.loads(str(golden(name)['est_json' if estimator else 'spn_json']))
    assert ref.graphs_differ(digraph(learned(name, estimator)), want) is None


@pytest.mark.parametrize('name', CONFIGS)
def test_likelihoods_against_the_reference(name):
    from deeprob.spn.algorithms.inference import log_likelihood
    g = golden(name)
    x = g['data'].astype(np.float32)
    x_nan = x.copy()
    x_nan[np.unpackbits(g['nan_mask'])[:x.size].reshape(x.shape).astype(bool)] = np.nan
    for circuit, data, want in ((learned(name, True), x, g['ll']), (learned(name, True), x_nan, g['ll_nan']),
                                (learned(name, False), x, g['ll_spn'])):
        got = np.asarray(log_likelihood(circuit, data), np.float64).reshape(-1)
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        print(name, 'max rel err of LL', float(err.max()))
        assert np.all(err <= 1e-5)


def test_device_tensor_input_gives_the_same_graph():
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting.rdc import rdc_cols
    g = golden('mixed10')
    dists, doms, _, _ = spec(g['ks'])
    flat = learn_spn(torch.from_numpy(g['data'].astype(np.float32)).cuda(), dists, doms, split_rows='random', split_cols=rdc_cols,
                     min_rows_slice=int(g['min_rows_slice']), random_state=int(g['seed']), verbose=False)
    assert text_of(flat) == text_of(learned('mixed10', False))


def test_two_runs_are_byte_identical():
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting.rdc import rdc_cols
    g = golden('wide16')
    dists, doms, _, _ = spec(g['ks'])
    texts = [text_of(learn_spn(g['data'].astype(np.float32), dists, doms, split_rows='kmeans', split_cols=rdc_cols,
                               min_rows_slice=128, random_state=11, verbose=False)) for _ in range(2)]
    assert texts[0] == texts[1]


def device_kmeans(rows, ks, rs, n, stats=None):
    """The device's k-means on one slice, seeded as ``learn_spn`` seeds it: the labels of the restart it would pick."""
    from deeprob.hip import learn as L
    from deeprob.spn.learning.learnspn import KMEANS_RESTARTS
    seeds = np.stack([rs.choice(len(rows), n, replace=False) for _ in range(KMEANS_RESTARTS)])
    data = L.DeviceData(torch.from_numpy(np.ascontiguousarray(rows.T).astype(np.uint8)).cuda().reshape(-1), *rows.shape)
    index = torch.arange(len(rows), dtype=torch.int32, device='cuda')
    batch = L.KMeansBatch(data, index, [(0, len(rows), list(range(rows.shape[1])), list(ks), seeds)], KMEANS_RESTARTS, n,
                          max(2, max(ks)))
    inertia, _, labels, _ = batch.run()
    return labels[int(np.argmin(inertia[0]))].cpu().numpy().astype(np.int64)


def test_kmeans_route_against_the_restatement():
    """k-means row splits with rdc column splits.  On this data the rows that k-means is asked to split after a failed
    column split hold few distinct values and tie between centroids (the restatement's centroid gap is 0 for every seed
    tried), so the restatement is fed the device's own k-means labels, slice by slice: what is compared is everything
    else -- the draws, the scores, the components and the graph.  Every score is >= 1e-9 away from d; the device's is
    within 1e-12 of the restatement's, so no decision can flip."""
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting.rdc import rdc_cols
    g = golden('mixed10')
    dists, doms, names, ks = spec(g['ks'])
    stats = {}
    want = rdc_ref.learn_spn(g['data'], names, ks, split_rows='kmeans', min_rows_slice=128, random_state=4, stats=stats,
                             kmeans=device_kmeans)
    print('score margin', stats.get('margin'), 'rdc calls', stats.get('calls'))
    assert stats['calls'] > 0 and stats['margin'] >= 1e-9
    flat = learn_spn(g['data'].astype(np.float32), dists, doms, split_rows='kmeans', split_cols=rdc_cols, min_rows_slice=128,
                     random_state=4, verbose=False)
    assert ref.graphs_differ(digraph(flat), ref.to_digraph(want)) is None


def test_split_cols_kwargs_reach_the_split():
    """d = 0.9 and k = 25 (more numbers drawn per column) against the restatement given the same: another graph than
    with the defaults.  The restatement's scores are >= 1e-9 away from d, the device's within 1e-12 of them."""
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.learning.splitting.rdc import rdc_cols
    g = golden('mixed10')
    dists, doms, names, ks = spec(g['ks'])
    stats = {}
    want = rdc_ref.learn_spn(g['data'], names, ks, split_rows='random', min_rows_slice=128, random_state=int(g['seed']), d=0.9,
                             k=25, stats=stats)
    assert stats['calls'] > 0 and stats['margin'] >= 1e-9
    flat = learn_spn(g['data'].astype(np.float32), dists, doms, split_rows='random', split_cols=rdc_cols,
                     split_cols_kwargs={'d': 0.9, 'k': 25, 's': 0.5}, min_rows_slice=128, random_state=int(g['seed']), verbose=False)
    assert ref.graphs_differ(digraph(flat), ref.to_digraph(want)) is None
    assert ref.graphs_differ(digraph(flat), digraph(learned('mixed10', False))) is not None


def test_launches_do_not_grow_with_the_tasks_of_a_generation():
    from deeprob.spn.learning import learn_spn, learnspn
    from deeprob.spn.learning.splitting.rdc import rdc_cols
    g = golden('binary16')
    dists, doms, _, _ = spec(g['ks'])
    assert learnspn.LAUNCHES_PER_GENERATION == LAUNCHES_PER_GENERATION
    infos = {}
    for split_rows, rows in (('random', 64), ('random', 256), ('kmeans', 64)):
        learn_spn(g['data'].astype(np.float32), dists, doms, split_rows=split_rows, split_cols=rdc_cols, min_rows_slice=rows,
                  random_state=3, verbose=False)
        info = infos[split_rows, rows] = learnspn.last_info()
        print(split_rows, 'min_rows_slice', rows, info)
        assert info['generations'] == len(info['tasks_per_generation'])
        assert info['launches'] <= LAUNCHES_PER_GENERATION * info['generations']
    narrow, wide = infos['random', 256]['tasks_per_generation'], infos['random', 64]['tasks_per_generation']
    assert narrow != wide and max(wide) > max(narrow)


def test_classifier():
    from tests.test_learnspn_gpu import classifier_data
    from deeprob.spn.learning import learn_classifier
    from deeprob.spn.learning.splitting.rdc import rdc_cols
    from deeprob.spn.algorithms.inference import mpe
    data, ks = classifier_data()
    dists, doms, _, _ = spec(ks)
    flat = learn_classifier(data, dists, doms, class_idx=-1, verbose=False, split_rows='random', split_cols=rdc_cols,
                            min_rows_slice=64, random_state=0)
    assert flat.classes[0] == 'Sum' and len(flat.children[0]) == 3
    query = data.copy()
    query[:, -1] = np.nan
    accuracy = float(np.mean(np.asarray(mpe(flat, query))[:, -1] == data[:, -1]))
    print('classifier accuracy on the training rows', accuracy)
    assert accuracy >= 0.9
