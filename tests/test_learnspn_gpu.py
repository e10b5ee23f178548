"""LearnSPN on the HIP device: the statistics kernels alone against numpy on poisoned, guard-banded outputs, the learned
graphs against the reference's golden graphs and against the numpy restatement (tests/learnspn_ref.py), the learned
circuits through the evaluator, EM and MPE."""
import io
import json
import os

import numpy as np
import pytest
import torch

from tests import learnspn_ref as ref
from tests.buffer_contract import contract

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CONFIGS = ['binary16_gvs', 'binary16_rgvs', 'cat3x12_gvs', 'cat3x12_rgvs', 'mixed10_gvs', 'mixed10_rgvs']
LAUNCHES_PER_GENERATION = 14          # DESIGN.md, "LearnSPN on the device"

_cache = {}


def golden(name):
    if name not in _cache:
        g = np.load(os.path.join(GOLDEN, 'learnspn_%s.npz' % name))
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
        g = golden(name)
        dists, doms, _, _ = spec(g['ks'])
        fn = learn_estimator if estimator else learn_spn
        _cache[key] = fn(g['data'].astype(np.float32), dists, doms, split_rows='random', split_cols=name.split('_')[1],
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


# ---- the kernels alone -----------------------------------------------------------------------------------------------------
KERNEL_CASES = {
    # name -> (domain sizes of the data columns, [(rows of the task, its columns)])
    'binary33': ([2] * 33, [(n, list(range(33))) for n in (1, 63, 64, 65, 257)]),
    'k3': ([3, 3, 3], [(257, [0, 1, 2]), (65, [2, 0]), (1, [1, 2]), (64, [1])]),
    'k5': ([5, 5], [(63, [0, 1]), (257, [1, 0]), (1, [0])]),
    'k16': ([16, 16, 16], [(257, [0, 1, 2]), (64, [2, 1]), (1, [0, 2])]),
    'mixed33': ([2, 3, 5, 16] * 8 + [2], [(257, list(range(33))), (65, [3, 0, 7, 1, 2]), (1, [4, 3]), (63, [32])]),
}


@pytest.mark.parametrize('pattern', [0xFF, 0x7F])
@pytest.mark.parametrize('case', sorted(KERNEL_CASES))
def test_counts_and_g_against_numpy(case, pattern):
    from deeprob.hip import learn as L
    ks, tasks = KERNEL_CASES[case]
    rs = np.random.RandomState(len(case))
    n_rows = 300
    x = rs.randint(0, np.asarray(ks), size=(n_rows, len(ks))).astype(np.uint8)
    x[:, 0] = x[:, -1] if ks[0] == ks[-1] and case != 'binary33' else x[:, 0]        # (one dependent pair where it fits)
    data = L.DeviceData(torch.from_numpy(np.ascontiguousarray(x.T)).cuda().reshape(-1), n_rows, len(ks))
    # row subsets through a shuffled index: the segments of the tasks, one after the other
    segs = [np.sort(rs.permutation(n_rows)[:n]) if i % 2 else rs.permutation(n_rows)[:n] for i, (n, _) in enumerate(tasks)]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
    row_index = torch.from_numpy(np.concatenate(segs).astype(np.int32)).cuda()
    kmax = max(2, max(ks))
    item_col, item_off, item_n, want_counts = [], [], [], []
    pairs, want_g = {k: [] for k in ('ci', 'cj', 'off', 'n', 'ki', 'kj')}, []
    for t, (n, cols) in enumerate(tasks):
        rows = segs[t]
        for c in cols:
            item_col.append(c)
            item_off.append(offs[t])
            item_n.append(n)
            want_counts.append(np.bincount(x[rows, c], minlength=kmax))
        for a in range(len(cols)):
            for b in range(a + 1, len(cols)):
                i, j = cols[a], cols[b]
                for k, v in zip(('ci', 'cj', 'off', 'n', 'ki', 'kj'), (i, j, offs[t], n, ks[i], ks[j])):
                    pairs[k].append(v)
                want_g.append(ref.g_value(ref.joint_counts(x[rows, i], x[rows, j], ks[i], ks[j]), n))
    with contract(pattern, record=False) as c:
        c.frozen(data.x, row_index)
        counts = c.expect_written(L.column_counts(data, row_index, item_col, item_off, item_n, kmax))
        g = c.expect_written(L.pair_g(data, row_index, pairs['ci'], pairs['cj'], pairs['off'], pairs['n'], pairs['ki'],
                                      pairs['kj']))
        c.check()
    assert np.array_equal(counts.cpu().numpy(), np.asarray(want_counts)), 'counts must be exactly equal'
    got, want = g.cpu().numpy(), np.asarray(want_g)
    err = np.abs(got - want) / np.abs(want)
    print(case, 'pairs', len(want), 'max rel err of G', float(err.max()))
    assert np.all(err <= 1e-12), (float(err.max()), int(err.argmax()))


@pytest.mark.parametrize('pattern', [0xFF, 0x7F])
def test_partition_rows_is_stable(pattern):
    from deeprob.hip import learn as L
    rs = np.random.RandomState(3)
    src = rs.permutation(5000).astype(np.int32)
    segs = [(0, 1), (1, 63), (64, 64), (128, 65), (193, 257), (450, 1300)]            # (offset, rows) of the parents
    labels = rs.randint(0, 3, size=len(src)).astype(np.uint8)
    child = {k: [] for k in ('so', 'sn', 'lo', 'lb', 'do', 'dn')}
    want = []
    for off, n in segs:
        picks = [(-1, src[off:off + n])] if n == 64 else \
            [(c, src[off:off + n][labels[off:off + n] == c]) for c in range(3) if (labels[off:off + n] == c).any()]
        if n == 65:
            picks.append((-1, src[off:off + n]))           # a copy next to filtered children
        for lb, rows in picks:
            for k, v in zip(('so', 'sn', 'lo', 'lb', 'do', 'dn'), (off, n, off, lb, sum(len(w) for w in want), len(rows))):
                child[k].append(v)
            want.append(rows)
    want = np.concatenate(want)
    with contract(pattern, record=False) as c:
        d_src, d_lab = torch.from_numpy(src).cuda(), torch.from_numpy(labels).cuda()
        c.frozen(d_src, d_lab)
        out = c.expect_written(L.partition_rows(d_src, child['so'], child['sn'], child['lo'], child['lb'], child['do'],
                                                child['dn'], d_lab, len(want)))
        c.check()
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize('pattern', [0xFF, 0x7F])
@pytest.mark.parametrize('n_clusters', sorted(ref.KMEANS_CASE_TASKS))
def test_discrete_kmeans_against_the_restatement(n_clusters, pattern):
    """``dpl_kmeans_*`` alone: one generation of three tasks (300, 256 and 5 or 8 rows) on one matrix with domain sizes
    2, 2, 5, 3, 2 -- both branches of the distance, kmax = 5 above some K -- against ``kmeans_restart`` per restart.  The
    case has no distance ties (tests/learnspn_ref.py:kmeans_case; test_learnspn_host.py asserts its gap >= 1e-6), so labels
    and sizes are exact; the inertia is the same float64 sum in the same order, compared at the float test's 1e-12."""
    from deeprob.hip import learn as L
    assert max(ref.KMEANS_CASE_TASKS) == L.DPL_MAX_CLUSTERS
    x, segments, tasks, want, _ = ref.kmeans_case(n_clusters)
    ks = ref.KMEANS_CASE_KS
    data = L.DeviceData(torch.from_numpy(np.ascontiguousarray(x.T)).cuda().reshape(-1), *x.shape)
    row_index = torch.from_numpy(np.concatenate(segments).astype(np.int32)).cuda()
    offs = np.concatenate([[0], np.cumsum([len(s) for s in segments])])
    with contract(pattern, record=False) as c:
        c.frozen(data.x, row_index)
        batch = L.KMeansBatch(data, row_index, [(offs[i], n, cols, [ks[col] for col in cols], seeds)
                                                for i, (n, cols, seeds) in enumerate(tasks)],
                              ref.KMEANS_CASE_RESTARTS, n_clusters, max(ks))
        inertia, sizes, labels, iterations = batch.run()
        c.expect_written(labels, batch.cent)
        c.check()
    labels = labels.cpu().numpy()
    assert iterations >= 2 or n_clusters == 1
    for i, (n, _, _) in enumerate(tasks):
        for r in range(ref.KMEANS_CASE_RESTARTS):
            w_labels, w_inertia, w_sizes, _ = want[i][r]
            assert np.array_equal(labels[r, batch.lab_off[i]:batch.lab_off[i] + n], w_labels), (i, r)
            assert np.array_equal(sizes[i, r], w_sizes), (i, r)
            err = abs(inertia[i, r] - w_inertia) / (abs(w_inertia) if w_inertia else 1.0)
            print('task', i, 'restart', r, 'inertia', inertia[i, r], 'restated', w_inertia, 'rel err', err)
            assert err <= 1e-12, (i, r)


# ---- the learned graphs ------------------------------------------------------------------------------------------------------
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
    g = golden('mixed10_gvs')
    dists, doms, _, _ = spec(g['ks'])
    flat = learn_spn(torch.from_numpy(g['data'].astype(np.float32)).cuda(), dists, doms, split_rows='random', split_cols='gvs',
                     min_rows_slice=64, random_state=int(g['seed']), verbose=False)
    assert text_of(flat) == text_of(learned('mixed10_gvs', False))


KMEANS_SEEDS = list(range(12))        # the table: the first seed whose restatement gap is >= 1e-6 is the fixture


@pytest.mark.parametrize('name', ['binary16_gvs', 'mixed10_gvs'])
def test_kmeans_route_against_the_restatement(name):
    from deeprob.spn.learning import learn_spn
    g = golden(name)
    dists, doms, names, ks = spec(g['ks'])
    for seed in KMEANS_SEEDS:
        stats = {}
        want = ref.learn_spn(g['data'], names, ks, split_rows='kmeans', split_cols='gvs', min_rows_slice=64, random_state=seed,
                             stats=stats)
        if stats['gap'] >= 1e-6:
            break
    else:
        pytest.fail('no seed of the table has a centroid gap of 1e-6')
    print(name, 'seed', seed, 'centroid gap', stats['gap'])
    flat = learn_spn(g['data'].astype(np.float32), dists, doms, split_rows='kmeans', split_cols='gvs', min_rows_slice=64,
                     random_state=seed, verbose=False)
    assert ref.graphs_differ(digraph(flat), ref.to_digraph(want)) is None


def test_random_cols_route_against_the_restatement():
    from deeprob.spn.learning import learn_spn
    g = golden('mixed10_gvs')
    dists, doms, names, ks = spec(g['ks'])
    want = ref.learn_spn(g['data'], names, ks, split_rows='random', split_cols='random', min_rows_slice=128, random_state=5)
    flat = learn_spn(g['data'].astype(np.float32), dists, doms, split_rows='random', split_cols='random', min_rows_slice=128,
                     random_state=5, verbose=False)
    assert ref.graphs_differ(digraph(flat), ref.to_digraph(want)) is None


def test_quality_on_held_out_rows():
    """Held-out rows of the same mixture are more likely under the learned circuit than under one naive factorisation."""
    from deeprob.spn.learning import learn_estimator
    from deeprob.spn.algorithms.inference import log_likelihood
    ks = [2] * 16
    x, _ = ref.mixture(ks, 2500, seed=5)
    train, test = x[:2000].astype(np.float32), x[2000:].astype(np.float32)
    dists, doms, _, _ = spec(ks)
    flat = learn_estimator(train, dists, doms, split_rows='kmeans', split_cols='gvs', min_rows_slice=64, random_state=0,
                           verbose=False)
    learned_ll = float(np.mean(np.asarray(log_likelihood(flat, test), np.float64)))
    p = (train.sum(0).astype(np.float64) + 0.1) / (len(train) + 0.2)
    naive_ll = float(np.mean(np.sum(np.where(test == 1, np.log(p), np.log1p(-p)), axis=1)))
    print('held-out mean LL: learned', learned_ll, 'naive', naive_ll)
    assert learned_ll > naive_ll


def test_two_runs_are_byte_identical():
    from deeprob.spn.learning import learn_spn
    g = golden('binary16_gvs')
    dists, doms, _, _ = spec(g['ks'])
    texts = [text_of(learn_spn(g['data'].astype(np.float32), dists, doms, split_rows='kmeans', split_cols='gvs',
                               min_rows_slice=64, random_state=11, verbose=False)) for _ in range(2)]
    assert texts[0] == texts[1]


def test_round_trip_through_json_and_em():
    from deeprob.spn.structure.io import load_spn_json
    from deeprob.spn.algorithms.inference import log_likelihood
    from deeprob.spn.learning import expectation_maximization
    g = golden('mixed10_rgvs')
    x = g['data'].astype(np.float32)
    flat = load_spn_json(io.StringIO(text_of(learned('mixed10_rgvs', True))))
    before = float(np.mean(np.asarray(log_likelihood(flat, x), np.float64)))
    expectation_maximization(flat, x, num_iter=5, batch_perc=0.99, step_size=0.5, random_init=False, random_state=0,
                             verbose=False)
    after = float(np.mean(np.asarray(log_likelihood(flat, x), np.float64)))
    print('training mean LL', before, '->', after)
    assert np.isfinite(after) and after >= before - 1e-3


def classifier_data():
    """900 rows of 12 binary features around 3 separated prototypes (10 % noise), the class in the last column."""
    rs = np.random.RandomState(9)
    protos = np.array([[0] * 12, [1] * 6 + [0] * 6, [0] * 6 + [1] * 6], np.uint8)
    z = rs.randint(0, 3, size=900)
    x = np.where(rs.rand(900, 12) < 0.1, rs.randint(0, 2, size=(900, 12)), protos[z])
    return np.column_stack([x, z]).astype(np.float32), [2] * 12 + [3]


def test_classifier():
    from deeprob.spn.learning import learn_classifier
    from deeprob.spn.algorithms.inference import mpe
    data, ks = classifier_data()
    dists, doms, _, _ = spec(ks)
    flat = learn_classifier(data, dists, doms, class_idx=-1, verbose=False, split_rows='random', split_cols='gvs',
                            min_rows_slice=64, random_state=0)
    assert flat.classes[0] == 'Sum' and len(flat.children[0]) == 3
    freq = np.bincount(data[:, -1].astype(int), minlength=3) / len(data)
    assert np.allclose(flat.child_weight[int(flat.arg0[0]):int(flat.arg0[0]) + 3], freq, atol=1e-6)
    query = data.copy()
    query[:, -1] = np.nan
    filled = np.asarray(mpe(flat, query))
    accuracy = float(np.mean(filled[:, -1] == data[:, -1]))
    print('classifier accuracy on the training rows', accuracy)
    assert accuracy >= 0.9


def test_launches_do_not_grow_with_the_tasks_of_a_generation():
    """Random row splits: min_rows_slice 64 and 256 give generations of different widths (k-means splits rows only at the
    root and after a failed column split, so there the two settings can coincide); every route stays under the constant."""
    from deeprob.spn.learning import learn_spn, learnspn
    g = golden('binary16_gvs')
    dists, doms, _, _ = spec(g['ks'])
    assert learnspn.LAUNCHES_PER_GENERATION == LAUNCHES_PER_GENERATION
    infos = {}
    for split_rows, rows in (('random', 64), ('random', 256), ('kmeans', 64)):
        learn_spn(g['data'].astype(np.float32), dists, doms, split_rows=split_rows, split_cols='gvs', min_rows_slice=rows,
                  random_state=3, verbose=False)
        info = infos[split_rows, rows] = learnspn.last_info()
        print(split_rows, 'min_rows_slice', rows, info)
        assert info['generations'] == len(info['tasks_per_generation'])
        assert info['launches'] <= LAUNCHES_PER_GENERATION * info['generations']
    narrow, wide = infos['random', 256]['tasks_per_generation'], infos['random', 64]['tasks_per_generation']
    assert narrow != wide and max(wide) > max(narrow)
    assert infos['kmeans', 64]['lloyd_launches'] > 0
