"""``learn_spn(learn_leaf=learn_binary_clt)`` on the HIP device: ``dpl_pair_ones`` alone against numpy on poisoned,
guard-banded outputs, the learned circuits against the reference's goldens (tools/gen_golden_learnspn_clt.py) and against
``BinaryCLT.fit``, and the circuits through the wrappers and the evaluator."""
import io
import json

import numpy as np
import pytest
import torch

from tests import learnspn_ref as ref
from tests import learn_clt_cases as cases
from tests.buffer_contract import contract

pytestmark = pytest.mark.gpu

_cache = {}


def learned(name, to_pc=False):
    """``(circuit, last_info())`` of the replay of a golden (learned once per setting)."""
    key = (name, to_pc)
    if key not in _cache:
        from deeprob.spn.learning import learn_spn, learnspn
        data, dists, doms, kw = cases.call_kwargs(name, to_pc)
        _cache[key] = (learn_spn(data, dists, doms, **kw), learnspn.last_info())
    return _cache[key]


def text_of(flat):
    from deeprob.spn.structure.io import save_spn_json
    buf = io.StringIO()
    save_spn_json(flat, buf)
    return buf.getvalue()


def digraph(flat):
    from deeprob.spn.structure.io import spn_to_digraph
    return spn_to_digraph(flat)


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------
SEGMENTS = (1, 63, 64, 65, 257, 300)
N_ROWS, N_COLS, ZERO_COL, ONE_COL = 400, 80, 5, 6


def kernel_case():
    """Binary data with an all-zero and an all-one column; the six segments one after the other in the row index (every
    one but the first starts past offset 0), sorted and unsorted alternately, over shuffled rows."""
    rs = np.random.RandomState(7)
    x = (rs.rand(N_ROWS, N_COLS) < rs.rand(N_COLS)[None, :]).astype(np.uint8)
    x[:, ZERO_COL], x[:, ONE_COL] = 0, 1
    x[:, 9] = x[:, 8]                                   # (one pair of equal columns)
    segs = [np.sort(rs.permutation(N_ROWS)[:n]) if i % 2 else rs.permutation(N_ROWS)[:n] for i, n in enumerate(SEGMENTS)]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
    return x, segs, offs


def check_pair_ones(blocks, segs_of, pattern, row_chunk=None):
    from deeprob.hip import learn as L
    x, segs, offs = kernel_case()
    data = L.DeviceData(torch.from_numpy(np.ascontiguousarray(x.T)).cuda().reshape(-1), N_ROWS, N_COLS)
    row_index = torch.from_numpy(np.concatenate(segs).astype(np.int32)).cuda()
    L.reset_counters()
    with contract(pattern, record=False) as c:
        c.frozen(data.x, row_index)
        ones, out_off = L.pair_ones(data, row_index, [(offs[s], len(segs[s]), cols) for s, cols in zip(segs_of, blocks)],
                                    row_chunk=row_chunk)
        c.expect_written(ones)
        c.check()
    assert L.COUNTERS['uploads'] == 1 and L.COUNTERS['kernels'] == 2 and L.COUNTERS['reads'] == 0
    got = ones.cpu().numpy()
    assert ones.dtype == torch.int32 and len(got) == sum(len(cols) ** 2 for cols in blocks)
    for s, cols, off in zip(segs_of, blocks, out_off):
        sub = x[segs[s]][:, cols].astype(np.int64)
        want = sub.T @ sub
        m = len(cols)
        block = got[off:off + m * m].reshape(m, m)
        assert np.array_equal(block, want), (len(segs[s]), cols)
        assert np.array_equal(block, block.T) and np.array_equal(np.diag(block), sub.sum(0))


@pytest.mark.parametrize('pattern', [0xFF, 0x7F])
def test_pair_ones_against_numpy(pattern):
    """Every segment with column sets of 33, 17, 2 and 1 columns (the sets in non-increasing order of size, the columns of
    a set in decreasing order), in one launch; the sets share columns, and hold the all-zero and the all-one column."""
    sets = [list(range(39, 6, -1))[:31] + [ONE_COL, ZERO_COL], list(range(20, 3, -1)), [ONE_COL, 3], [12]]
    assert [len(s) for s in sets] == [33, 17, 2, 1] and all(s == sorted(s, reverse=True) for s in sets)
    assert set(sets[0]) & set(sets[1]) and ZERO_COL in sets[1] and ONE_COL in sets[1] and 12 in sets[0]
    blocks, segs_of = [], []
    for s in range(len(SEGMENTS)):
        for cols in sets:
            blocks.append(cols)
            segs_of.append(s)
    check_pair_ones(blocks, segs_of, pattern)


@pytest.mark.parametrize('pattern', [0xFF, 0x7F])
def test_pair_ones_over_column_tiles_and_row_chunks(pattern):
    """The two other paths of the kernel: more than 64 columns (three tile pairs, the mirror image of the off-diagonal one)
    and segments longer than the row chunk (units of one block meeting by atomics), here with a chunk of 128 rows."""
    wide = [int(c) for c in np.random.RandomState(1).permutation(N_COLS)[:70]]
    blocks = [wide, wide, [ONE_COL, 3], wide, [12]]
    segs_of = [5, 0, 4, 3, 5]
    check_pair_ones(blocks, segs_of, pattern, row_chunk=128)
    if pattern == 0xFF:
        check_pair_ones(blocks, segs_of, pattern, row_chunk=64)      # (a chunk of exactly one word)


# ---- the learned circuits -------------------------------------------------------------------------------------------------------
def test_leaves_equal_binaryclt_fit_on_the_same_rows():
    """Each Chow-Liu leaf of a learned circuit is, bit for bit in tree and parameters, ``BinaryCLT(scope, root).fit`` on
    the rows of its task: the same host code on equal counts."""
    from deeprob.spn.structure.cltree import BinaryCLT
    g = cases.golden('a')
    x = g['data'].astype(np.float32)
    _, info = learned('a')
    assert len(info['clt_leaves']) == int(g['clt_leaves'])
    for rec in info['clt_leaves']:
        rows = rec['rows'].cpu().numpy()
        assert len(rows) == rec['n']
        leaf = BinaryCLT(rec['scope'], root=rec['root'])
        leaf.fit(x[rows][:, rec['scope']], [[0, 1]] * len(rec['scope']), alpha=float(g['alpha']))
        assert np.array_equal(leaf.tree, rec['tree']), rec['scope']
        assert leaf.params.dtype == rec['params'].dtype and np.array_equal(leaf.params, rec['params']), rec['scope']


@pytest.mark.parametrize('name', cases.CONFIGS)
def test_graph_and_leaves_against_the_reference(name):
    g = cases.golden(name)
    flat, info = learned(name)
    # the leaves, in queue order: scopes, roots and trees exactly, the CPTs within 1e-6, the rows as a set
    want = cases.golden_leaves(name)
    assert len(info['clt_leaves']) == len(want)
    worst = 0.0
    for rec, (node, rows) in zip(info['clt_leaves'], want):
        assert rec['scope'] == [int(s) for s in node['scope']]
        assert rec['root'] == int(node['params']['root'])
        assert list(rec['tree']) == list(node['params']['tree']), rec['scope']
        assert np.array_equal(np.sort(rec['rows'].cpu().numpy()), np.sort(rows))
        err = float(np.max(np.abs(rec['params'].astype(np.float64) - np.asarray(node['params']['params']))))
        worst = max(worst, err)
        assert err <= 1e-6, rec['scope']
    print(name, len(want), 'leaves, max abs err of the CPTs', worst)
    # the whole circuit: the reference's to_pc=True graph (every node above and inside the leaves: ids, classes, scopes and
    # edges exactly, weights within 1e-6) ...
    assert ref.graphs_differ(digraph(flat), json.loads(str(g['pc_json']))) is None
    # ... and the nodes above the leaves of the to_pc=False graph, whose expansion it is
    assert ref.graphs_differ(digraph(flat), digraph(cases.expand(json.loads(str(g['clt_json']))))) is None


@pytest.mark.parametrize('name', cases.CONFIGS)
def test_likelihoods_against_the_reference(name):
    from deeprob.spn.algorithms.inference import log_likelihood
    g = cases.golden(name)
    flat, _ = learned(name)
    x = g['data'].astype(np.float32)
    x_nan = x.copy()
    x_nan[np.unpackbits(g['nan_mask'])[:x.size].reshape(x.shape).astype(bool)] = np.nan
    for data, want in ((x, g['ll']), (x_nan, g['ll_nan'])):
        got = np.asarray(log_likelihood(flat, data), np.float64).reshape(-1)
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        print(name, 'max rel err of LL', float(err.max()))
        assert np.all(err <= 1e-5)


@pytest.mark.parametrize('name', cases.CONFIGS)
def test_to_pc_true_and_false_give_the_same_circuit(name):
    assert text_of(learned(name, True)[0]) == text_of(learned(name, False)[0])


def test_device_tensor_input_gives_the_same_circuit():
    from deeprob.spn.learning import learn_spn
    data, dists, doms, kw = cases.call_kwargs('b')
    flat = learn_spn(torch.from_numpy(data).cuda(), dists, doms, **kw)
    assert text_of(flat) == text_of(learned('b')[0])


def test_an_integer_leaf_seed_reseeds_for_every_leaf():
    from deeprob.spn.learning import learn_spn, learnspn
    data, dists, doms, kw = cases.call_kwargs('a')
    kw['learn_leaf_kwargs'] = dict(kw['learn_leaf_kwargs'], random_state=7)
    learn_spn(data, dists, doms, **kw)
    leaves = learnspn.last_info()['clt_leaves']
    assert len(leaves) == int(cases.golden('a')['clt_leaves'])         # (the splits do not see the leaves' generator)
    for rec in leaves:
        assert rec['root'] == rec['scope'][int(np.random.RandomState(7).choice(len(rec['scope'])))]


def test_learn_estimator_gives_the_pruned_circuit():
    from deeprob.spn.learning import learn_estimator
    from deeprob.spn.algorithms.structure import prune
    from deeprob.spn.algorithms.inference import log_likelihood
    data, dists, doms, kw = cases.call_kwargs('a')
    est = learn_estimator(data, dists, doms, **kw)
    flat, _ = learned('a')
    before = text_of(flat)
    assert text_of(est) == text_of(prune(flat))
    assert text_of(flat) == before and len(est.classes) < len(flat.classes)
    got, want = (np.asarray(log_likelihood(c, data), np.float64).reshape(-1) for c in (est, flat))
    assert np.all(np.abs(got - want) / np.maximum(1.0, np.abs(want)) <= 1e-5)


def test_learn_classifier_on_a_bernoulli_class_column():
    from deeprob.spn.learning import learn_classifier
    from deeprob.spn.learning.leaf import learn_binary_clt
    from deeprob.spn.structure.leaf import Bernoulli
    from deeprob.spn.algorithms.inference import mpe
    rs = np.random.RandomState(9)
    protos = np.array([[0] * 6 + [1] * 6, [1] * 6 + [0] * 6], np.uint8)
    z = rs.randint(0, 2, size=800)
    x = np.where(rs.rand(800, 12) < 0.1, rs.randint(0, 2, size=(800, 12)), protos[z])
    data = np.column_stack([x, z]).astype(np.float32)
    flat = learn_classifier(data, [Bernoulli] * 13, [[0, 1]] * 13, class_idx=-1, verbose=False, learn_leaf=learn_binary_clt,
                            split_rows='random', split_cols='gvs', min_rows_slice=128, random_state=0,
                            learn_leaf_kwargs={'random_state': 1})
    assert flat.classes[0] == 'Sum' and len(flat.children[0]) == 2
    query = data.copy()
    query[:, -1] = np.nan
    accuracy = float(np.mean(np.asarray(mpe(flat, query))[:, -1] == data[:, -1]))
    print('classifier accuracy on the training rows', accuracy)
    assert accuracy >= 0.9


def test_clt_leaves_fit_better_than_mle_leaves():
    from deeprob.spn.learning import learn_spn
    from deeprob.spn.algorithms.inference import log_likelihood
    data, dists, doms, kw = cases.call_kwargs('a')
    mle = learn_spn(data, dists, doms, **dict(kw, learn_leaf='mle', learn_leaf_kwargs={'alpha': kw['learn_leaf_kwargs']['alpha']}))
    ll_clt = float(np.mean(np.asarray(log_likelihood(learned('a')[0], data), np.float64)))
    ll_mle = float(np.mean(np.asarray(log_likelihood(mle, data), np.float64)))
    print('mean training LL: CLT leaves', ll_clt, 'MLE leaves', ll_mle)
    assert ll_clt > ll_mle


def test_mpe_and_sample_return_complete_rows():
    from deeprob.spn.algorithms.inference import mpe
    from deeprob.spn.algorithms.sampling import sample
    g = cases.golden('b')
    flat, _ = learned('b')
    x = g['data'][:200].astype(np.float32)
    x[np.random.RandomState(2).rand(*x.shape) < 0.4] = np.nan
    x[0] = np.nan
    for filled in (np.asarray(mpe(flat, x)), np.asarray(sample(flat, x, seed=3))):
        assert np.isin(filled, (0.0, 1.0)).all()
        assert np.array_equal(filled[~np.isnan(x)], x[~np.isnan(x)])


def test_the_function_on_its_own():
    from deeprob.spn.learning.leaf import learn_binary_clt, learn_mle
    from deeprob.spn.structure.cltree import BinaryCLT
    from deeprob.spn.structure.leaf import Bernoulli
    g = cases.golden('a')
    x = g['data'][:500, :5].astype(np.float32)
    scope = [10, 11, 12, 13, 14]
    one = learn_binary_clt(x[:, :1], [Bernoulli], [[0, 1]], [10], alpha=0.1)
    assert one.classes == ['Bernoulli'] and text_of(one) == text_of(learn_mle(x[:, :1], [Bernoulli], [[0, 1]], [10]))
    assert abs(float(one.raw0[0]) - (x[:, 0].sum() + 0.1) / (500 + 0.2)) <= 1e-6
    leaf = learn_binary_clt(x, [Bernoulli] * 5, [[0, 1]] * 5, scope, random_state=4)
    want = BinaryCLT(scope, root=scope[int(np.random.RandomState(4).choice(5))])
    want.fit(x, [[0, 1]] * 5)
    assert isinstance(leaf, BinaryCLT) and np.array_equal(leaf.tree, want.tree) and np.array_equal(leaf.params, want.params)
    pc = learn_binary_clt(x, [Bernoulli] * 5, [[0, 1]] * 5, scope, to_pc=True, random_state=4)
    assert text_of(pc) == text_of(want.to_pc())
    naive = learn_mle(x, [Bernoulli] * 5, [[0, 1]] * 5, scope)
    assert naive.classes == ['Product'] + ['Bernoulli'] * 5


def test_launches_stay_within_the_bound_of_a_generation():
    """The two goldens have different numbers of leaves and of tasks per generation; both stay within the per-generation
    constant, which is the one of MLE leaves plus the four of ``pair_ones``."""
    from deeprob.spn.learning import learnspn
    infos = {name: learned(name)[1] for name in cases.CONFIGS}
    assert len(infos['a']['clt_leaves']) != len(infos['b']['clt_leaves'])
    for name, info in infos.items():
        print(name, {k: v for k, v in info.items() if k != 'clt_leaves'})
        bound = learnspn.LAUNCHES_PER_GENERATION + learnspn.CLT_LAUNCHES_PER_GENERATION
        assert info['launches_per_generation'] == bound == 18
        assert info['launches'] <= bound * info['generations']
