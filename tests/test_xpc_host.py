"""The XPC learners without a device: the numpy restatement (tests/xpc_ref.py) against the reference's fixtures
(tests/golden/xpc_*.npz, tools/gen_golden_xpc.py), the ``dpc_xpc_*`` entries of the CLT header and library, the argument
errors of ``learn_xpc`` / ``learn_expc``, the ``Partition`` record and the routing of ``learn_estimator``."""
import os
import re

import numpy as np
import pytest

from tests import xpc_ref

LL_BAR = 1e-5               # the project's bar: |got - want| / max(1, |want|)
MAX_BYTES = 150 * 1000


def _close(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape and np.isfinite(want).all()
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


# ---- the restatement against the reference -------------------------------------------------------------------------------
def test_configurations_cover_the_learners():
    kws = [kw for _, _, kw in xpc_ref.CONFIGS.values()]
    xpcs = [kw for learner, _, kw in xpc_ref.CONFIGS.values() if learner == 'xpc']
    assert {s[:2] for _, s, _ in xpc_ref.CONFIGS.values()} == {(600, 12), (2000, 24), (4097, 40)}
    assert {kw['min_part_inst'] for kw in kws} == {32, 64} and {kw['conj_len'] for kw in kws} == {2, 3}
    assert {kw['arity'] for kw in kws} == {3, 4} and all(40 <= kw['n_max_parts'] <= 60 for kw in kws)
    assert {(kw['sd'], kw['det']) for kw in xpcs} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(not kw.get('use_clt', True) and not kw['det'] for kw in xpcs) and any(kw.get('use_greedy_ordering') for kw in xpcs)
    ensembles = [(s[:2], kw) for learner, s, kw in xpc_ref.CONFIGS.values() if learner == 'expc']
    assert sorted(kw['sd_level'] for _, kw in ensembles) == [0, 1, 2]
    assert all(shape == (2000, 24) and kw['ensemble_dim'] == 4 for shape, kw in ensembles)


@pytest.mark.parametrize('name', list(xpc_ref.CONFIGS))
def test_restatement_makes_the_decisions_of_the_reference(name):
    g = xpc_ref.golden(name)
    assert os.path.getsize(os.path.join(xpc_ref.GOLDEN, 'xpc_%s.npz' % name)) <= MAX_BYTES
    learner, shape, _ = xpc_ref.CONFIGS[name]
    assert (int(g['n_rows']), int(g['n_vars']), int(g['data_seed'])) == (shape[0], shape[1], shape[4])
    model = xpc_ref.restated(name)
    assert len(model['members']) == int(g['n_members'])
    for m, member in enumerate(model['members']):
        for k, v in xpc_ref.tree_record(member['root'], int(g['n_rows'])).items():
            assert np.array_equal(v, g['m%d_%s' % (m, k)]), (m, k)
        assert member['n_parts'] == int(g['m%d_n_parts' % m])
        assert member['conj_vars_l'] == g['m%d_conj_vars' % m].tolist()
        xpc_ref.assert_trees(name, m, member['trees_dict'])
        for node in xpc_ref.preorder(member['root']):           # the reference's row ids are ascending in every partition
            assert (np.diff(node['rows']) > 0).all()


@pytest.mark.parametrize('name', list(xpc_ref.CONFIGS))
def test_restatement_log_likelihoods(name):
    g = xpc_ref.golden(name)
    model = xpc_ref.restated(name)
    for rows, want in ((g['x'], g['ll_train']), (g['fresh'], g['ll_fresh']), (xpc_ref.queries(g['fresh']), g['ll_nan'])):
        assert _close(xpc_ref.log_likelihood(model, rows), want) <= LL_BAR


def test_an_sd_fixture_has_only_unique_spanning_trees():
    unique = []
    for name, (learner, _, kw) in xpc_ref.CONFIGS.items():
        g = xpc_ref.golden(name)
        flags = [g['m%d_tree_unique' % m] for m in range(int(g['n_members']))]
        if all(len(f) for f in flags) and all(f.all() for f in flags):
            unique.append(name)
    assert unique


def test_restatement_marginalises_exactly():
    """All NaN gives log 1; a row with one NaN entry is the log-sum of its two completions."""
    g = xpc_ref.golden('b24det')
    model = xpc_ref.restated('b24det')
    rows = g['fresh'][:8].copy()
    assert abs(xpc_ref.log_likelihood(model, np.full((1, rows.shape[1]), np.nan))[0]) <= 1e-5
    hole = rows.copy()
    hole[:, 5] = np.nan
    zero, one = rows.copy(), rows.copy()
    zero[:, 5], one[:, 5] = 0, 1
    both = np.logaddexp(xpc_ref.log_likelihood(model, zero), xpc_ref.log_likelihood(model, one))
    assert _close(xpc_ref.log_likelihood(model, hole), both) <= LL_BAR


# ---- header and library ------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_once_and_the_library_exports_them():
    from deeprob.hip import clt
    with open(clt.HEADER_PATH) as f:
        text = re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)
    entries = sorted(s for s in clt.SIGNATURES if s.startswith('dpc_xpc_'))
    assert entries == ['dpc_xpc_code_counts', 'dpc_xpc_partition']
    for name in entries:
        assert len(re.findall(r'\b%s\s*\(' % name, text)) == 1
    lib = clt.load_library()
    for name in entries:
        assert getattr(lib, name).argtypes == clt.SIGNATURES[name][1]
    assert lib.dpc_abi_version() >= 4 and clt.DPC_XPC_MAX_CONJ == 8 and clt.DPC_XPC_CHUNK % 64 == 0
    import deeprob.spn.learning as learning
    assert learning.SD_LEVELS == [learning.SD_LEVEL_0, learning.SD_LEVEL_1, learning.SD_LEVEL_2] == [0, 1, 2]


# ---- arguments -----------------------------------------------------------------------------------------------------------------
def _data():
    return (np.arange(400).reshape(50, 8) % 3 == 0).astype(np.float32)


GOOD = dict(det=False, sd=False, min_part_inst=4, conj_len=2, arity=2)


@pytest.mark.parametrize('change, message', [
    (dict(conj_len=0), "conj_len must be in the interval [1, 8] (DPC_XPC_MAX_CONJ)"),
    (dict(conj_len=9), "conj_len must be in the interval [1, 8] (DPC_XPC_MAX_CONJ)"),
    (dict(arity=1), "Arity must be in the interval [2, 2 ** conj_len]"),
    (dict(min_part_inst=0), "min_part_inst must be at least 1"),
    (dict(use_greedy_ordering=True), "Using the greedy ordering makes sense only if sd = True."),
    (dict(det=True, use_clt=False), None),
])
def test_learn_xpc_argument_errors(change, message):
    from deeprob.spn.learning import learn_xpc
    with pytest.raises(ValueError) as e:
        learn_xpc(_data(), **dict(GOOD, **change))
    assert message is None or str(e.value) == message


@pytest.mark.parametrize('change, message', [
    (dict(sd_level=3), "Choose a value in {0, 1, 2}."),
    (dict(sd_level=2, conj_len=1), "No randomness in this setting. Change hyper parameters."),
    (dict(arity=1), "Arity must be in the interval [2, 2 ** conj_len]"),
    (dict(conj_len=9), "conj_len must be in the interval [1, 8] (DPC_XPC_MAX_CONJ)"),
    (dict(min_part_inst=0), "min_part_inst must be at least 1"),
    (dict(det=True, use_clt=False), None),
    (dict(ensemble_dim=0), "ensemble_dim must be at least 1"),
])
def test_learn_expc_argument_errors(change, message):
    from deeprob.spn.learning import learn_expc
    kw = dict(ensemble_dim=2, det=False, sd_level=0, min_part_inst=4, conj_len=2, arity=2)
    with pytest.raises(ValueError) as e:
        learn_expc(_data(), **dict(kw, **change))
    assert message is None or str(e.value) == message


@pytest.mark.parametrize('spoil', [2.0, 0.5, np.nan])
def test_data_must_be_binary(spoil):
    from deeprob.spn.learning import learn_expc, learn_xpc
    data = _data()
    data[3, 2] = spoil
    with pytest.raises(ValueError):
        learn_xpc(data, **GOOD)
    with pytest.raises(ValueError):
        learn_expc(data, ensemble_dim=2, det=False, sd_level=0, min_part_inst=4, conj_len=2, arity=2)


def test_an_arity_beyond_the_codes_is_accepted():
    """``arity > 2 ** conj_len`` passes the checks, as the reference's assertion lets it."""
    from deeprob.spn.learning import xpc
    xpc._check(conj_len=1, arity=5, min_part_inst=1, det=False, use_clt=True)


# ---- the partition record and the host decision ------------------------------------------------------------------------------------
def test_partition_is_the_reference_record():
    from deeprob.spn.utils.partitioning import Partition
    root = Partition(np.arange(6), [3, 1, 2], [3, 1, 2])
    assert not root.is_partitioned() and not root.is_horizontally_partitioned() and root.get_vertical_split() == []
    sub = Partition([0, 2, 4], [3, 1, 2], [1], parent_partition=root)
    assert root.sub_partitions == [sub] and sub.parent_partition is root and root.is_horizontally_partitioned()
    cond, rest = sub.get_vertical_split()
    assert cond.tolist() == [3, 2] and rest.tolist() == [1]
    same = Partition(np.arange(6), [3], [], parent_partition=Partition(np.arange(6), [3, 1], [1]), is_naive=True)
    assert same.parent_partition.is_partitioned() and not same.parent_partition.is_horizontally_partitioned()
    data = np.arange(24).reshape(6, 4)
    assert np.array_equal(sub.get_slice(data), data[[0, 2, 4]][:, [3, 1, 2]])
    assert sub.disc_assignments is None and same.is_naive and not same.is_conj and sub.uncond_vars == [1]


def test_the_full_count_decides_a_split():
    """The host's choice from a histogram is the reference's variable-by-variable filter (tests/xpc_ref._horizontal)."""
    import itertools
    from deeprob.spn.utils.partitioning import _choose
    rs = np.random.RandomState(3)
    for trial in range(200):
        n, conj_len = int(rs.randint(8, 200)), int(rs.randint(1, 4))
        min_part_inst, arity = int(rs.randint(1, 30)), int(rs.randint(2, 6))
        data = (rs.rand(n, conj_len) < rs.rand()).astype(np.float32)
        if trial % 10 == 0:
            data[:] = data[0]
        assignments = [list(a) for a in itertools.product([0, 1], repeat=conj_len)]
        rs.shuffle(assignments)

        class Fixed:                        # hands the restatement the same order of assignments, draws nothing else
            def shuffle(self, x):
                x[:] = assignments
        node = xpc_ref._part(np.arange(n), range(conj_len), range(conj_len))
        want = xpc_ref._horizontal(data, node, min_part_inst, conj_len, arity, True, Fixed())
        codes = (data.astype(np.int64) << np.arange(conj_len)).sum(axis=1)
        hist = np.bincount(codes, minlength=1 << conj_len)
        got = _choose(hist, n, assignments, min_part_inst, arity) if n >= 2 * min_part_inst else None
        if want is None:
            assert got is None
            continue
        assert got is not None and len(got) == len(want[1]) - 1
        for code, rows in zip(got, want[1][1:]):
            assert np.array_equal(np.flatnonzero(codes == code), rows)


# ---- learn_estimator ---------------------------------------------------------------------------------------------------------------
def test_learn_estimator_routes_and_names_the_missing_keywords(monkeypatch):
    from deeprob.spn.learning import learn_estimator, xpc
    from deeprob.spn.structure.leaf import Bernoulli
    data = _data()
    dists, doms = [Bernoulli] * 8, [[0, 1]] * 8
    with pytest.raises(NotImplementedError) as e:
        learn_estimator(data, dists, doms, method='xpc', det=False, conj_len=2)
    assert all(k in str(e.value) for k in ('sd', 'min_part_inst', 'arity')) and 'conj_len' not in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        learn_estimator(data, dists, doms, method='ensemble-xpc', **GOOD)
    assert 'ensemble_dim' in str(e.value) and 'sd_level' in str(e.value)
    with pytest.raises(ValueError) as e:            # the reference's domain check comes first
        learn_estimator(data, dists, [[0, 1]] * 7 + [[0, 1, 2]], method='xpc')
    assert str(e.value) == "The domains must be binary for learning a XPC"
    with pytest.raises(ValueError) as e:
        learn_estimator(data, dists, [[0, 1]] * 7 + [[0, 1, 2]], method='ensemble-xpc')
    assert str(e.value) == "The domains must be binary for learning an Ensemble-XPC"
    calls = []
    monkeypatch.setattr(xpc, 'learn_xpc', lambda d, **kw: (calls.append(('xpc', d, kw)) or 'circuit', {}))
    monkeypatch.setattr(xpc, 'learn_expc', lambda d, **kw: (calls.append(('expc', d, kw)) or 'mixture', [{}]))
    assert learn_estimator(data, dists, doms, method='xpc', n_max_parts=9, **GOOD) == 'circuit'
    assert learn_estimator(data, dists, method='ensemble-xpc', ensemble_dim=3, det=True, sd_level=1, min_part_inst=4,
                           conj_len=2, arity=2) == 'mixture'
    assert [c[0] for c in calls] == ['xpc', 'expc'] and calls[0][1] is data and calls[0][2] == dict(GOOD, n_max_parts=9)
