"""The histogram column splits (splitting/entropy.py, gini.py, gvs.py) without a device: the argument checks (all raised
before any device work), the numpy restatement of the device's edge and bin rule against ``np.histogram`` and
``np.histogram2d``, the host statistics against the clusters the reference recorded (tests/golden/learnspn_hist_*.npz,
written by tools/gen_golden_learnspn_hist.py), and the header entries."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
FUNCTIONS = ('entropy_cols', 'entropy_adaptive_cols', 'gini_cols', 'gini_adaptive_cols', 'gvs_cols', 'rgvs_cols')
ROW_SETS = ('all', 'a', 'b')

_cache = {}


def golden(kind):
    if kind not in _cache:
        g = np.load(os.path.join(GOLDEN, 'learnspn_hist_%s.npz' % kind))
        _cache[kind] = {k: g[k] for k in g.files}
    return _cache[kind]


def function(name):
    from deeprob.spn.learning import splitting
    return getattr(splitting, name)


def _cont(n=40, m=4):
    from deeprob.spn.structure.leaf import Gaussian
    return np.random.RandomState(0).randn(n, m).astype(np.float32), [Gaussian] * m, [(-5.0, 5.0)] * m


def _disc(n=40):
    from deeprob.spn.structure.leaf import Bernoulli, Categorical
    ks = [2, 3, 5, 2]
    data = np.random.RandomState(0).randint(0, ks, size=(n, len(ks))).astype(np.float32)
    return data, [Bernoulli if k == 2 else Categorical for k in ks], [list(range(k)) for k in ks]


# ---- arguments ----------------------------------------------------------------------------------------------------------------
def test_the_functions_are_exported_with_the_reference_defaults():
    import inspect
    from deeprob.spn.learning import splitting
    defaults = {name: {k: p.default for k, p in inspect.signature(getattr(splitting, name)).parameters.items()
                       if p.default is not inspect.Parameter.empty} for name in FUNCTIONS + ('gtest',)}
    assert defaults['entropy_cols'] == defaults['gini_cols'] == {'e': 0.3, 'alpha': 0.1}
    assert defaults['entropy_adaptive_cols'] == defaults['gini_adaptive_cols'] == {'e': 0.3, 'alpha': 0.1, 'size': None}
    assert defaults['gvs_cols'] == defaults['rgvs_cols'] == {'p': 5.0} and defaults['gtest'] == {'p': 5.0, 'test': True}
    for name in FUNCTIONS:
        assert list(inspect.signature(getattr(splitting, name)).parameters)[:4] == ['data', 'distributions', 'domains', 'random_state']
    assert not hasattr(splitting, 'wrgvs_cols')


@pytest.mark.parametrize('args', [_cont, _disc], ids=['gaussian', 'discrete'])
@pytest.mark.parametrize('name, message', [
    ('entropy_adaptive_cols', "Missing data size for Adaptive Entropy column splitting method"),
    ('gini_adaptive_cols', "Missing data size for Adaptive Gini column splitting method")])
def test_missing_size_raises_the_reference_message(name, message, args):
    from deeprob.spn.learning import learn_spn, learn_estimator
    data, dists, doms = args()
    for call in (lambda: function(name)(data, dists, doms, np.random.RandomState(0)),
                 lambda: learn_spn(data, dists, doms, split_rows='random', split_cols=function(name)),
                 lambda: learn_estimator(data, dists, doms, split_rows='random', split_cols=function(name),
                                         split_cols_kwargs={'e': 0.5})):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == message


@pytest.mark.parametrize('args', [_cont, _disc], ids=['gaussian', 'discrete'])
@pytest.mark.parametrize('name, bad', [('entropy_cols', {'p': 5.0}), ('entropy_cols', {'size': 10}), ('gini_cols', {'d': 0.3}),
                                       ('entropy_adaptive_cols', {'size': 10, 'k': 2}), ('gini_adaptive_cols', {'n': 2}),
                                       ('gvs_cols', {'e': 0.3}), ('rgvs_cols', {'alpha': 0.1})])
def test_unknown_keywords_raise_type_error(name, bad, args):
    from deeprob.spn.learning import learn_spn
    data, dists, doms = args()
    with pytest.raises(TypeError) as e:
        learn_spn(data, dists, doms, split_rows='random', split_cols=function(name), split_cols_kwargs=bad)
    assert name in str(e.value)
    with pytest.raises(TypeError):
        function(name)(data, dists, doms, np.random.RandomState(0), **bad)


@pytest.mark.parametrize('args', [_cont, _disc], ids=['gaussian', 'discrete'])
@pytest.mark.parametrize('name', ['ebvs', 'ebvs_ae', 'gbvs', 'gbvs_ag', 'wrgvs'])
def test_the_strings_still_raise(name, args):
    from deeprob.spn.learning import learn_spn
    data, dists, doms = args()
    with pytest.raises(NotImplementedError) as e:
        learn_spn(data, dists, doms, split_rows='random', split_cols=name)
    assert name in str(e.value)


@pytest.mark.parametrize('name', ['gvs', 'rgvs'])
def test_the_g_test_strings_still_raise_for_gaussian_columns(name):
    from deeprob.spn.learning import learn_spn
    data, dists, doms = _cont()
    with pytest.raises(NotImplementedError) as e:
        learn_spn(data, dists, doms, split_rows='random', split_cols=name)
    assert 'table' in str(e.value)


def test_a_wrapper_around_a_function_is_not_recognised():
    from deeprob.spn.learning import learn_spn, learnspn
    data, dists, doms = _cont()
    fn = function('entropy_cols')
    assert learnspn.hist_split(fn) == 'entropy_cols' and learnspn.hist_split('entropy_cols') is None
    assert learnspn.hist_split(function('gvs_cols')) == 'gvs' and learnspn.hist_split(function('gtest')) is None
    with pytest.raises(NotImplementedError):
        learn_spn(data, dists, doms, split_rows='random', split_cols=lambda *a, **k: fn(*a, **k))


def test_shape_errors_of_a_function_called_alone():
    data, dists, doms = _cont()
    for name in FUNCTIONS:
        kw = {'size': 40} if 'adaptive' in name else {}
        with pytest.raises(ValueError) as e:
            function(name)(data, dists, doms[:3], np.random.RandomState(0), **kw)
        assert str(e.value) == "Each data column should correspond to a random variable having a distribution and a domain"
        with pytest.raises(ValueError) as e:
            function(name)(data, dists, doms[:3] + [[0, 1]], np.random.RandomState(0), **kw)
        assert 'domain' in str(e.value)


# ---- numpy's bins restated -------------------------------------------------------------------------------------------------------
def columns():
    """Random, rounded, constant, two-valued, heavy-tailed, offset and one-row float32 columns."""
    rs = np.random.RandomState(3)
    cols = []
    for n in (1, 2, 3, 7, 64, 255, 256, 257, 1000, 5000):
        cols.append(rs.randn(n))
        cols.append(np.round(3.0 * rs.randn(n), 1))
        cols.append(np.round(rs.randn(n), 0))
        cols.append(1000.0 + 0.01 * rs.randn(n))
        cols.append(rs.randn(n) ** 3)
        cols.append(rs.rand(n) * 1e-3 - 7.0)
        cols.append(np.full(n, 2.5))
        cols.append(np.where(rs.rand(n) < 0.9, 0.0, 1.0))
    return [np.asarray(c, np.float32) for c in cols]


@pytest.mark.parametrize('rule', ['scott', 'fd'])
def test_restated_bins_equal_numpys_bit_for_bit(rule):
    """Edges and counts.  The bin COUNT is compared where the float64 quotient is clear of an integer (the margin the
    fixtures are held to); the edges and the counts are then compared for numpy's own number of bins."""
    from deeprob.spn.learning.splitting import hist as H
    compared = 0
    for col in columns():
        want_counts, want_edges = np.histogram(col, bins=rule)
        bins = len(want_counts)
        lo, hi, got_bins = H.column_bins(col, rule)
        width = (float(hi) - float(lo)) / got_bins if got_bins else 0.0
        if rule == 'scott':
            w = H.scott_width(len(col), float(np.var(col.astype(np.float64))))
        else:
            s = np.sort(col)
            (a0, a1, ta), (b0, b1, tb) = H.quartile_positions(len(col))
            w = H.fd_width(len(col), H.lerp(s[a0], s[a1], ta), H.lerp(s[b0], s[b1], tb))
        quotient = (float(hi) - float(lo)) / w if w else 0.5
        if abs(quotient - round(quotient)) >= 1e-3:
            assert got_bins == bins, (len(col), quotient, width)
            compared += 1
        edges = H.bin_edges(lo, hi, bins)
        assert edges.dtype == np.float32 == want_edges.dtype and np.array_equal(edges, want_edges)
        codes = H.bin_codes(col, lo, hi, bins)
        assert codes.min() >= 0 and codes.max() < bins
        assert np.array_equal(np.bincount(codes, minlength=bins), want_counts), (len(col), bins)
    assert compared >= 60


def test_restated_codes_give_histogram2d_on_fd_edges():
    from deeprob.spn.learning.splitting import hist as H
    cols = [c for c in columns() if len(c) == 1000]
    for x, y in zip(cols, cols[1:] + cols[:1]):
        b1, b2 = np.histogram_bin_edges(x, bins='fd'), np.histogram_bin_edges(y, bins='fd')
        want, _, _ = np.histogram2d(x, y, bins=[b1, b2])
        lo1, hi1 = H.outer_edges(x.min(), x.max())
        lo2, hi2 = H.outer_edges(y.min(), y.max())
        ca, cb = H.bin_codes(x, lo1, hi1, len(b1) - 1), H.bin_codes(y, lo2, hi2, len(b2) - 1)
        joint = np.zeros((len(b1) - 1, len(b2) - 1), np.int64)
        np.add.at(joint, (ca, cb), 1)
        assert np.array_equal(joint, want.astype(np.int64))


def test_values_on_edges_and_the_last_edge():
    from deeprob.spn.learning.splitting import hist as H
    edges = H.bin_edges(-1.0, 2.0, 7)
    x = np.concatenate([edges, np.nextafter(edges[1:], np.float32(-np.inf)), np.nextafter(edges[:-1], np.float32(np.inf))])
    codes = H.bin_codes(x, -1.0, 2.0, 7)
    assert np.array_equal(codes[:8], [0, 1, 2, 3, 4, 5, 6, 6])              # (x == hi falls in the last bin)
    assert np.array_equal(codes[8:15], [0, 1, 2, 3, 4, 5, 6]) and np.array_equal(codes[15:], [0, 1, 2, 3, 4, 5, 6])
    want, _ = np.histogram(x, bins=edges)
    assert np.array_equal(np.bincount(codes, minlength=7), want)
    assert np.array_equal(H.bin_codes(np.float32([4.0, 4.0]), *H.outer_edges(4.0, 4.0), 1), [0, 0])
    assert H.outer_edges(4.0, 4.0) == (np.float32(3.5), np.float32(4.5)) and H.bin_count(3.5, 4.5, 0.0) == 1


# ---- the host statistics against the reference's recorded clusters -----------------------------------------------------------------
@pytest.mark.parametrize('name', FUNCTIONS[:4])
def test_discrete_statistics_reproduce_the_recorded_clusters_from_counts(name):
    from deeprob.spn.learning.splitting import hist as H
    g = golden('disc')
    kw = dict(H.DEFAULTS[name], **json.loads(str(g['kwargs_json']))[name])
    ks = [int(k) for k in g['ks']]
    seen = set()
    for key in ROW_SETS:
        rows = g['data'][g['rows_' + key]]
        counts = [np.bincount(rows[:, i], minlength=k) for i, k in enumerate(ks)]
        got = H.stat_clusters(name, kw, counts, len(rows), False)
        assert got.dtype == np.int64 and np.array_equal(got, g['clusters_%s_%s' % (name, key)]), key
        seen |= set(got.tolist())
    assert seen == {0, 1}


@pytest.mark.parametrize('name', FUNCTIONS[:4])
def test_continuous_statistics_reproduce_the_recorded_clusters_from_restated_bins(name):
    from deeprob.spn.learning.splitting import hist as H
    g = golden('cont')
    kw = dict(H.DEFAULTS[name], **json.loads(str(g['kwargs_json']))[name])
    for key in ROW_SETS:
        rows = g['data'][g['rows_' + key]]
        hists = []
        for i in range(rows.shape[1]):
            lo, hi, bins = H.column_bins(rows[:, i], 'scott')
            assert bins == int(g['bins_scott_' + key][i])
            hists.append(np.bincount(H.bin_codes(rows[:, i], lo, hi, bins), minlength=bins))
        assert np.array_equal(H.stat_clusters(name, kw, hists, len(rows), True), g['clusters_%s_%s' % (name, key)]), key


def test_restated_g_is_the_reference_g_within_its_float32_rounding():
    """The reference sums its table in float32; 1e-3 relative is the margin its decisions are recorded with."""
    from deeprob.spn.learning.splitting import hist as H
    g = golden('cont')
    for key in ROW_SETS:
        rows = g['data'][g['rows_' + key]]
        binned = []
        for i in range(rows.shape[1]):
            lo, hi, bins = H.column_bins(rows[:, i], 'fd')
            assert bins == int(g['bins_fd_' + key][i])
            binned.append((H.bin_codes(rows[:, i], lo, hi, bins), bins))
        for i in range(rows.shape[1]):
            for j in range(i + 1, rows.shape[1]):
                joint = np.zeros((binned[i][1], binned[j][1]), np.int64)
                np.add.at(joint, (binned[i][0], binned[j][0]), 1)
                want = float(g['g_' + key][i, j])
                assert abs(H.g_of_table(joint, len(rows)) - want) <= 1e-3 * abs(want), (key, i, j)


def test_one_bin_gives_nan_entropy_and_cluster_zero():
    from deeprob.spn.learning.splitting import hist as H
    assert np.isnan(H.entropy_of(np.array([10]), 10, 0.1, True))
    assert H.stat_clusters('entropy_cols', {'e': 0.3, 'alpha': 0.1}, [np.array([10])], 10, True).tolist() == [0]
    assert H.threshold('gini_adaptive_cols', {'e': 0.3, 'size': 10 ** 12}, 10) == np.finfo(np.float32).eps


def test_the_fixtures_decide_something():
    for kind in ('cont', 'disc'):
        g = golden(kind)
        assert float(g['margin_stat']) >= 1e-6 and float(g['margin_g']) >= 1e-3
        for name in FUNCTIONS[:4]:
            assert set(g['clusters_%s_all' % name].tolist()) == {0, 1}
        for name in FUNCTIONS:
            graph = json.loads(str(g['spn_json_' + name]))
            cls = {int(n['id']): n['class'] for n in graph['nodes']}
            assert any(cls[int(e['target'])] == 'Product' and cls[int(e['source'])] != 'Gaussian' and
                       cls[int(e['source'])] in ('Sum', 'Product') for e in graph.get('links', graph.get('edges')))
    g = golden('cont')
    assert float(g['margin_bins']) >= 1e-3 and g['data'].dtype == np.float32 and g['data'].shape == (600, 6)
    p = json.loads(str(g['kwargs_json']))['gvs_cols']['p']
    ratio = g['g_all'] / (2.0 * p * np.outer(g['bins_fd_all'] - 1, g['bins_fd_all'] - 1))
    off = ratio[np.triu_indices(6, 1)]
    assert (off < 1).any() and (off > 1).any()                  # the continuous G-test comes out both ways


# ---- the header and the binding ---------------------------------------------------------------------------------------------------
def test_header_declares_the_new_entries_once_and_the_binding_parses_them():
    from deeprob import hip
    from deeprob.hip import learn
    text = open(os.path.join(ROOT, 'include', 'deeprob_learn.h')).read()
    declared = re.findall(r'\b(dpl_\w+)\s*\(', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    sigs, consts, _ = hip.parse_header(text, prefix='dpl', header='deeprob_learn.h')
    for name in ('dpl_hist_codes', 'dpl_code_counts', 'dpl_pair_g_codes'):
        assert declared.count(name) == 1 and name in sigs
    assert sigs == learn.SIGNATURES
    assert consts['DPL_HIST_MAX_BINS'] == 1024 == learn.DPL_HIST_MAX_BINS and consts['DPL_HIST_MAX_BINS'] <= 65536
    # the largest table, its marginals and the 256 partial sums fit the 64 KiB a work-group gets by default
    cells = consts['DPL_HIST_MAX_CELLS']
    marginals = max(a + cells // a for a in range(1, 1025) if cells // a <= 1024)
    assert 4 * cells + 8 * marginals + 8 * 256 <= 65536
    lib = learn.load_library()
    assert lib.dpl_abi_version() >= 5 and all(hasattr(lib, n) for n in ('dpl_hist_codes', 'dpl_code_counts', 'dpl_pair_g_codes'))


def test_over_cap_bins_raise_before_any_launch():
    from deeprob.hip import learn
    with pytest.raises(ValueError) as e:
        learn.check_bins([7, 3], [10, 1025])
    assert 'column 3' in str(e.value) and '1025' in str(e.value)
    with pytest.raises(ValueError) as e:
        learn.check_cells([2], [5], [1024], [13])
    assert 'columns 2 and 5' in str(e.value) and '1024 and 13' in str(e.value)
    learn.check_bins([0], [1024])
    learn.check_cells([0], [1], [1024], [12])
