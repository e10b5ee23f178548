"""The histogram column splits on the HIP device: ``dpl_hist_codes``, ``dpl_code_counts`` and ``dpl_pair_g_codes`` alone
against numpy on poisoned, guard-banded outputs (codes and counts exactly equal, G against the float64 restatement in the
same order), the six functions alone and ``learn_spn`` end to end against what the reference recorded
(tests/golden/learnspn_hist_*.npz, tools/gen_golden_learnspn_hist.py)."""
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
FUNCTIONS = ('entropy_cols', 'entropy_adaptive_cols', 'gini_cols', 'gini_adaptive_cols', 'gvs_cols', 'rgvs_cols')
ROW_SETS = ('all', 'a', 'b')
#: the largest |difference| of a Gaussian leaf's mean or stddev from the reference's float32 np.mean / np.std that was
#: measured on the MI355X over the six continuous fixtures, and the bound asserted: ten times that
GAUSS_MEASURED = 4.8e-7
GAUSS_TOL = 10 * GAUSS_MEASURED

_cache = {}


def golden(kind):
    if kind not in _cache:
        g = np.load(os.path.join(GOLDEN, 'learnspn_hist_%s.npz' % kind))
        _cache[kind] = {k: g[k] for k in g.files}
    return _cache[kind]


def function(name):
    from deeprob.spn.learning import splitting
    return getattr(splitting, name)


def spec(kind):
    from deeprob.spn.structure.leaf import Bernoulli, Categorical, Gaussian
    g = golden(kind)
    if kind == 'cont':
        data = g['data']
        return data, [Gaussian] * data.shape[1], [(float(data[:, i].min()), float(data[:, i].max())) for i in range(data.shape[1])]
    ks = [int(k) for k in g['ks']]
    return g['data'].astype(np.float32), [Bernoulli if k == 2 else Categorical for k in ks], [list(range(k)) for k in ks]


def digraph(flat):
    from deeprob.spn.structure.io import spn_to_digraph
    return spn_to_digraph(flat)


def text_of(flat):
    from deeprob.spn.structure.io import save_spn_json
    buf = io.StringIO()
    save_spn_json(flat, buf)
    return buf.getvalue()


def learned(kind, name):
    """``(circuit, last_info())`` of ``learn_spn`` on a fixture with the fixture's settings (learned once)."""
    key = ('learned', kind, name)
    if key not in _cache:
        from deeprob.spn.learning import learn_spn, learnspn
        g = golden(kind)
        data, dists, doms = spec(kind)
        flat = learn_spn(data, dists, doms, learn_leaf='mle', split_rows='random', split_cols=function(name),
                         split_cols_kwargs=json.loads(str(g['learn_kwargs_json']))[name], min_rows_slice=int(g['min_rows_slice']),
                         random_state=int(g['seed']), verbose=False)
        _cache[key] = (flat, learnspn.last_info())
    return _cache[key]


# ---- the entries alone ---------------------------------------------------------------------------------------------------------
N_ROWS = 1100
SEGMENTS = (1, 2, 255, 256, 257, 1000)
#: column -> what it holds; the bins asked of every (segment, column): numpy's own count under both rules, and 1, 2, 17 and
#: the cap
COLUMNS = ('gaussian', 'rounded to one decimal', 'constant', 'offset by 1000', 'cubed', 'two values')
FIXED_BINS = (1, 2, 17, 1024)


def case():
    """(x float32 [N_ROWS, 6], device data, device row index, segments, offsets): every segment a scattered subset, every
    one but the first at a non-zero offset, sorted and unsorted alternately.  Built once and left unchanged."""
    if 'case' not in _cache:
        from deeprob.hip import learn as L
        rs = np.random.RandomState(9)
        x = np.stack([rs.randn(N_ROWS), np.round(3.0 * rs.randn(N_ROWS), 1), np.full(N_ROWS, 2.5), 1000.0 + 0.01 * rs.randn(N_ROWS),
                      rs.randn(N_ROWS) ** 3, np.where(rs.rand(N_ROWS) < 0.9, 0.0, 1.0)], axis=1).astype(np.float32)
        segs = [np.sort(rs.permutation(N_ROWS)[:n]) if i % 2 else rs.permutation(N_ROWS)[:n] for i, n in enumerate(SEGMENTS)]
        offs = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
        data = L.DeviceData(torch.from_numpy(np.ascontiguousarray(x.T)).cuda().reshape(-1), N_ROWS, x.shape[1])
        row_index = torch.from_numpy(np.concatenate(segs).astype(np.int32)).cuda()
        _cache['case'] = (x, data, row_index, segs, offs)
    return _cache['case']


def hist_items():
    """The items of the one launch: per (segment, column) numpy's 'scott' and 'fd' bins and the fixed bin counts; the
    expected codes from the numpy restatement and the expected counts from ``np.histogram`` itself."""
    if 'items' not in _cache:
        from deeprob.spn.learning.splitting import hist as H
        x, _, _, segs, offs = case()
        items = {k: [] for k in ('col', 'off', 'n', 'lo', 'hi', 'bins', 'codes', 'counts')}
        for s, rows in enumerate(segs):
            for c in range(x.shape[1]):
                v = x[rows, c]
                lo, hi = H.outer_edges(v.min(), v.max())
                for bins in [len(np.histogram(v, bins=rule)[0]) for rule in ('scott', 'fd')] + list(FIXED_BINS):
                    try:
                        want_counts, want_edges = np.histogram(v, bins=bins)
                    except ValueError:          # (numpy makes no 1024 bins in a span of fewer float32 numbers: no answer)
                        assert bins == 1024 and c == 3
                        continue
                    assert np.array_equal(want_edges, H.bin_edges(lo, hi, bins))
                    for k, val in zip(items, (c, offs[s], len(rows), lo, hi, bins, H.bin_codes(v, lo, hi, bins), want_counts)):
                        items[k].append(val)
        _cache['items'] = items
    return _cache['items']


@pytest.mark.parametrize('pattern', [0xFF, 0x7F])
def test_codes_and_counts_equal_numpys_exactly(pattern):
    """All items in one launch each: different n and bin counts side by side; values on edges (the rounded column), the
    maximum itself in every item (x == hi), constant columns (lo == hi) and n = 1."""
    from deeprob.hip import learn as L
    x, data, row_index, segs, _ = case()
    it = hist_items()
    assert {1, 2, 17, 1024} <= set(it['bins']) and set(it['n']) == set(SEGMENTS) and len(set(it['bins'])) > 8
    L.reset_counters()
    with contract(pattern, record=False) as c:
        c.frozen(data.x, row_index)
        codes, code_off = L.hist_codes(data, row_index, it['col'], it['off'], it['n'], it['lo'], it['hi'], it['bins'])
        counts, count_off = L.code_counts(codes, code_off, it['n'], it['bins'])
        c.expect_written(codes, counts)
        c.check()
    assert L.COUNTERS['kernels'] == 2 and L.COUNTERS['uploads'] == 2 and L.COUNTERS['reads'] == 0
    assert codes.dtype == torch.uint16 and counts.dtype == torch.int32
    assert list(code_off) == list(np.concatenate([[0], np.cumsum(it['n'])])[:-1])
    assert list(count_off) == list(np.concatenate([[0], np.cumsum(it['bins'])])[:-1])
    got_codes, got_counts = codes.cpu().numpy().astype(np.int64), counts.cpu().numpy()
    assert len(got_codes) == sum(it['n']) and len(got_counts) == sum(it['bins'])
    on_edge = 0
    for i in range(len(it['col'])):
        mine = got_codes[code_off[i]:code_off[i] + it['n'][i]]
        assert np.array_equal(mine, it['codes'][i]), (i, it['col'][i], it['n'][i], it['bins'][i])
        assert np.array_equal(got_counts[count_off[i]:count_off[i] + it['bins'][i]], it['counts'][i]), (i, it['bins'][i])
        if it['counts'][i].max() < it['n'][i] or it['bins'][i] == 1:   # (not a constant item, whose hi is max + 0.5)
            assert mine.max() == it['bins'][i] - 1                      # (the item's maximum: x == hi, the last bin)
    from deeprob.spn.learning.splitting import hist as H
    for i in range(len(it['col'])):
        if it['col'][i] == 1 and it['n'][i] >= 255:
            seg = segs[SEGMENTS.index(it['n'][i])]
            on_edge += int(np.isin(x[seg, 1], H.bin_edges(it['lo'][i], it['hi'][i], it['bins'][i])[1:-1]).sum())
    assert on_edge > 0, 'the rounded column puts values on inner edges'


#: (rows, bins of a, bins of b): 1 x 1, 1 x 7, 17 x 5, one larger than the 256 threads, non-square ones, two at the cell
#: cap (the widest and the squarest the caps admit), and n = 1
PAIR_TABLES = [(300, 1, 1), (257, 1, 7), (1000, 17, 5), (1000, 20, 30), (255, 7, 1), (1, 3, 4), (2, 2, 2), (1000, 1024, 12),
               (1000, 96, 128), (256, 80, 80)]


def pair_case():
    """Coded columns for PAIR_TABLES, one after the other in one uint16 array: dependent codes (b follows a), so the
    statistic is far from zero where the table allows it, with every bin's last code present."""
    if 'pairs' not in _cache:
        rs = np.random.RandomState(4)
        chunks, off_a, off_b, pos = [], [], [], 0
        for n, ba, bb in PAIR_TABLES:
            a = rs.randint(0, ba, size=n)
            b = np.where(rs.rand(n) < 0.5, (a * bb) // ba, rs.randint(0, bb, size=n))
            a[-1], b[-1] = ba - 1, bb - 1
            chunks += [a, b]
            off_a.append(pos)
            off_b.append(pos + n)
            pos += 2 * n
        _cache['pairs'] = (np.concatenate(chunks).astype(np.uint16), np.asarray(off_a), np.asarray(off_b))
    return _cache['pairs']


@pytest.mark.parametrize('pattern', [0xFF, 0x7F])
def test_pair_g_on_codes_against_the_restatement(pattern):
    from deeprob.hip import learn as L
    from deeprob.spn.learning.splitting import hist as H
    host, off_a, off_b = pair_case()
    assert max(ba * bb for _, ba, bb in PAIR_TABLES) == L.DPL_HIST_MAX_CELLS and any(ba * bb > 256 for _, ba, bb in PAIR_TABLES)
    codes = torch.from_numpy(host.view(np.int16)).cuda().view(torch.uint16)
    ns, bas, bbs = (np.asarray(v) for v in zip(*PAIR_TABLES))
    L.reset_counters()
    with contract(pattern, record=False) as c:
        c.frozen(codes)
        got = c.expect_written(L.pair_g_codes(codes, off_a, off_b, ns, bas, bbs))
        c.check()
    assert L.COUNTERS['kernels'] == 1 and L.COUNTERS['uploads'] == 1
    got = got.cpu().numpy()
    for q, (n, ba, bb) in enumerate(PAIR_TABLES):
        joint = np.zeros((ba, bb), np.int64)
        np.add.at(joint, (host[off_a[q]:off_a[q] + n].astype(np.int64), host[off_b[q]:off_b[q] + n].astype(np.int64)), 1)
        want = H.g_of_table(joint, n)
        err = abs(got[q] - want) / (abs(want) if want else 1.0)
        print('table', ba, 'x', bb, 'rows', n, 'g', got[q], 'restated', want, 'rel err', err)
        assert err <= 1e-12, (n, ba, bb)


def test_over_cap_bins_raise_before_any_launch():
    from deeprob.hip import learn as L
    from deeprob.spn.structure.leaf import Gaussian
    _, data, row_index, _, offs = case()
    L.reset_counters()
    with pytest.raises(ValueError) as e:
        L.hist_codes(data, row_index, [0, 4], [0, offs[5]], [1, 1000], [0.0, 0.0], [1.0, 1.0], [1, 1025])
    assert 'column 4' in str(e.value) and '1025' in str(e.value)
    codes = torch.zeros(64, dtype=torch.int16, device=data.device).view(torch.uint16)
    with pytest.raises(ValueError) as e:
        L.pair_g_codes(codes, [0], [32], [32], [1024], [13], [3], [5])
    assert 'columns 3 and 5' in str(e.value)
    with pytest.raises(ValueError):
        L.code_counts(codes, [0], [32], [1025])
    assert L.COUNTERS['kernels'] == 0 and L.COUNTERS['uploads'] == 0
    # a function alone: one far outlier gives the 'fd' rule tens of thousands of bins
    rs = np.random.RandomState(0)
    x = rs.randn(500, 3).astype(np.float32)
    x[17, 1] = 1.0e5
    with pytest.raises(ValueError) as e:
        function('gvs_cols')(x, [Gaussian] * 3, [(-1.0, 1.0)] * 3, np.random.RandomState(0))
    assert 'column 1' in str(e.value) and 'at most 1024' in str(e.value)


# ---- the functions alone, against the reference's recorded results ------------------------------------------------------------
@pytest.mark.parametrize('kind', ['cont', 'disc'])
@pytest.mark.parametrize('name', FUNCTIONS)
def test_functions_alone_give_the_recorded_clusters(name, kind):
    g = golden(kind)
    data, dists, doms = spec(kind)
    kw = json.loads(str(g['kwargs_json']))[name]
    for k, key in enumerate(ROW_SETS):
        got = function(name)(data[g['rows_' + key]], dists, doms, np.random.RandomState(int(g['seed']) + k), **kw)
        assert isinstance(got, np.ndarray) and got.dtype == np.int64
        assert np.array_equal(got, g['clusters_%s_%s' % (name, key)]), (key, got)


def test_discrete_g_functions_are_the_string_path():
    """``gvs_cols`` / ``rgvs_cols`` in ``learn_spn`` on discrete data: the circuit of the strings, byte for byte."""
    from deeprob.spn.learning import learn_spn
    g = golden('disc')
    data, dists, doms = spec('disc')
    for name in ('gvs', 'rgvs'):
        flat = learn_spn(data, dists, doms, split_rows='random', split_cols=name, min_rows_slice=int(g['min_rows_slice']),
                         random_state=int(g['seed']), verbose=False)
        assert text_of(flat) == text_of(learned('disc', name + '_cols')[0])


def test_gtest_alone_gives_the_recorded_values_and_decisions():
    g = golden('cont')
    data, dists, doms = spec('cont')
    p = json.loads(str(g['kwargs_json']))['gvs_cols']['p']
    worst = 0.0
    for key in ROW_SETS[:2]:
        rows = data[g['rows_' + key]]
        dof = np.outer(g['bins_fd_' + key] - 1, g['bins_fd_' + key] - 1)
        for i, j in ((0, 1), (0, 3), (2, 4), (4, 5), (5, 1)):
            value = function('gtest')(rows, i, j, dists, doms, p=p, test=False)
            want = float(g['g_' + key][i, j])
            worst = max(worst, abs(value - want) / abs(want))
            assert isinstance(value, float) and abs(value - want) <= 1e-3 * abs(want), (key, i, j, value, want)
            assert function('gtest')(rows, i, j, dists, doms, p=p) is bool(want < 2.0 * dof[i, j] * p)
    print('largest relative difference of G from the reference float32 value', worst)


def test_gtest_alone_on_discrete_columns_is_the_restated_g():
    g = golden('disc')
    data, dists, doms = spec('disc')
    ks = [int(k) for k in g['ks']]
    for i, j in ((0, 1), (2, 5), (9, 4)):
        want = ref.g_value(ref.joint_counts(g['data'][:, i], g['data'][:, j], ks[i], ks[j]), len(data))
        value = function('gtest')(data, i, j, dists, doms, test=False)
        assert abs(value - want) <= 1e-12 * abs(want), (i, j, value, want)
        assert function('gtest')(data, i, j, dists, doms) is bool(want < 2.0 * (ks[i] - 1) * (ks[j] - 1) * 5.0)


# ---- learn_spn end to end ----------------------------------------------------------------------------------------------------------
def leaf_differences(got, want, cls):
    """The largest |difference| of a parameter over the leaves of class ``cls`` of two node-link dicts of one structure."""
    gn = {int(r['id']): r for r in got['nodes']}
    worst = 0.0
    for w in want['nodes']:
        if w['class'] == cls:
            for key, val in w['params'].items():
                worst = max(worst, float(np.max(np.abs(np.asarray(gn[int(w['id'])]['params'][key], np.float64) - np.asarray(val, np.float64)))))
    return worst


@pytest.mark.parametrize('name', FUNCTIONS)
def test_learn_spn_gives_the_reference_circuit_on_continuous_data(name):
    """Clusters and graph exact (a wrong cluster anywhere changes the scopes); Sum weights within 1e-6 as in the discrete
    tests; Gaussian means and deviations within ten times the difference measured from the reference's float32 moments."""
    want = json.loads(str(golden('cont')['spn_json_' + name]))
    got = digraph(learned('cont', name)[0])
    assert ref.graphs_differ(got, want, atol=np.inf) is None                 # nodes, classes, scopes, edges
    worst = leaf_differences(got, want, 'Gaussian')
    print(name, 'largest |difference| of a Gaussian mean / stddev from the reference', worst)
    weights = {int(r['id']): r for r in got['nodes']}
    for w in want['nodes']:
        if w['class'] == 'Sum':
            assert np.max(np.abs(np.subtract(weights[int(w['id'])]['weights'], w['weights']))) <= 1e-6
    assert worst <= GAUSS_TOL
    assert ref.graphs_differ(got, want, atol=GAUSS_TOL) is None


@pytest.mark.parametrize('name', FUNCTIONS)
def test_learn_spn_gives_the_reference_circuit_on_discrete_data(name):
    want = json.loads(str(golden('disc')['spn_json_' + name]))
    assert ref.graphs_differ(digraph(learned('disc', name)[0]), want) is None         # (atol 1e-6: the discrete tests' tolerance)


def test_learn_estimator_passes_the_functions_through():
    from deeprob.spn.learning import learn_estimator
    from deeprob.spn.algorithms.structure import prune
    g = golden('cont')
    data, dists, doms = spec('cont')
    est = learn_estimator(data, dists, doms, learn_leaf='mle', split_rows='random', split_cols=function('gini_cols'),
                          split_cols_kwargs=json.loads(str(g['learn_kwargs_json']))['gini_cols'],
                          min_rows_slice=int(g['min_rows_slice']), random_state=int(g['seed']), verbose=False)
    from deeprob.spn.learning import learn_spn
    flat = learn_spn(data, dists, doms, learn_leaf='mle', split_rows='random', split_cols=function('gini_cols'),
                     split_cols_kwargs=json.loads(str(g['learn_kwargs_json']))['gini_cols'],
                     min_rows_slice=int(g['min_rows_slice']), random_state=int(g['seed']), verbose=False)
    assert text_of(est) == text_of(prune(flat, copy=False)) and est.n_nodes <= learned('cont', 'gini_cols')[0].n_nodes


def test_two_runs_are_byte_identical_and_a_device_tensor_gives_the_same_circuit():
    from deeprob.spn.learning import learn_spn
    g = golden('cont')
    data, dists, doms = spec('cont')
    for name in ('gvs_cols', 'entropy_cols'):
        flat = learn_spn(torch.from_numpy(data).cuda(), dists, doms, learn_leaf='mle', split_rows='random',
                         split_cols=function(name), split_cols_kwargs=json.loads(str(g['learn_kwargs_json']))[name],
                         min_rows_slice=int(g['min_rows_slice']), random_state=int(g['seed']), verbose=False)
        assert text_of(flat) == text_of(learned('cont', name)[0])


def per_generation(monkeypatch, **kw):
    """launches + reads + uploads of every generation of a ``learn_spn`` run: the counters at each call of the kind's
    ``column_stats``, which opens a generation."""
    from deeprob.hip import learn as L
    from deeprob.spn.learning import learn_spn, learnspn
    marks = []
    orig = learnspn.DiscreteColumns.column_stats

    def column_stats(self, *a):
        marks.append(L.COUNTERS['kernels'] + L.COUNTERS['reads'] + L.COUNTERS['uploads'])
        return orig(self, *a)
    monkeypatch.setattr(learnspn.DiscreteColumns, 'column_stats', column_stats)
    data, dists, doms = spec('disc')
    learn_spn(data, dists, doms, split_rows='random', min_rows_slice=64, random_state=int(golden('disc')['seed']), verbose=False, **kw)
    info = learnspn.last_info()
    marks.append(info['launches'])
    assert len(marks) == info['generations'] + 1 and marks[0] == 0
    return np.diff(marks), info


@pytest.mark.parametrize('name', FUNCTIONS[:4])
def test_discrete_statistics_add_no_launch_read_or_upload(name, monkeypatch):
    """On discrete data the histograms are the counts ``column_stats`` has read: a generation costs no more than the
    bound of DESIGN.md, and no more than a generation of the same data under ``split_cols='random'``."""
    from deeprob.spn.learning import learnspn
    g = golden('disc')
    mine, info = per_generation(monkeypatch, split_cols=function(name),
                                split_cols_kwargs=json.loads(str(g['learn_kwargs_json']))[name])
    plain, _ = per_generation(monkeypatch, split_cols='random')
    print(name, 'per generation', mine.tolist(), "under 'random'", plain.tolist())
    assert info['launches_per_generation'] == learnspn.LAUNCHES_PER_GENERATION == 14
    assert mine.max() <= learnspn.LAUNCHES_PER_GENERATION and mine.max() <= plain.max()
    assert info['launches'] <= info['generations'] * learnspn.LAUNCHES_PER_GENERATION
