"""The XPC learners on the device: ``dpc_xpc_code_counts`` and ``dpc_xpc_partition`` against integer numpy on poisoned,
guard-banded device memory (tests/buffer_contract.py, both patterns, byte for byte), and ``learn_xpc`` / ``learn_expc``
against the reference's fixtures (tests/golden/xpc_*.npz, tools/gen_golden_xpc.py) and the restatement
(tests/xpc_ref.py)."""
import numpy as np
import pytest
import torch

from tests import xpc_ref
from tests.buffer_contract import PATTERNS, contract

pytestmark = pytest.mark.gpu

LL_BAR = 1e-5               # the project's bar: |got - want| / max(1, |want|)


def _chunk():
    from deeprob.hip import clt
    return clt.DPC_XPC_CHUNK


# ---- the kernels -----------------------------------------------------------------------------------------------------------
def _segments(rs, n, layout):
    """Ascending, non-contiguous subsets of the rows 0 .. n-1 as the segments of the tasks."""
    def subset(k):
        return np.sort(rs.choice(n, size=k, replace=False))
    if layout == 'one':
        return [subset(max(1, (3 * n) // 4))] if n > 1 else [np.arange(1)]
    return [subset(n), np.zeros(0, np.int64), subset(max(1, n // 3))]


def _child_maps(rs, n_tasks, n_codes):
    """Random children, everything to one child, and one child left empty."""
    yield rs.randint(0, n_codes, size=(n_tasks, n_codes))
    yield np.full((n_tasks, n_codes), n_codes - 1)
    yield np.where(rs.rand(n_tasks, n_codes) < 0.5, 0, min(2, n_codes - 1))


def _codes(x, rows, cols):
    return sum(x[rows][:, c].astype(np.int64) << i for i, c in enumerate(cols))


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('layout', ['one', 'three'])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 'chunk-1', 'chunk+1', 4097])
def test_code_counts_and_partition(n, layout, pattern):
    from deeprob.hip import clt, xpc
    chunk = _chunk()
    n = {'chunk-1': chunk - 1, 'chunk+1': chunk + 1}.get(n, n)
    rs = np.random.RandomState(1000 * n + len(layout))
    for d in (1, 2, 33, 65):
        x = (rs.rand(n, d) < 0.5).astype(np.float32)
        planes = clt.pack_bits(torch.from_numpy(x).cuda())
        for conj_len in (1, 2, 3, clt.DPC_XPC_MAX_CONJ):
            n_codes = 1 << conj_len
            segs = _segments(rs, n, layout)
            sizes = [len(s) for s in segs]
            cols = rs.randint(0, d, size=(len(segs), conj_len))
            rows = torch.from_numpy(np.concatenate(segs).astype(np.int32)).cuda()
            want_hist = np.stack([np.bincount(_codes(x, s, c), minlength=n_codes) for s, c in zip(segs, cols)])
            for child_of_code in _child_maps(rs, len(segs), n_codes):
                with contract(pattern, record=False) as c:
                    c.frozen(planes, rows)
                    split = xpc.Split(planes, n, rows, sizes, cols)
                    hist = split.counts()
                    out = split.partition(child_of_code, want_hist)
                    c.expect_written(hist, split.chunk_hist, out)
                got_hist = hist.cpu().numpy()
                assert got_hist.dtype == np.int32 and np.array_equal(got_hist, want_hist), (d, conj_len)
                # the per-chunk histograms: each chunk's own rows, and they add up to the totals
                chunk_hist, at = split.chunk_hist.cpu().numpy(), 0
                for t, (s, cc) in enumerate(zip(segs, cols)):
                    for lo in range(0, len(s), chunk):
                        assert np.array_equal(chunk_hist[at], np.bincount(_codes(x, s[lo:lo + chunk], cc), minlength=n_codes))
                        at += 1
                    lo = split.chunk_off[t]
                    assert split.chunk_off[t + 1] == at
                    total = chunk_hist[lo:at].sum(axis=0) if at > lo else np.zeros(n_codes, np.int64)
                    assert np.array_equal(total, want_hist[t])
                # the split: task after task, child after child, every child's rows in their order (stable: ascending)
                want = []
                for s, cc, m in zip(segs, cols, child_of_code):
                    child = m[_codes(x, s, cc)] if len(s) else np.zeros(0, np.int64)
                    for k in range(n_codes):
                        piece = s[child == k]
                        assert (np.diff(piece) > 0).all()
                        want.append(piece)
                got = out.cpu().numpy()
                assert got.dtype == np.int32 and got.tobytes() == np.concatenate(want).astype(np.int32).tobytes(), (d, conj_len)


def test_entry_points_refuse_bad_arguments():
    from deeprob.hip import clt
    lib = clt.load_library()
    C = clt
    p = torch.zeros(64, dtype=torch.int64, device='cuda').data_ptr()
    ok = (p, 1, 64, 4, p, p, p, p)
    assert lib.dpc_xpc_code_counts(*ok, 0, 1, 0, p, p, None) == C.DPC_EINVAL and lib.dpc_last_error()
    assert lib.dpc_xpc_code_counts(*ok, C.DPC_XPC_MAX_CONJ + 1, 1, 0, p, p, None) == C.DPC_EINVAL
    assert lib.dpc_xpc_code_counts(p, 2, 64, 4, p, p, p, p, 1, 1, 0, p, p, None) == C.DPC_EINVAL       # n_words != (n + 63) / 64
    assert lib.dpc_xpc_code_counts(p, 1, 64, C.DPC_MAX_D + 1, p, p, p, p, 1, 1, 0, p, p, None) == C.DPC_EINVAL
    assert lib.dpc_xpc_code_counts(*ok, 1, 0, 0, p, p, None) == C.DPC_EINVAL
    assert lib.dpc_xpc_code_counts(*ok, 1, 1, 0, p, None, None) == C.DPC_EINVAL
    assert lib.dpc_xpc_partition(*ok, 0, p, p, p, 1, 0, p, None) == C.DPC_EINVAL
    assert lib.dpc_xpc_partition(*ok, 1, p, None, p, 1, 0, p, None) == C.DPC_EINVAL
    assert lib.dpc_xpc_partition(*ok, 1, None, p, p, 1, 1, p, None) == C.DPC_EINVAL                   # chunks without histograms


# ---- the learners ------------------------------------------------------------------------------------------------------------
_learned = {}


def _learn(name, data=None):
    from deeprob.spn.learning import learn_expc, learn_xpc
    learner, _, kw = xpc_ref.CONFIGS[name]
    data = xpc_ref.golden(name)['x'] if data is None else data
    if learner == 'xpc':
        return learn_xpc(data, **kw)
    np.random.seed(xpc_ref.GLOBAL_SEED)
    return learn_expc(data, **kw)


def learned(name):
    """``(circuit, [utils per member])`` of a fixture's data (numpy input); learned once."""
    if name not in _learned:
        circuit, utils = _learn(name)
        _learned[name] = (circuit, utils if isinstance(utils, list) else [utils])
    return _learned[name]


def _as_dicts(part):
    node = xpc_ref._part(part.row_ids, part.col_ids, part.uncond_vars, None, bool(part.is_naive), bool(part.is_conj))
    if part.disc_assignments is not None:
        node['disc'] = sorted(tuple(int(v) for v in a) for a in part.disc_assignments)
    node['subs'] = [_as_dicts(sub) for sub in part.sub_partitions]
    return node


def _circuit_bytes(circuit):
    names = ('order', 'kind', 'arg0', 'arg1', 'arg2', 'par0', 'par1', 'raw0', 'raw1', 'child_index', 'child_weight')
    return b''.join(np.ascontiguousarray(getattr(circuit, k)).tobytes() for k in names)


def _close(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape
    both_inf = np.isneginf(got) & np.isneginf(want)
    worst = float(np.max(np.where(both_inf, 0.0, np.abs(got - want) / np.maximum(1.0, np.abs(want)))))
    print('worst relative difference %.3g' % worst)
    return worst


@pytest.mark.parametrize('name', list(xpc_ref.CONFIGS))
def test_structure_agrees_with_the_reference(name):
    g = xpc_ref.golden(name)
    _, utils = learned(name)
    base = xpc_ref.restated(name)
    assert len(utils) == int(g['n_members'])
    for m, u in enumerate(utils):
        key = lambda k: g['m%d_%s' % (m, k)]
        got = xpc_ref.tree_record(_as_dicts(u['part_root']), int(g['n_rows']))
        for k, v in got.items():
            assert np.array_equal(v, key(k)), (m, k)
        assert u['n_parts'] == int(key('n_parts'))
        assert [[int(v) for v in c] for c in u['conj_vars_l']] == key('conj_vars').tolist()
        assert sorted(u) == ['cl_parts_l', 'conj_vars_l', 'n_parts', 'part_root', 'trees_dict']
        for part, node in zip(u['cl_parts_l'], base['members'][m]['cl_parts']):
            assert np.array_equal(part.row_ids, node['rows']) and part.col_ids.tolist() == node['cols']
            assert (np.diff(part.row_ids) > 0).all()
        xpc_ref.assert_trees(name, m, u['trees_dict'])


@pytest.mark.parametrize('name', list(xpc_ref.CONFIGS))
def test_log_likelihood_agrees_with_the_reference_and_the_restatement(name):
    from deeprob.spn.algorithms.inference import log_likelihood
    g = xpc_ref.golden(name)
    circuit, _ = learned(name)
    base = xpc_ref.restated(name)
    for rows, want in ((g['x'], g['ll_train']), (g['fresh'], g['ll_fresh']), (xpc_ref.queries(g['fresh']), g['ll_nan'])):
        got = log_likelihood(circuit, rows)
        assert _close(got, want) <= LL_BAR
        assert _close(got, xpc_ref.log_likelihood(base, rows)) <= LL_BAR


@pytest.mark.parametrize('name', list(xpc_ref.CONFIGS))
def test_sum_weights_add_to_one(name):
    circuit, _ = learned(name)
    sums = np.flatnonzero(circuit.kind == 0)
    assert len(sums)
    for i in sums:
        w = circuit.child_weight[circuit.arg0[i]:circuit.arg0[i] + circuit.arg1[i]].astype(np.float64)
        assert abs(w.sum() - 1.0) <= 1e-6 * len(w) and (w >= 0).all()


@pytest.mark.parametrize('name', ['a12', 'd40sd', 'g24e1'])
def test_device_tensor_input_and_poison_give_the_same_circuit(name):
    want = _circuit_bytes(learned(name)[0])
    x = torch.from_numpy(xpc_ref.golden(name)['x']).cuda()
    assert _circuit_bytes(_learn(name, x)[0]) == want
    for pattern in PATTERNS:
        with contract(pattern, record=False):
            circuit, _ = _learn(name)
        assert _circuit_bytes(circuit) == want


@pytest.mark.parametrize('name', ['b24det', 'g24e2'])
def test_mpe_and_sample_keep_the_observed_entries(name):
    from deeprob.spn.algorithms.inference import mpe
    from deeprob.spn.algorithms.sampling import sample
    circuit, _ = learned(name)
    q = xpc_ref.queries(xpc_ref.golden(name)['fresh'], n=64)
    seen = ~np.isnan(q)
    for out in (mpe(circuit, q), sample(circuit, q, seed=3)):
        assert out.shape == q.shape and np.isin(out, (0.0, 1.0)).all()
        assert np.array_equal(out[seen].view(np.uint32), q[seen].view(np.uint32))


def test_learn_estimator_routes_to_the_learners():
    from deeprob.spn.learning import learn_estimator
    from deeprob.spn.structure.leaf import Bernoulli
    g = xpc_ref.golden('a12')
    d = g['x'].shape[1]
    kw = xpc_ref.CONFIGS['a12'][2]
    circuit = learn_estimator(g['x'], [Bernoulli] * d, [[0, 1]] * d, method='xpc', **kw)
    assert _circuit_bytes(circuit) == _circuit_bytes(learned('a12')[0])
    np.random.seed(xpc_ref.GLOBAL_SEED)
    mixture = learn_estimator(g['x'], [Bernoulli] * d, method='ensemble-xpc', ensemble_dim=2, sd_level=1, **{
        k: v for k, v in kw.items() if k != 'sd'})
    assert mixture.classes[mixture.root] == 'Sum' and len(mixture.children[mixture.root]) == 2
