"""Mixtures of Chow-Liu trees without a device: the header and the binding of the two ``dpc_mix_*`` entry points, the
argument errors (raised before any device work), the package's pure-numpy tied-CPT update and the float64 restatement of
batch EM (tests/clt_mixture_ref.py) against the reference's golden run (tools/gen_golden_clt_mixture.py), and the
derivation of the bound the device test holds the float32 mixing to.

Bars: after one iteration every probability within 1e-4 of the reference's; after 30 within max(1e-4, 4 dref), dref being
the distance between the reference's float32 run and its float64 restatement -- the bars tests/test_flat_spn_queries_gpu.py
holds EM to."""
import ctypes

import numpy as np
import pytest
import torch

from tests import clt_mixture_ref as mref
from tests import clt_ref

STEP, NUM_ITER = 0.5, 30


def given():
    """``(g, data, trees (bfs, tree), roots)`` of the golden."""
    g = mref.golden()
    data = clt_ref.unpack(g['data'], int(g['n_rows']), int(g['n_vars']))
    trees = [(clt_ref.bfs_order(t), t) for t in g['tree']]
    return g, data, trees, [int(r) for r in g['root']]


def mixture(g):
    from deeprob.spn.structure import BinaryCLTMixture
    from deeprob.spn.structure.cltree import BinaryCLT
    scope = list(range(int(g['n_vars'])))
    return BinaryCLTMixture(scope, [BinaryCLT(scope, tree=t.copy(), params=p.copy()) for t, p in zip(g['tree'], g['params'])],
                            g['weights'].copy())


# ---- the header and the binding ----------------------------------------------------------------------------------------------
def test_header_declares_the_mixture_entry_points():
    from deeprob.hip import clt
    p, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert clt.SIGNATURES['dpc_mix_log_likelihood'] == (ctypes.c_int, [p, i64, i32, p, i64, i32] + [p] * 11)
    assert clt.SIGNATURES['dpc_mix_em_stats'] == (ctypes.c_int, [p, i64, i32, p, i64, i32] + [p] * 5)
    assert clt.DPC_MIX_MAX_K >= 8 and clt.DPC_MIX_CHUNK % 256 == 0
    lib = clt.load_library()
    assert lib.dpc_abi_version() >= 5 == clt.MIX_ABI_VERSION and clt.ABI_VERSION == 2
    assert lib.dpc_mix_em_stats.argtypes == clt.SIGNATURES['dpc_mix_em_stats'][1]
    assert lib.dpc_mix_log_likelihood.argtypes == clt.SIGNATURES['dpc_mix_log_likelihood'][1]
    text = open(clt.HEADER_PATH).read()
    assert 'int dpc_mix_log_likelihood(' in text and 'int dpc_mix_em_stats(' in text


def test_an_older_library_asks_to_be_rebuilt(monkeypatch):
    from deeprob.hip import HipError, clt
    monkeypatch.setattr(clt, 'MIX_ABI_VERSION', clt.load_library().dpc_abi_version() + 1)
    with pytest.raises(HipError, match='rebuild'):
        clt._mix_library()


def test_entry_points_reject_what_the_header_excludes():
    from deeprob.hip import clt
    lib = clt.load_library()
    one = 8         # (no pointer is followed: every call is refused on its sizes or on a null pointer)
    assert lib.dpc_mix_log_likelihood(one, 4, 0, None, 4, 2, *[one] * 11) == clt.DPC_EINVAL and b'd = 0' in lib.dpc_last_error()
    assert lib.dpc_mix_log_likelihood(one, 4, 3, None, 4, clt.DPC_MIX_MAX_K + 1, *[one] * 11) == clt.DPC_EINVAL
    assert lib.dpc_mix_log_likelihood(one, 4, 3, None, 3, 2, *[one] * 11) == clt.DPC_EINVAL      # nb != b without rows
    assert lib.dpc_mix_log_likelihood(one, 4, 3, None, 4, 2, None, *[one] * 10) == clt.DPC_EINVAL
    assert lib.dpc_mix_em_stats(one, 4, 3, None, 4, 0, one, one, one, one, None) == clt.DPC_EINVAL
    assert lib.dpc_mix_em_stats(one, 4, 3, None, 4, 2, one, None, one, one, None) == clt.DPC_EINVAL
    assert lib.dpc_mix_em_stats(one, 4, 3, None, 4, 2, None, one, one, one, None) == clt.DPC_EINVAL


# ---- argument errors, before any device work -------------------------------------------------------------------------------------
def test_constructor_errors():
    from deeprob.spn.structure import BinaryCLTMixture
    from deeprob.spn.structure.cltree import BinaryCLT
    a, b = BinaryCLT([0, 1, 2]), BinaryCLT([0, 1, 3])
    with pytest.raises(ValueError, match='different scopes'):
        BinaryCLTMixture([0, 1, 2], [a, b], [0.5, 0.5])
    with pytest.raises(ValueError, match="sum up to 1"):
        BinaryCLTMixture([0, 1, 2], [a, BinaryCLT([0, 1, 2])], [0.5, 0.6])
    with pytest.raises(ValueError, match='length mismatch'):
        BinaryCLTMixture([0, 1, 2], [a], [0.5, 0.5])
    with pytest.raises(ValueError):
        BinaryCLTMixture([], None)
    m = BinaryCLTMixture([0, 1, 2], [a, BinaryCLT([0, 1, 2])], [0.25, 0.75])
    assert m.weights.dtype == np.float32 and m.scope == [0, 1, 2]


def test_em_argument_errors_come_before_any_device_work(monkeypatch):
    from deeprob.hip import clt
    from deeprob.spn.learning import expectation_maximization
    from deeprob.spn.structure import BinaryCLTMixture
    from deeprob.spn.structure.cltree import BinaryCLT
    monkeypatch.setattr(clt, 'load_library', lambda: pytest.fail('the library was asked for'))
    g, data, _, _ = given()
    m = mixture(g)
    for kw, text in ((dict(num_iter=0), 'number of iterations'), (dict(batch_perc=1.0), 'batch percentage'),
                     (dict(batch_perc=0.0), 'batch percentage'), (dict(step_size=0.0), 'step size'),
                     (dict(step_size=1.0), 'step size')):
        with pytest.raises(ValueError, match=text):
            m.em(data, **kw)
        with pytest.raises(ValueError, match=text):
            expectation_maximization(m, data, **kw)
    with pytest.raises(ValueError, match='must be already initialized'):
        BinaryCLTMixture(m.scope).em(data)
    with pytest.raises(ValueError, match='expected data'):
        m.em(data[:, :5])
    unset = BinaryCLT(m.scope)
    with pytest.raises(ValueError, match="The CLT's structure must be already initialized"):
        unset.em_init(np.random.RandomState(0))
    with pytest.raises(ValueError, match="The CLT's structure must be already initialized"):
        unset.em_step(np.ones(4, np.float32), data[:4], 0.5)
    with pytest.raises(ValueError, match='expected data'):
        m.components[0].em_step(np.ones(3, np.float32), data[:4], 0.5)


def test_a_cpu_tensor_raises_hip_error():
    from deeprob.hip import HipError
    g, data, _, _ = given()
    m = mixture(g)
    with pytest.raises(HipError):
        m.log_likelihood(torch.from_numpy(data))
    with pytest.raises(HipError):
        m.em(torch.from_numpy(data), num_iter=1, verbose=False)


def test_em_init_draws_as_the_reference():
    g, _, _, roots = given()
    m = mixture(g)
    rs, twin = np.random.RandomState(7), np.random.RandomState(7)
    m.components[1].em_init(rs)
    probs = twin.rand(len(m.scope), 2)
    probs[roots[1], 0] = probs[roots[1], 1]
    p = np.exp(m.components[1].params)
    assert m.components[1].params.dtype == np.float32 and np.allclose(p[:, :, 1], probs, atol=1e-6)
    assert np.allclose(p.sum(axis=2), 1.0, atol=1e-6) and np.array_equal(p[roots[1], 0], p[roots[1], 1])


# ---- the update and the loop against the reference's run ---------------------------------------------------------------------------
def test_update_function_reproduces_the_reference_em_step():
    from deeprob.spn.structure.cltree import em_update
    g, data, trees, roots = given()
    x = data[g['step_rows']]
    stats = mref.em_stats(x, g['step_stats'][:, None], [trees[0][1]])[0]
    got = em_update(g['params'][0], trees[0][1], roots[0], stats, STEP)
    assert got.dtype == np.float32
    assert np.max(np.abs(np.exp(got.astype(np.float64)) - np.exp(g['step_params'].astype(np.float64)))) <= 1e-4
    assert np.max(np.abs(np.exp(mref.tree_update(g['params'][0], trees[0][1], roots[0], stats, STEP)) -
                         np.exp(g['step_params'].astype(np.float64)))) <= 1e-4


@pytest.mark.parametrize('tag', ['cold', 'rand'])
@pytest.mark.parametrize('how', ['float64', 'package update'])
def test_restated_loop_reproduces_the_reference(tag, how):
    from deeprob.spn.structure.cltree import em_update
    g, data, trees, roots = given()
    dtype, update = (np.float64, None) if how == 'float64' else (np.float32, em_update)
    for iters, bars in ((1, (1e-4, 1e-4)), (NUM_ITER, [max(1e-4, 4.0 * float(d)) for d in g['dref_' + tag]])):
        init = np.random.RandomState(int(g['seed'])) if tag == 'rand' else None
        w, p, _ = mref.em_run(trees, roots, g['params'], g['weights'], data, g['index_' + tag][:iters], STEP, dtype, init, update)
        errs = mref.prob_err(w, p, g['%s%d.weights' % (tag, iters)], g['%s%d.params' % (tag, iters)])
        print('restated EM %s %s %d iterations: weights %.3e (bar %.1e) CPTs %.3e (bar %.1e)' % (how, tag, iters, errs[0],
                                                                                                 bars[0], errs[1], bars[1]))
        assert errs[0] <= bars[0] and errs[1] <= bars[1]
    gain = mref.mean_ll(trees, p, w, data) - float(g['ll_start'])
    ref_gain = float(g['ll_' + tag]) - float(g['ll_start'])
    assert ref_gain > 0 and gain >= 0.5 * ref_gain


def test_fixture_holds_what_the_tests_need():
    g, data, trees, roots = given()
    assert data.shape == (600, 16) and set(np.unique(data)) <= {0.0, 1.0}
    assert g['index_cold'].shape == g['index_rand'].shape == (NUM_ITER, 300)
    assert all(len(set(rows)) == 300 and 0 <= rows.min() and rows.max() < 600 for rows in g['index_rand'])
    for (bfs, tree), root in zip(trees, roots):
        assert tree[root] == -1 and (tree >= 0).sum() == 15 and bfs[0] == root
    assert np.allclose(np.exp(g['params']).sum(axis=3), 1.0, atol=1e-6) and abs(float(g['weights'].sum()) - 1.0) <= 1e-6
    assert abs(mref.mean_ll(trees, g['params'], g['weights'], data) - float(g['ll_start'])) <= 1e-4


# ---- the bound of the float32 mixing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 2, 3, 8])
def test_float32_mixing_stays_inside_its_bound(k):
    """|ll32 - ll64| <= 2^-23 (max_k |a_k| + K + 4) for the numpy float32 restatement in the device's order, over component
    values from tiny to -700 and weights that include -inf; the responsibilities of a row sum to 1 within K 2^-22."""
    rs = np.random.RandomState(k)
    comp = np.concatenate([-rs.rand(4000, k) * s for s in (1e-3, 1.0, 30.0, 700.0)]).astype(np.float32)
    comp[::7, 0] = comp[::7, -1]                        # ties
    logw = np.log(rs.dirichlet(np.ones(k))).astype(np.float32)
    for lw in (logw, np.where(np.arange(k) == 0, -np.inf, logw).astype(np.float32) if k > 1 else logw):
        ll32, resp32 = mref.mix(comp, lw, np.float32)
        ll64, _ = mref.mix(comp, lw)
        assert ll32.dtype == np.float32 and (np.abs(ll32.astype(np.float64) - ll64) <= mref.ll_bound(comp, lw)).all()
        assert (np.abs(resp32.astype(np.float64).sum(axis=1) - 1.0) <= k * 2.0 ** -22).all()
        assert (np.abs(resp32.astype(np.float64) - mref.mix(comp, lw)[1]) <= mref.resp_bound(comp, lw)[:, None]).all()
    dead_ll, dead_resp = mref.mix(np.full((3, k), -np.inf, np.float32), logw, np.float32)
    assert (dead_ll == -np.inf).all() and (dead_resp == 0).all()
