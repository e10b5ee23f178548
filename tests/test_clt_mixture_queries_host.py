"""The posterior queries of a mixture of Chow-Liu trees without a device: the numpy restatement
(tests/clt_mixture_queries_ref.py) against enumeration of all 2^D rows, the header section and the binding of the three
``dpc_mixq_*`` entry points, the ABI gate, the argument errors (raised before any device work), and how many rows of the
device test's batches the replay of the sampler sets aside on its own.

Bar: 1e-12 between the float64 restatement and enumeration (both are float64 sums of at most 2^10 terms of size <= 1)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import clt_mixture_queries_ref as qref
from tests import clt_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(d, k) for d in (1, 2, 5, 10) for k in (1, 3)]


def rows_of(d):
    x = qref.batch(d, n=40, seed=3)
    x[2] = np.nan
    x[2, 0] = 1.0
    return x


def mixture(model):
    from deeprob.spn.structure import BinaryCLTMixture
    from deeprob.spn.structure.cltree import BinaryCLT
    trees, logw = model
    scope = list(range(len(trees[0][1])))
    w = np.exp(logw.astype(np.float64))
    return BinaryCLTMixture(scope, [BinaryCLT(scope, tree=t.copy(), params=p.copy()) for _, t, p in trees], w / w.sum())


# ---- the restatement against enumeration ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,k', SMALL)
def test_restated_marginals_equal_enumeration(d, k):
    model, x = qref.random_model(d, k), rows_of(d)
    got, want = qref.marginals(model, x), qref.marginals_by_enumeration(model, x)
    obs = ~np.isnan(x)
    assert np.array_equal(got[obs], x[obs].astype(np.float64)) and not np.isnan(got).any()
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize('d,k', SMALL)
def test_restated_component_posterior_equals_enumeration(d, k):
    model, x = qref.random_model(d, k), rows_of(d)
    pi = qref.posterior(model, x)
    for r in range(0, len(x), 5):
        assert np.abs(pi[r] - qref.joint_posterior(model, x[r]).sum(axis=1)).max() <= 1e-12
    assert np.abs(pi.sum(axis=1) - 1.0).max() <= 1e-12


@pytest.mark.parametrize('d,k', SMALL)
def test_restated_mpe_attains_the_enumerated_maximum(d, k):
    model, x = qref.random_model(d, k), rows_of(d)
    filled, comp = qref.mpe(model, x, np.float64)
    obs = ~np.isnan(x)
    assert np.array_equal(filled[obs], x[obs]) and set(np.unique(filled)) <= {0.0, 1.0} and comp.min() >= 0 and comp.max() < k
    assert np.abs(qref.log_joint(model, comp, filled) - qref.best_by_enumeration(model, x)).max() <= 1e-12


def test_restatement_on_a_zero_weight_and_on_impossible_rows():
    model, x = qref.zero_weight_model(), rows_of(10)
    assert np.abs(qref.marginals(model, x) - qref.marginals_by_enumeration(model, x)).max() <= 1e-12
    assert (qref.posterior(model, x)[:, 1] == 0).all()
    assert (qref.sample_replay(model, x, 5)[1] != 1).all() and (qref.mpe(model, x)[1] != 1).all()
    model, x = qref.impossible_model(), qref.impossible_rows()
    with np.errstate(invalid='ignore', divide='ignore'):
        got, want = qref.marginals(model, x), qref.marginals_by_enumeration(model, x)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isnan(got), np.isnan(x) & (np.arange(len(x)) < 2)[:, None])
    assert np.nanmax(np.abs(got - want)) <= 1e-12
    filled, comp, _ = qref.sample_replay(model, x, 9)
    assert comp.tolist()[:2] == [-1, -1] and comp[3] == 0 and comp[5] == -1 and comp[6] == 0
    assert np.array_equal(np.isnan(filled), np.isnan(got))
    filled, comp = qref.mpe(model, x)
    assert comp.tolist()[:2] == [-1, -1] and comp[5] == -1 and np.array_equal(np.isnan(filled), np.isnan(got))


def test_one_component_reduces_to_the_tree():
    """K = 1: pi = 1 exactly, the marginals are the tree's and the MPE is the tree's."""
    from tests import marginals_ref as mref
    model, x = qref.random_model(10, 1), rows_of(10)
    (bfs, tree, params), = model[0]
    assert (qref.posterior(model, x) == 1.0).all()
    for dtype in (np.float32, np.float64):
        assert np.array_equal(qref.marginals(model, x, dtype), mref.tree_marginals(bfs, tree, params, x, dtype).astype(np.float64))
    assert np.array_equal(qref.mpe(model, x)[0], clt_ref.mpe(bfs, tree, params, x))


def test_the_replay_sets_few_rows_aside_on_the_device_tests_batches():
    """A row holds at most 1 + 130 draws and each lies within NEAR = 1e-5 of its probability with a chance of 2e-5: about
    0.3 % of the rows at most, well inside the 2 % the device test allows."""
    for d, k in ((130, 3), (33, 2), (10, 64)):
        model = qref.random_model(d, k)
        x = np.concatenate([qref.batch(d, seed=s) for s in range(5)])
        filled, comp, near = qref.sample_replay(model, x, 2024)
        assert near.mean() <= 0.02
        assert not np.isnan(filled).any() and comp.min() >= 0 and comp.max() < k
        obs = ~np.isnan(x)
        assert np.array_equal(filled[obs], x[obs])
        again = qref.sample_replay(model, x[100:300], 2024, row0=100)
        assert np.array_equal(again[0], filled[100:300]) and np.array_equal(again[1], comp[100:300])


# ---- the header and the binding ------------------------------------------------------------------------------------------------
def test_header_declares_the_query_entry_points():
    from deeprob import hip
    from deeprob.hip import clt
    p, i64, i32, u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint64
    head = [p, p, i64, i32, i32] + [p] * 6
    want = {'dpc_mixq_marginals': head + [p, p, p], 'dpc_mixq_sample': head + [u64, i64, p, p, p, p],
            'dpc_mixq_mpe': head + [p, p, p, p]}
    text = open(os.path.join(ROOT, 'include', 'deeprob_clt.h')).read()
    sigs, consts, _ = hip.parse_header(text, prefix='dpc', header='deeprob_clt.h')
    lib = clt.load_library()
    for name, args in want.items():
        assert sigs[name] == clt.SIGNATURES[name] == (ctypes.c_int, args)
        assert getattr(lib, name).argtypes == args and text.count('int %s(' % name) == 1
    # the new section is the last one, after the dpc_mix_* entry points
    assert text.index('int dpc_mix_em_stats(') < text.index('Posterior queries of a mixture') < text.index('int dpc_mixq_marginals(')
    assert list(sigs)[-3:] == list(want)
    assert lib.dpc_abi_version() >= 6 == clt.MIXQ_ABI_VERSION and clt.MIX_ABI_VERSION == 5 and clt.ABI_VERSION == 2
    assert '16 * d + 8 * n_comp' in text and '8 * d + 8 * n_comp' in text


def test_an_older_library_asks_to_be_rebuilt(monkeypatch):
    from deeprob.hip import HipError, clt
    monkeypatch.setattr(clt, 'MIXQ_ABI_VERSION', clt.load_library().dpc_abi_version() + 1)
    with pytest.raises(HipError, match='rebuild'):
        clt._mixq_library()
    clt._mix_library()          # the gate of the dpc_mix_* entry points is its own


def test_entry_points_reject_what_the_header_excludes():
    from deeprob.hip import clt
    lib = clt.load_library()
    one = 8         # (no pointer is followed: every call is refused on its sizes, on a null pointer or on the alignment)

    def args(name, **kw):
        a = dict(x=one, codes=one, b=4, d=3, n_comp=2, bfs=one, parent=one, params=one, child_off=one, child_idx=one, logw=one,
                 seed=1, row0=0, work=one, out=one, component=one)
        a.update(kw)
        keys = ['x', 'codes', 'b', 'd', 'n_comp', 'bfs', 'parent', 'params', 'child_off', 'child_idx', 'logw']
        keys += {'dpc_mixq_marginals': ['work', 'out'], 'dpc_mixq_sample': ['seed', 'row0', 'work', 'out', 'component'],
                 'dpc_mixq_mpe': ['work', 'out', 'component']}[name]
        return [a[key] for key in keys] + [None]

    cases = [dict(d=0), dict(d=clt.DPC_MAX_D + 1), dict(n_comp=0), dict(n_comp=clt.DPC_MIX_MAX_K + 1), dict(b=-1), dict(b=2 ** 31),
             dict(x=None), dict(codes=None), dict(bfs=None), dict(parent=None), dict(params=None), dict(child_off=None),
             dict(child_idx=None), dict(logw=None), dict(work=None), dict(out=None), dict(work=12)]
    for name in ('dpc_mixq_marginals', 'dpc_mixq_sample', 'dpc_mixq_mpe'):
        for case in cases:
            assert getattr(lib, name)(*args(name, **case)) == clt.DPC_EINVAL and name.encode() in lib.dpc_last_error(), (name, case)
        assert getattr(lib, name)(*args(name, b=0)) == clt.DPC_OK                               # writes nothing
        assert getattr(lib, name)(*args(name, b=0, d=1, child_idx=None)) == clt.DPC_OK          # one variable: no children
    assert lib.dpc_mixq_sample(*args('dpc_mixq_sample', row0=-1)) == clt.DPC_EINVAL and b'row0' in lib.dpc_last_error()
    assert lib.dpc_mixq_sample(*args('dpc_mixq_sample', b=0, component=None)) == clt.DPC_OK


# ---- argument errors, before any device work -----------------------------------------------------------------------------------
def test_a_cpu_tensor_raises_hip_error_before_any_device_work(monkeypatch):
    from deeprob.hip import HipError, clt
    m = mixture(qref.random_model(5, 3))
    x = torch.from_numpy(rows_of(5))
    for name in ('pack_query', 'mixture_marginals', 'mixture_sample', 'mixture_mpe'):
        monkeypatch.setattr(clt, name, lambda *a, **k: pytest.fail('device work was started'))
    for query in (m.marginals, m.sample, m.mpe, lambda t: m.sample(t, seed=3, return_component=True),
                  lambda t: m.mpe(t, return_component=True)):
        with pytest.raises(HipError, match='no CPU fallback'):
            query(x)


def test_public_methods_check_the_model_and_the_shape(monkeypatch):
    from deeprob.spn.structure import BinaryCLTMixture
    for name in ('marginals', 'sample', 'mpe'):
        with pytest.raises(ValueError, match='must be already initialized'):
            getattr(BinaryCLTMixture([0, 1, 2]), name)(np.zeros((2, 3), np.float32))
    doc = __import__('deeprob.spn.structure.cltmix', fromlist=['x']).__doc__
    assert 'not the MAP' in doc and 'to_pc()' in doc and 'NP-hard' in BinaryCLTMixture.mpe.__doc__
