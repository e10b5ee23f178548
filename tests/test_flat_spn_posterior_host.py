"""Posterior queries on node-graph SPNs without a device: the header and the exports of libdeeprob_spnq.so, the struct
mirror, the leaf table, every argument error raised before anything reaches the device, ``likelihood``, and the float64
oracle the GPU tests compare against (tests/flat_spn_posterior_ref.py) against enumeration and against the reference's
goldens (tools/gen_golden_spn_moments.py)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import flat_spn_posterior_ref as pref
from tests.flat_spn_cases import random_circuit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


def _json(name):
    with open(os.path.join(GOLD, 'spn_%s.json' % name)) as f:
        return json.load(f)


def _load(name):
    from deeprob.spn.structure.io import load_spn_json
    return load_spn_json(os.path.join(GOLD, 'spn_%s.json' % name))


# ---- the header and the library --------------------------------------------------------------------------------------------
def test_spnq_header_parses_and_declares_its_entry_points_once():
    from deeprob import hip
    from deeprob.hip import spnq
    text = open(os.path.join(ROOT, 'include', 'deeprob_spnq.h')).read()
    sigs, consts, structs = hip.parse_header(text, prefix='dpq', header='deeprob_spnq.h')
    assert sigs == spnq.SIGNATURES and list(structs) == ['dpq_flat_spn_circuit']
    assert sorted(sigs) == ['dpq_abi_version', 'dpq_flat_spn_posterior', 'dpq_flat_spn_posterior_workspace_bytes',
                            'dpq_last_error']
    assert consts['DPQ_OK'] == 0 and consts['DPQ_EINVAL'] == -1 and consts['DPQ_EWORKSPACE'] == -2
    assert consts['DPQ_MODE_MOMENTS'] == 0 and consts['DPQ_MODE_VALUES'] == 1 and consts['DPQ_MAX_ORDERS'] == 4
    assert consts['DPQ_FLAG_FORCE_WORKSPACE'] == 1 and consts['DPQ_LDS_BUDGET_BYTES'] == 65536
    declared = re.findall(r'\b(dpq_\w+)\s*\(', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    assert sorted(declared) == sorted(set(declared)) == sorted(sigs), 'every entry point is declared once'
    assert len(sigs['dpq_flat_spn_posterior'][1]) == 17
    assert sigs['dpq_flat_spn_posterior_workspace_bytes'][0] is ctypes.c_int64


def test_spnq_entry_points_validate_before_any_device_work():
    from deeprob.hip import spnq
    lib = spnq.load_library()
    assert lib.dpq_abi_version() >= 1
    # argument validation happens before any device work
    assert lib.dpq_flat_spn_posterior_workspace_bytes(4, None, 0) == spnq.DPQ_EINVAL and b'bad sizes' in lib.dpq_last_error()
    assert lib.dpq_flat_spn_posterior(None, 4, 4, None, None, None, 1, 0, 1, 0, None, 0, None, 0, None, 0, None) == -1
    assert b'null circuit' in lib.dpq_last_error()


def test_missing_spnq_library_names_the_make_command(monkeypatch):
    from deeprob.hip import HipError, spnq
    monkeypatch.setattr(spnq, '_lib', None)
    monkeypatch.setattr(spnq, 'LIB_PATH', os.path.join(ROOT, 'no', 'such', 'libdeeprob_spnq.so'))
    with pytest.raises(HipError) as e:
        spnq.load_library()
    assert 'make -C deeprob-kit_amd/csrc' in str(e.value)


def test_circuit_record_mirrors_the_one_of_deeprob_hip():
    """The new header declares a layout-identical struct (the .hip file asserts it at compile time against the C
    declarations; this is the same statement about what the two bindings read)."""
    from deeprob import hip
    from deeprob.hip import spnq
    assert spnq.FlatSpnCircuit._fields_ == hip.FlatSpnCircuit._fields_
    assert ctypes.sizeof(spnq.FlatSpnCircuit) == ctypes.sizeof(hip.FlatSpnCircuit)
    for name, _ in hip.FlatSpnCircuit._fields_:
        assert getattr(spnq.FlatSpnCircuit, name).offset == getattr(hip.FlatSpnCircuit, name).offset, name
    src = open(os.path.join(ROOT, 'deeprob-kit_amd', 'csrc', 'spnq', 'flat_spn_posterior.hip')).read()
    for name, _ in hip.FlatSpnCircuit._fields_:
        assert 'DPQ_SAME_FIELD(%s)' % name in src, name
    assert 'sizeof(dpq_flat_spn_circuit) == sizeof(dpk_flat_spn_circuit)' in src


def test_on_chip_budget_holds_binary16_and_the_size_function_follows_the_header():
    from deeprob.hip import spnq
    lib = spnq.load_library()
    spn = _load('binary16')
    assert spn.n_nodes == 72 and spn.n_nodes * 512 <= spnq.DPQ_LDS_BUDGET_BYTES
    rec = spnq.FlatSpnCircuit(n_nodes=72)
    assert lib.dpq_flat_spn_posterior_workspace_bytes(1 << 20, ctypes.addressof(rec), 0) == 0
    forced = lib.dpq_flat_spn_posterior_workspace_bytes(100, ctypes.addressof(rec), spnq.DPQ_FLAG_FORCE_WORKSPACE)
    assert forced == 2 * ((72 * 100 * 4 + 255) // 256 * 256)
    rec = spnq.FlatSpnCircuit(n_nodes=129)
    assert lib.dpq_flat_spn_posterior_workspace_bytes(64, ctypes.addressof(rec), 0) == 2 * 129 * 64 * 4
    rec = spnq.FlatSpnCircuit(n_nodes=128)
    assert lib.dpq_flat_spn_posterior_workspace_bytes(64, ctypes.addressof(rec), 0) == 0


def test_leaf_table_lists_every_leaf_under_its_variable_in_increasing_id():
    from deeprob.hip import spnq
    from deeprob.spn.structure.io import digraph_to_spn
    for d in (_json('binary16'), _json('mixed4'), random_circuit(9, 2)[0]):
        spn = digraph_to_spn(d)
        ora = pref.Oracle(d)
        off, leaf = spnq.leaf_table(spn)
        assert off.dtype == np.int32 and leaf.dtype == np.int32 and off[0] == 0 and off[-1] == len(leaf)
        for j in range(spn.n_features):
            assert list(leaf[off[j]:off[j + 1]]) == ora.var_leaves.get(j, []), j


# ---- argument errors, none of which needs a device -----------------------------------------------------------------------------
def test_argument_errors_need_no_device():
    from deeprob.hip import HipError
    from deeprob.spn.algorithms import moments as mom
    from deeprob.spn.algorithms.inference import posterior, likelihood, posterior_values
    spn = _load('mixed4')
    x = np.full((3, 4), np.nan, np.float32)
    stats = (mom.expectation, mom.variance, mom.skewness, mom.kurtosis)
    for fn in stats + (lambda r, x=None: mom.moment(r, 2, x),):
        with pytest.raises(TypeError):
            fn(object(), x)
        with pytest.raises(TypeError):
            fn(object())
        with pytest.raises(ValueError):
            fn(spn, np.zeros((3, 2), np.float32))
        with pytest.raises(ValueError):
            fn(spn, np.zeros(4, np.float32))
        with pytest.raises(HipError):
            fn(spn, torch.zeros(3, 4))                       # a CPU tensor: no fallback
        out = fn(spn, np.zeros((0, 5), np.float32))          # B = 0: no launch, no device
        assert isinstance(out, np.ndarray) and out.shape == (0, 5) and out.dtype == np.float32
    with pytest.raises(ValueError, match='non-negative'):
        mom.moment(spn, -1)
    with pytest.raises(ValueError, match='non-negative'):
        mom.moment(spn, -1, x)
    with pytest.raises(NotImplementedError):
        mom.moment(spn, 5)
    ones = mom.moment(spn, 0)
    assert ones.dtype == np.float32 and np.array_equal(ones, np.ones(4, np.float32))
    assert np.array_equal(mom.moment(spn, 0, x), np.ones((3, 4), np.float32))
    assert np.array_equal(mom.moment(spn, 0, x.tolist()), np.ones((3, 4), np.float32))      # anything np.asarray takes
    with pytest.raises(HipError):
        mom.moment(spn, 0, torch.zeros(3, 4))

    with pytest.raises(TypeError):
        posterior(object(), x, 0)
    with pytest.raises(ValueError):
        posterior(spn, np.zeros((3, 2), np.float32), 0)
    with pytest.raises(HipError):
        posterior(spn, torch.zeros(3, 4), 0)
    families = [spn.classes[[i for i in range(spn.n_nodes) if spn.kind[i] >= 2 and spn.arg0[i] == v][0]] for v in range(4)]
    for v, f in enumerate(families):
        if f in ('Gaussian', 'Uniform'):
            with pytest.raises(ValueError, match='continuous'):
                posterior(spn, x, v)
        else:
            values = posterior_values(spn, v)
            assert values.dtype == np.float32 and list(values) == sorted(set(values))
            if f == 'Bernoulli':
                assert list(values) == [0.0, 1.0]
            out = posterior(spn, np.zeros((0, 4), np.float32), v)
            assert out.shape == (0, len(values)) and out.dtype == np.float32
            with pytest.raises(ValueError):
                posterior(spn, x, v, values=np.zeros((2, 2), np.float32))
            with pytest.raises(ValueError):
                posterior(spn, x, v, values=[])
            for bad in ([0.5], [0.0, 1.5], [np.nan], [np.inf]):
                with pytest.raises(ValueError, match='whole numbers'):
                    posterior(spn, x, v, values=bad)
            assert posterior_values(spn, v) is values           # kept per variable
    assert {'Gaussian', 'Bernoulli'} <= set(families) or {'Uniform', 'Categorical'} <= set(families)
    for bad in (-1, 4, 17):
        with pytest.raises(ValueError):
            posterior(spn, x, bad)
    with pytest.raises(TypeError):
        likelihood(object(), x)

    broken = _json('mixed4')
    sums = [n for n in broken['nodes'] if n['class'] == 'Sum']
    from deeprob.spn.structure.io import digraph_to_spn
    bad_spn = digraph_to_spn(broken)
    bad_spn.scopes[int(sums[0]['id'])] = [0, 1, 2, 3, 4]      # no longer smooth: check() runs first
    bad_spn._checked = False
    with pytest.raises(ValueError, match='smooth|decomposable'):
        mom.expectation(bad_spn, x)
    with pytest.raises(ValueError, match='smooth|decomposable'):
        posterior(bad_spn, x, 0)


def test_likelihood_is_exp_of_log_likelihood(monkeypatch):
    from deeprob.spn.algorithms import inference
    ll = np.array([-1.5, 0.0, -1e31], np.float32)
    table = np.stack([ll, ll - 1.0])
    seen = []

    def fake(root, x, return_results=False, n_jobs=0):
        seen.append((root, return_results, n_jobs))
        return (ll, table) if return_results else ll

    monkeypatch.setattr(inference, 'log_likelihood', fake)
    got = inference.likelihood('spn', 'x')
    assert got.dtype == np.float32 and np.array_equal(got, np.exp(ll)) and got[2] == 0.0
    a, b = inference.likelihood('spn', 'x', return_results=True, n_jobs=3)
    assert np.array_equal(a, np.exp(ll)) and np.array_equal(b, np.exp(table))
    assert seen == [('spn', False, 0), ('spn', True, 3)]
    monkeypatch.setattr(inference, 'log_likelihood', lambda *a, **k: torch.from_numpy(ll))
    t = inference.likelihood('spn', 'x')
    assert isinstance(t, torch.Tensor) and torch.equal(t, torch.exp(torch.from_numpy(ll)))


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def test_oracle_forward_is_the_reference_forward():
    """The oracle's plain forward against the reference's stored log-likelihoods (float32 tables: 1e-5)."""
    for circuit, vectors in (('binary16', 'binary16_nan'), ('mixed4', 'mixed4')):
        g = np.load(os.path.join(GOLD, 'spn_%s.npz' % vectors))
        ora = pref.Oracle(_json(circuit))
        got = ora.log_likelihood(g['x'])
        want = g['per_node'][0].astype(np.float64)
        live = want > -1e30
        assert np.array_equal(np.isfinite(got), live)
        assert np.max(np.abs(got[live] - want[live]) / np.maximum(1.0, np.abs(want[live]))) < 1e-5


@pytest.mark.parametrize('n_features,seed', [(6, 11), (8, 12)])
def test_oracle_against_enumeration(n_features, seed):
    d, _ = random_circuit(n_features, seed, kinds=('Bernoulli',))
    ora = pref.Oracle(d)
    rs = np.random.RandomState(seed)
    x = rs.randint(0, 2, (40, n_features)).astype(np.float32)
    x[rs.rand(*x.shape) < 0.6] = np.nan
    x[0] = np.nan
    want = pref.enumerate_binary(ora, x)
    got, scale = ora.moments(x, 4)
    nan = np.isnan(x)
    assert np.isfinite(got).all()
    for k in range(4):                                   # x^k = x for a binary variable
        assert np.max(np.abs(got[k] - want)) < 1e-12
        assert np.max(np.abs(scale[k] - want)) < 1e-12      # every leaf moment is non-negative
    assert np.array_equal(got[0][~nan], x[~nan].astype(np.float64))
    for var in (0, n_features - 1):
        p = ora.posterior(x, var, [0.0, 1.0])
        assert np.max(np.abs(p[:, 1] - want[:, var])) < 1e-12 and np.max(np.abs(p.sum(axis=1) - 1.0)) < 1e-12


def test_oracle_marks_zero_probability_evidence():
    d, family = random_circuit(5, 0)
    ora = pref.Oracle(d)
    x = np.full((2, 5), np.nan, np.float32)
    bounded = [v for v, f in enumerate(family) if f in ('Uniform', 'Categorical')]
    assert bounded
    x[1, bounded[0]] = 5.0 if family[bounded[0]] == 'Categorical' else 1e3
    got, _ = ora.moments(x, 2)
    others = [v for v in range(5) if v != bounded[0]]
    assert np.isfinite(got[:, 0]).all() and np.isnan(got[:, 1][:, others]).all()
    assert got[0, 1, bounded[0]] == x[1, bounded[0]]        # the observed entry is a point mass all the same


def test_oracle_against_the_reference_moments():
    """All-NaN rows: the oracle's conditional moments are the reference's unconditional ones (float32 results: 1e-6 of
    the scale), and variance / kurtosis formed from them the reference's."""
    g = np.load(os.path.join(GOLD, 'spn_moments.npz'))
    for name in ('binary16', 'mixed4'):
        ora = pref.Oracle(_json(name))
        x = np.full((1, ora.n_features), np.nan, np.float32)
        got, scale = ora.moments(x, 4)
        for k in range(4):
            want = g['%s.moment%d' % (name, k + 1)].astype(np.float64)
            assert np.max(np.abs(got[k, 0] - want) / np.maximum(1.0, scale[k, 0])) < 1e-6, (name, k)
        var, _, kurt = pref.statistics(got[:, 0])
        assert np.max(np.abs(var - g[name + '.variance']) / np.maximum(1.0, scale[1, 0])) < 1e-5
        assert np.max(np.abs(kurt - g[name + '.kurtosis']) / np.maximum(1.0, np.abs(kurt))) < 1e-3
