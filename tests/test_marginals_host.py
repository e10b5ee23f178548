"""Posterior marginals of Chow-Liu trees and cutset networks without a device: the numpy restatement
(tests/marginals_ref.py) against enumeration of all 2^D rows, the two ``dpc_mar_*`` entries of the CLT header, the argument
handling of ``BinaryCLT.marginals`` / ``BinaryCNet.marginals``, the scratch of the binding and the coverage flag of
``DeviceCNet``.

The float64 restatement is held to enumeration at 1e-12, a round-off bound (1.5e-15 was measured); the device is held to
the float64 restatement in tests/test_marginals_gpu.py."""
import os
import re

import numpy as np
import pytest
import torch

from tests import clt_ref
from tests import cnet_ref
from tests import marginals_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['d10', 'd16'])
def test_restated_tree_marginals_equal_enumeration(name):
    g = clt_ref.golden(name)
    bfs, tree, params = clt_ref.restated(name)
    want = mref.tree_by_enumeration(tree, params, g['q'])
    got = mref.tree_marginals(bfs, tree, params, g['q'], np.float64)
    single = mref.tree_marginals(bfs, tree, params, g['q'], np.float32)
    obs = ~np.isnan(g['q'])
    assert np.array_equal(got[obs], g['q'][obs]) and not np.isnan(got).any() and got.min() >= 0.0 and got.max() <= 1.0
    print('tree %s: float64 %.3g, float32 %.3g from enumeration' % (name, np.abs(got - want).max(), np.abs(single - want).max()))
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize('name', ['d5', 'd10'])
def test_restated_network_marginals_equal_enumeration(name):
    model = cnet_ref.restated(name)
    q = cnet_ref.queries(name, n=128)
    want = mref.cnet_by_enumeration(model, q)
    got = mref.cnet_marginals(model, q, np.float64)
    single = mref.cnet_marginals(model, q, np.float32)
    obs = ~np.isnan(q)
    assert np.array_equal(got[obs], q[obs]) and not np.isnan(got).any() and got.min() >= 0.0 and got.max() <= 1.0
    assert np.array_equal(got[1], q[1]) and np.isnan(q[0]).all()
    print('network %s: float64 %.3g, float32 %.3g from enumeration' % (name, np.abs(got - want).max(),
                                                                        np.abs(single - want).max()))
    assert np.abs(got - want).max() <= 1e-12


def test_restated_marginals_of_a_deterministic_table():
    """x1 = x0 with certainty: evidence that agrees gives the enumerated values through ``-inf - (-inf)``, evidence that cannot
    happen gives NaN in exactly the unobserved entries."""
    bfs, tree, params, x = deterministic_chain()
    with np.errstate(divide='ignore'):
        want = mref.tree_by_enumeration(tree, params, x)
    for dtype in (np.float64, np.float32):
        got = mref.tree_marginals(bfs, tree, params, x, dtype)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.isnan(got).sum() == 1 and np.isnan(got[2, 2])
        assert np.nanmax(np.abs(got - want)) <= (1e-12 if dtype == np.float64 else 1e-6)


def deterministic_chain():
    """``(bfs, tree, params, rows)``: the chain 0 -> 1 -> 2 with x1 = x0 for certain."""
    with np.errstate(divide='ignore'):
        params = np.log(np.array([[[0.4, 0.6], [0.4, 0.6]], [[1.0, 0.0], [0.0, 1.0]], [[0.8, 0.2], [0.3, 0.7]]], np.float32))
    nan = np.nan
    x = np.array([[nan, 1, nan], [nan, nan, 1], [0, 1, nan], [1, nan, nan], [0, 1, 1], [nan, nan, nan]], np.float32)
    return np.array([0, 1, 2], np.int32), np.array([-1, 0, 1], np.int32), params, x


# ---- the header --------------------------------------------------------------------------------------------------------------
def test_marginal_entries_parse_once_with_the_documented_arguments():
    from deeprob import hip
    from deeprob.hip import clt
    text = open(os.path.join(ROOT, 'include', 'deeprob_clt.h')).read()
    sigs, consts, structs = hip.parse_header(text, prefix='dpc', header='deeprob_clt.h')
    entries = sorted(s for s in sigs if s.startswith('dpc_mar_'))
    assert entries == ['dpc_mar_clt', 'dpc_mar_cnet'] and not structs
    declared = re.findall(r'\b(dpc_mar_\w+)\s*\(', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    assert sorted(declared) == entries
    for name in entries:
        assert clt.SIGNATURES[name] == sigs[name]
    assert len(sigs['dpc_mar_clt'][1]) == 12 and len(sigs['dpc_mar_cnet'][1]) == 16
    lib = clt.load_library()
    assert lib.dpc_abi_version() >= 3 and clt.ABI_VERSION == 2
    assert lib.dpc_mar_clt.argtypes == sigs['dpc_mar_clt'][1] and lib.dpc_mar_cnet.argtypes == sigs['dpc_mar_cnet'][1]


# ---- the classes and the binding ---------------------------------------------------------------------------------------------
def hand_built():
    """Column 0 cut at the root, a two-variable leaf over columns 1 and 2 on either side."""
    from deeprob.spn.structure.cltree import BinaryCLT
    from deeprob.spn.structure.cnet import BinaryCNet
    half = float(np.log(0.5))
    left, right = BinaryCNet([1, 2]), BinaryCNet([1, 2])
    for node in (left, right):
        node.clt = BinaryCLT([1, 2], tree=[-1, 0], params=[[[half, half]] * 2] * 2)
    return BinaryCNet([0, 1, 2], children=[left, right], weights=np.array([0.25, 0.75]), or_id=0)


def test_marginals_argument_errors():
    from deeprob.hip import HipError
    from deeprob.spn.structure.cltree import BinaryCLT
    from deeprob.spn.structure.cnet import BinaryCNet
    half = float(np.log(0.5))
    tree = BinaryCLT([0, 1, 2], tree=[-1, 0, 0], params=[[[half, half]] * 2] * 3)
    for model in (hand_built(), tree):
        with pytest.raises(HipError) as e:
            model.marginals(torch.full((4, 3), float('nan')))               # a CPU tensor
        assert 'make -C deeprob-kit_amd/csrc' in str(e.value)
        for bad in (np.zeros((4, 2), np.float32), np.zeros(3, np.float32), torch.zeros(4, 5), np.zeros((2, 3, 1), np.float32)):
            with pytest.raises(ValueError):
                model.marginals(bad)
    for unfitted in (BinaryCNet([0, 1, 2]), BinaryCNet([0, 1, 2], children=[BinaryCNet([1, 2])] * 2, weights=[0.5, 0.5], or_id=0)):
        with pytest.raises(ValueError) as e:
            unfitted.marginals(np.zeros((4, 3), np.float32))
        assert str(e.value) == "The CNet's structure and parameters must be already initialized"
    for unfitted in (BinaryCLT([0, 1, 2]), BinaryCLT([0, 1, 2], tree=[-1, 0, 0])):
        with pytest.raises(ValueError) as e:
            unfitted.marginals(torch.zeros(4, 3))                           # reported before where the rows live
        assert str(e.value) == "The CLT's structure and parameters must be already initialized"
    assert not hasattr(BinaryCNet, 'mpe')


def test_device_tables_carry_the_scratch_of_the_marginals_and_the_coverage():
    from deeprob.hip import cnet
    tables = hand_built()._on_device('cpu')
    assert (tables.levels, tables.max_leaf_d, tables.d) == (2, 2, 3)
    assert tables.marginals_row_bytes == 20 * 2 + 8 * 2 + 8 * 3 and tables.covered is True
    assert tables.row_bytes == 12 * 2 + 8 * 2 and tables.query_row_bytes == 16 * 2 + 8 * 2            # as before
    half = np.full((1, 2, 2), np.log(0.5), np.float32)
    leaf = lambda col: ([col], [0], [-1], half)                     # noqa: E731
    logw = np.log(np.full((5, 2), 0.5))
    # the path through node 1 cuts column 0 and ends in a leaf over column 1: column 2 is left out
    holes = cnet.DeviceCNet(3, [0, -1, 1, -1, -1], [[1, 2], [0, -1], [3, 4], [1, -1], [2, -1]], logw,
                            [leaf(1), leaf(2), leaf(2)], 'cpu')
    assert holes.covered is False and holes.marginals_row_bytes == 20 * 3 + 8 * 1 + 8 * 3
    with pytest.raises(ValueError) as e:
        cnet.marginals(holes, torch.full((4, 3), float('nan')))              # before the device is looked at, before any launch
    assert 'column' in str(e.value)
    two = np.full((2, 2, 2), np.log(0.5), np.float32)
    whole = cnet.DeviceCNet(3, [0, -1, 1, -1, -1], [[1, 2], [0, -1], [3, 4], [1, -1], [2, -1]], logw,
                            [([1, 2], [0, 1], [-1, 0], two), leaf(2), leaf(2)], 'cpu')
    assert whole.covered is True
    lone = cnet.DeviceCNet(2, [-1], [[0, -1]], [[0.0, 0.0]], [([1], [0], [-1], half)], 'cpu')
    assert lone.covered is False


def _record(monkeypatch, module):
    from deeprob import hip
    from deeprob.hip import clt
    calls = []
    monkeypatch.setattr(hip, 'require_device_f32', lambda t, name: t)
    monkeypatch.setattr(hip, 'stream_ptr', lambda device: None)
    monkeypatch.setattr(clt, 'pack_query', lambda xs: torch.zeros((xs.shape[1], xs.shape[0]), dtype=torch.uint8))
    monkeypatch.setattr(module, 'call', lambda fn, *args: calls.append((fn.__name__, args)))
    return calls


def test_a_long_batch_of_a_network_goes_in_pieces_of_query_rows(monkeypatch):
    """The launches of a 2 100-row batch with 1024-row pieces, recorded in place of the library calls."""
    from deeprob.hip import cnet
    tables = hand_built()._on_device('cpu')
    assert cnet.query_rows(tables.marginals_row_bytes) == (1 << 27) // 80 // 64 * 64
    calls = _record(monkeypatch, cnet)
    monkeypatch.setattr(cnet, 'WORK_BYTES', 0)
    assert cnet.query_rows(tables.marginals_row_bytes) == 1024
    x = torch.full((2100, 3), float('nan'))
    out = cnet.marginals(tables, x)
    assert out.shape == (2100, 3) and out.dtype == torch.float32
    assert [name for name, _ in calls] == ['dpc_mar_cnet'] * 3 and [len(args) for _, args in calls] == [16] * 3
    assert [args[2] for _, args in calls] == [1024, 1024, 52]
    assert [args[0] for _, args in calls] == [x.data_ptr() + 12 * r0 for r0 in (0, 1024, 2048)]
    assert [args[-2] for _, args in calls] == [out.data_ptr() + 12 * r0 for r0 in (0, 1024, 2048)]
    assert len({args[-3] for _, args in calls}) == 1                            # one scratch buffer, 1024 rows of it
    assert [(args[11], args[12]) for _, args in calls] == [(2, 2)] * 3                   # levels, max_leaf_d


def test_a_long_batch_of_a_tree_goes_in_pieces_of_query_rows(monkeypatch):
    from deeprob.hip import clt
    half = np.full((3, 2, 2), np.log(0.5), np.float32)
    tree = clt.DeviceTree([0, 1, 2], [-1, 0, 0], half, 'cpu')
    assert clt.query_rows(3) == (1 << 25) // 6 // 64 * 64                       # 2 * D floats per row, as the other queries
    calls = _record(monkeypatch, clt)
    monkeypatch.setattr(clt, 'WORK_FLOATS', 0)
    assert clt.query_rows(3) == 1024
    x = torch.full((2100, 3), float('nan'))
    out = clt.marginals(tree, x)
    assert out.shape == (2100, 3) and out.dtype == torch.float32
    assert [name for name, _ in calls] == ['dpc_mar_clt'] * 3 and [len(args) for _, args in calls] == [12] * 3
    assert [args[2] for _, args in calls] == [1024, 1024, 52]
    assert [args[0] for _, args in calls] == [x.data_ptr() + 12 * r0 for r0 in (0, 1024, 2048)]
    assert [args[-2] for _, args in calls] == [out.data_ptr() + 12 * r0 for r0 in (0, 1024, 2048)]
    assert len({args[-3] for _, args in calls}) == 1
