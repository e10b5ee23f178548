"""Sampling and MPE of cutset networks without a device: the numpy restatement (tests/cnet_queries_ref.py) against
enumeration, the two ``dpc_cnq_*`` entries of the CLT header, and the argument handling of ``BinaryCNet.sample`` and of the
binding.

Statistical bounds: a frequency over n independent draws lies within 4 binomial standard errors of its probability
(sqrt(p (1 - p) / n)); the draws of different rows use different counters of the generator.  The prototype of these rules
at n = 20 000 and seed 2024 measured a largest deviation of 2.7 / 2.1 / 1.7 standard errors on the three patterns."""
import os
import re

import numpy as np
import pytest
import torch

from deeprob.hip import cnet
from tests import cnet_queries_ref as qref
from tests import cnet_ref as ref

# What every test here is about.  The restatement is held to enumeration because the device queries are held to the
# restatement (tests/test_cnet_queries_gpu.py): without them this module does not import.
SAMPLE, MPE = cnet.sample, cnet.mpe
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS_D5, N_DRAWS = qref.PATTERNS_D5, qref.N_DRAWS


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pattern', range(3))
def test_restated_sampler_draws_from_the_posterior_by_enumeration(pattern):
    model = ref.restated('d5')
    row = np.asarray(PATTERNS_D5[pattern], np.float32)
    x = np.tile(row, (N_DRAWS, 1))
    filled, leaf, near = qref.sample_replay(model, x, 2024)
    obs = ~np.isnan(row)
    assert np.array_equal(filled[:, obs], x[:, obs]) and set(np.unique(filled)) <= {0.0, 1.0}
    assert np.array_equal(leaf, ref.leaf_of_rows(model, filled))
    worst, outside = qref.deviations(model, row, filled)
    print('pattern %d: worst deviation %.2f s.e., mass outside the support %g, near %g' % (pattern, worst, outside, near.mean()))
    assert outside == 0.0 and worst <= 4.0


def test_restated_sampler_depends_on_seed_and_absolute_row_only():
    model = ref.restated('d10')
    q = ref.queries('d10')
    first, leaf, _ = qref.sample_replay(model, q, 11)
    again, _, _ = qref.sample_replay(model, q, 11)
    other, _, _ = qref.sample_replay(model, q, 12)
    assert first.tobytes() == again.tobytes() and first.tobytes() != other.tobytes()
    tail, tail_leaf, _ = qref.sample_replay(model, q[100:], 11, row0=100)
    assert tail.tobytes() == first[100:].tobytes() and np.array_equal(tail_leaf, leaf[100:])
    assert np.array_equal(first[1], q[1]) and leaf[1] == ref.leaf_of_rows(model, q[1:2])[0]        # the complete row


def test_restated_mpe_is_optimal_by_enumeration():
    model = ref.restated('d10')
    q = ref.queries('d10')
    filled, leaf = qref.mpe(model, q)
    obs = ~np.isnan(q)
    assert np.array_equal(filled[obs], q[obs]) and set(np.unique(filled)) <= {0.0, 1.0}
    assert np.array_equal(leaf, ref.leaf_of_rows(model, filled))
    best = ref._path_values(model, filled.astype(np.int64))
    every = qref.every_row(10)
    ll_every = ref._path_values(model, every)
    shortfall = 0.0
    for r, row in enumerate(q):
        agrees = (every[:, obs[r]] == row[obs[r]]).all(axis=1)
        shortfall = max(shortfall, float(ll_every[agrees].max() - best[r]))
    print('restated MPE on d10: largest shortfall against enumeration %.3g' % shortfall)
    assert shortfall <= 0.0


@pytest.mark.parametrize('name', ['d5', 'd10', 'd24', 'd33', 'd130'])
def test_few_draws_of_the_fixtures_lie_near_their_probability(name):
    _, _, near = qref.sample_replay(ref.restated(name), ref.queries(name), 11)
    assert near.mean() <= 0.02


# ---- the header --------------------------------------------------------------------------------------------------------------
def test_query_entries_parse_once_with_the_documented_arguments():
    from deeprob import hip
    from deeprob.hip import clt
    text = open(os.path.join(ROOT, 'include', 'deeprob_clt.h')).read()
    sigs, consts, structs = hip.parse_header(text, prefix='dpc', header='deeprob_clt.h')
    entries = sorted(s for s in sigs if s.startswith('dpc_cnq_'))
    assert entries == ['dpc_cnq_mpe', 'dpc_cnq_sample'] and not structs
    declared = re.findall(r'\b(dpc_cnq_\w+)\s*\(', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    assert sorted(declared) == entries
    for name in entries:
        assert clt.SIGNATURES[name] == sigs[name]
    assert len(sigs['dpc_cnq_mpe'][1]) == 18 and len(sigs['dpc_cnq_sample'][1]) == 20
    lib = clt.load_library()
    assert lib.dpc_abi_version() >= 2 and clt.ABI_VERSION == 2
    assert lib.dpc_cnq_mpe.argtypes == sigs['dpc_cnq_mpe'][1] and lib.dpc_cnq_sample.argtypes == sigs['dpc_cnq_sample'][1]


def test_an_older_library_is_refused_with_the_make_hint(monkeypatch):
    from deeprob.hip import HipError, clt
    monkeypatch.setattr(clt, '_lib', None)
    monkeypatch.setattr(clt, 'ABI_VERSION', clt.load_library().dpc_abi_version() + 1)
    monkeypatch.setattr(clt, '_lib', None)
    with pytest.raises(HipError) as e:
        clt.load_library()
    assert 'make -C deeprob-kit_amd/csrc' in str(e.value) and 'ABI version' in str(e.value)


# ---- the class and the binding -----------------------------------------------------------------------------------------------
def hand_built():
    """Column 0 cut at the root, a two-variable leaf over columns 1 and 2 on either side."""
    from deeprob.spn.structure.cltree import BinaryCLT
    from deeprob.spn.structure.cnet import BinaryCNet
    half = float(np.log(0.5))
    left, right = BinaryCNet([1, 2]), BinaryCNet([1, 2])
    for node in (left, right):
        node.clt = BinaryCLT([1, 2], tree=[-1, 0], params=[[[half, half]] * 2] * 2)
    return BinaryCNet([0, 1, 2], children=[left, right], weights=np.array([0.25, 0.75]), or_id=0)


def test_sample_argument_errors():
    from deeprob.hip import HipError
    from deeprob.spn.structure.cnet import BinaryCNet
    model = hand_built()
    assert callable(BinaryCNet.sample)
    with pytest.raises(HipError) as e:
        model.sample(torch.full((4, 3), float('nan')), seed=1)               # a CPU tensor
    assert 'make -C deeprob-kit_amd/csrc' in str(e.value)
    for bad in (np.zeros((4, 2), np.float32), np.zeros(3, np.float32), torch.zeros(4, 5), np.zeros((2, 3, 1), np.float32)):
        with pytest.raises(ValueError):
            model.sample(bad, seed=1)
    for unfitted in (BinaryCNet([0, 1, 2]), BinaryCNet([0, 1, 2], children=[BinaryCNet([1, 2])] * 2, weights=[0.5, 0.5], or_id=0)):
        with pytest.raises(ValueError) as e:
            unfitted.sample(np.zeros((4, 3), np.float32), seed=1)
        assert str(e.value) == "The CNet's structure and parameters must be already initialized"


def test_device_tables_carry_the_parents_and_the_query_scratch():
    from deeprob.hip import cnet
    tables = hand_built()._on_device('cpu')
    assert tables.node_parent.tolist() == [-1, 0, 1] and tables.node_parent.dtype == torch.int32
    assert (tables.levels, tables.max_leaf_d) == (2, 2)
    assert tables.row_bytes == 12 * 2 + 8 * 2 and tables.query_row_bytes == 16 * 2 + 8 * 2
    assert tables.node_col.tolist() == [0, -1, -1] and tables.node_child.tolist() == [1, 2, 0, -1, 1, -1]
    assert tables.leaf_meta.tolist() == [2, 0, 0, 2, 10, 8]
    # a deeper tree: 2 * parent + side, breadth first
    half = np.full((1, 2, 2), np.log(0.5), np.float32)
    leaf = lambda col: ([col], [0], [-1], half)                     # noqa: E731
    deep = cnet.DeviceCNet(3, [0, -1, 1, -1, -1], [[1, 2], [0, -1], [3, 4], [1, -1], [2, -1]], np.log(np.full((5, 2), 0.5)),
                           [leaf(1), leaf(2), leaf(2)], 'cpu')
    assert deep.node_parent.tolist() == [-1, 0, 1, 4, 5] and deep.levels == 3


@pytest.mark.parametrize('what', ['mpe', 'sample'])
def test_a_long_batch_goes_in_pieces_of_query_rows(what, monkeypatch):
    """The launches of a 2 100-row batch with 1024-row pieces, recorded in place of the library calls: the rows, the
    counter offset and the scratch of every piece."""
    from deeprob import hip
    from deeprob.hip import clt, cnet
    tables = hand_built()._on_device('cpu')
    calls = []
    monkeypatch.setattr(cnet, 'WORK_BYTES', 0)
    monkeypatch.setattr(hip, 'require_device_f32', lambda t, name: t)
    monkeypatch.setattr(hip, 'stream_ptr', lambda device: None)
    monkeypatch.setattr(clt, 'pack_query', lambda xs: torch.zeros((xs.shape[1], xs.shape[0]), dtype=torch.uint8))
    monkeypatch.setattr(cnet, 'call', lambda fn, *args: calls.append((fn.__name__, args)))
    assert cnet.query_rows(tables.query_row_bytes) == 1024
    x = torch.full((2100, 3), float('nan'))
    if what == 'mpe':
        out, choice = cnet.mpe(tables, x, return_choice=True)
    else:
        out, choice = cnet.sample(tables, x, 5, return_choice=True)
    assert out.shape == (2100, 3) and out.dtype == torch.float32 and choice.shape == (2100,) and choice.dtype == torch.int32
    assert [name for name, _ in calls] == ['dpc_cnq_' + what] * 3
    assert [args[2] for _, args in calls] == [1024, 1024, 52]
    assert [args[0] for _, args in calls] == [x.data_ptr() + 12 * r0 for r0 in (0, 1024, 2048)]
    assert [args[-3] for _, args in calls] == [out.data_ptr() + 12 * r0 for r0 in (0, 1024, 2048)]
    assert [args[-2] for _, args in calls] == [choice.data_ptr() + 4 * r0 for r0 in (0, 1024, 2048)]
    assert len({args[-4] for _, args in calls}) == 1                            # one scratch buffer, 1024 rows of it
    if what == 'sample':
        assert [(args[14], args[15]) for _, args in calls] == [(5, 0), (5, 1024), (5, 2048)]
    assert [len(args) for _, args in calls] == [18 if what == 'mpe' else 20] * 3
