"""Host side of the node-graph SPN queries: EM initialisation and batch draws against the reference's, the JSON writer,
and the CPU restatement (tests/flat_spn_query_ref.py) pinned to the reference's goldens
(tools/gen_golden_spn_queries.py)."""
import io
import json
import os

import numpy as np
import pytest

from tests import flat_spn_query_ref as qref
from tests.flat_spn_cases import random_circuit
from tests.flat_spn_query_cases import support_inputs, RANDOM_CASES
from tests.util import rel_err, grad_err

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
FLOOR = np.float32(-1e31)


def _json(name):
    with open(os.path.join(GOLD, 'spn_%s.json' % name)) as f:
        return json.load(f)


def _load(name):
    from deeprob.spn.structure.io import load_spn_json
    return load_spn_json(os.path.join(GOLD, 'spn_%s.json' % name))


def eligible_rows(table):
    """(rows where every node value is above -1e3, floored rows, far-tail rows) of a [n_nodes, B] table, root = row 0."""
    floored = table[0] == FLOOR
    low = table.min(axis=0) < -1e3
    return ~low & ~floored, floored, low & ~floored


@pytest.mark.parametrize('name', ['binary16', 'mixed4'])
def test_em_init_and_batch_draws(name):
    from deeprob.spn.learning.em import draw_batches
    g = np.load(os.path.join(GOLD, 'spn_em_%s.npz' % name))
    spn = _load(name)
    rs = np.random.RandomState(42)
    spn.em_init(rs)
    got = qref.flat_params(spn)
    for k in qref.GROUPS:
        assert got[k].shape == g['init.' + k].shape
        assert np.allclose(got[k], g['init.' + k], rtol=1e-7, atol=0), k      # float32 weights, float64 leaves
    n = len(g['data'])
    assert np.array_equal(draw_batches(rs, n, int(0.5 * n), 30), g['index_rand'])
    assert np.array_equal(draw_batches(np.random.RandomState(42), n, int(0.5 * n), 30), g['index_cold'])
    # the derived arrays follow the new parameters
    assert np.allclose(np.exp(spn.child_logw), spn.child_weight, rtol=1e-6)
    assert np.allclose(np.exp(spn.cat_logp.astype(np.float64)), spn.probabilities, rtol=1e-6)
    # the helper draws the same
    st = qref.State(_json(name))
    qref.em_init(st, np.random.RandomState(42))
    for k, v in qref.params_of(st).items():
        assert np.allclose(v, g['init.' + k], rtol=1e-7, atol=0), k


def test_em_argument_errors():
    from deeprob.spn.learning import expectation_maximization
    spn = _load('binary16')
    data = np.zeros((10, 16), np.float32)
    for kw in (dict(num_iter=0), dict(batch_perc=0.0), dict(batch_perc=1.0), dict(step_size=0.0), dict(step_size=1.0)):
        with pytest.raises(ValueError):
            expectation_maximization(spn, data, **kw)


def test_uniform_leaf_not_implemented_and_untouched():
    from deeprob.spn.structure.io import digraph_to_spn
    from deeprob.spn.learning import expectation_maximization
    d, family = random_circuit(5, 0)
    assert 'Uniform' in family
    spn = digraph_to_spn(d)
    keep = {k: getattr(spn, k).copy() for k in ('child_weight', 'raw0', 'raw1', 'probabilities', 'par0', 'par1', 'cat_logp')}
    with pytest.raises(NotImplementedError):
        spn.em_init(np.random.RandomState(0))
    with pytest.raises(NotImplementedError):
        expectation_maximization(spn, np.zeros((10, 5), np.float32), num_iter=2, batch_perc=0.5, verbose=False)
    for k, v in keep.items():
        assert np.array_equal(getattr(spn, k), v), k


def _same_graph(a, b):
    key = lambda e: (e['source'], e['target'])
    ea, eb = a.get('links', a.get('edges')), b.get('links', b.get('edges'))
    return (sorted(a['nodes'], key=lambda n: n['id']) == sorted(b['nodes'], key=lambda n: n['id']) and
            sorted(ea, key=key) == sorted(eb, key=key))


@pytest.mark.parametrize('name', ['binary16', 'mixed4', 'binary16_em', 'mixed4_em'])
def test_save_spn_json_round_trip(name, tmp_path):
    from deeprob.spn.structure.io import load_spn_json, save_spn_json
    spn = _load(name)
    buf = io.StringIO()
    save_spn_json(spn, buf)
    assert _same_graph(json.loads(buf.getvalue()), _json(name))         # the reference's own export, reproduced
    path = str(tmp_path / 'again.json')
    save_spn_json(spn, path)
    again = load_spn_json(path)
    for k in ('order', 'kind', 'arg0', 'arg1', 'arg2', 'par0', 'par1', 'raw0', 'raw1', 'child_index', 'child_weight',
              'cat_value', 'cat_logp', 'probabilities', 'node_slot'):
        assert np.array_equal(getattr(again, k), getattr(spn, k)), k


def test_save_random_circuit_round_trip():
    from deeprob.spn.structure.io import digraph_to_spn, spn_to_digraph
    d, _ = random_circuit(7, 1)
    spn = digraph_to_spn(d)
    again = digraph_to_spn(spn_to_digraph(spn))
    for k in ('kind', 'child_index', 'child_weight', 'cat_value', 'cat_logp'):
        assert np.array_equal(getattr(again, k), getattr(spn, k)), k
    assert np.allclose(again.raw0, spn.raw0, atol=1e-8) and np.allclose(again.raw1, spn.raw1, atol=1e-8)


@pytest.mark.parametrize('circuit,vectors', [('binary16', 'binary16'), ('binary16', 'binary16_nan'), ('mixed4', 'mixed4')])
def test_helper_against_reference(circuit, vectors):
    """The restatement's node values, mpe and gradients are the reference's."""
    g = np.load(os.path.join(GOLD, 'spn_%s.npz' % vectors))
    q = np.load(os.path.join(GOLD, 'spn_queries_%s.npz' % vectors))
    st = qref.State(_json(circuit))
    lls = qref.forward(st, g['x'])
    assert rel_err(lls, g['per_node']) <= 1e-6
    filled, near = qref.mpe(st, g['x'], g['per_node'])
    assert near.mean() <= 0.01
    assert np.array_equal(filled[~near], q['mpe'][~near], equal_nan=True)
    rows = int(q['n_rows'])
    table = g['per_node'][:, :rows]
    grads = qref.backward(st, table)
    ok, floored, tail = eligible_rows(table)
    assert floored.mean() <= 0.05 and tail.mean() <= 0.01
    assert rel_err(grads[:, ok], q['grads'][:, ok]) <= 1e-5
    assert not np.isnan(grads).any()


@pytest.mark.parametrize('name', ['binary16', 'mixed4'])
@pytest.mark.parametrize('tag', ['cold', 'rand'])
def test_helper_em_step_against_reference(name, tag):
    g = np.load(os.path.join(GOLD, 'spn_em_%s.npz' % name))
    init = np.random.RandomState(42) if tag == 'rand' else None
    for dtype in (np.float32, np.float64):
        st = qref.em_run(_json(name), g['data'], g['index_' + tag][:1], 0.5, dtype, init and np.random.RandomState(42))
        for k, v in qref.params_of(st).items():
            assert grad_err(v, g['%s1.%s' % (tag, k)]) <= 1e-4 if len(v) else True, (k, dtype)


@pytest.mark.parametrize('n_features,seed,B', RANDOM_CASES)
def test_random_case_inputs_stay_inside_the_caps(n_features, seed, B):
    """Known before any GPU run: on the inputs of the GPU tests at most 1 % of the rows meet a near-tie and at most
    5 % sit on the floor (from the helper's values alone)."""
    d, family = random_circuit(n_features, seed)
    x = support_inputs(d, family, B, seed + 100)
    assert np.isnan(x[0]).all() and abs(np.isnan(x).mean() - 0.5) < 0.1 + 1.0 / B
    st = qref.State(d)
    lls = qref.forward(st, x)
    _, near = qref.mpe(st, x, lls)
    assert near.sum() <= 0.01 * B, near.mean()
    assert (lls[0] == FLOOR).sum() <= 0.05 * B
