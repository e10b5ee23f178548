"""MAF construction on the host: degrees, orderings, masks and state_dict layout against the reference's, and the
reference's ValueErrors (no GPU needed)."""
import os

import numpy as np
import pytest
import torch

from deeprob.flows.models import MAF
from deeprob.flows.layers.autoregressive import AutoregressiveLayer
from deeprob.torch.utils import MaskedLinear

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def structure():
    return np.load(os.path.join(GOLD, 'maf_structure.npz'))


def _check(tag, layer, g):
    np.testing.assert_array_equal(np.asarray(layer.ordering), g[tag + '.ordering'])
    np.testing.assert_array_equal(np.asarray(layer.inv_ordering), g[tag + '.inv_ordering'])
    for k, v in layer.state_dict().items():
        if k.endswith('mask'):
            np.testing.assert_array_equal(v.numpy(), g[tag + '.' + k])


def test_sequential_degrees_alternate(structure):
    torch.manual_seed(0)
    m = MAF(10, n_flows=3, units=8, depth=2)
    for i in range(3):
        _check('seq{}'.format(i), m.layers[2 * i], structure)
    assert not np.array_equal(m.layers[0].ordering, m.layers[2].ordering)


def test_random_degrees_random_state(structure):
    torch.manual_seed(0)
    m = MAF(12, n_flows=2, units=8, sequential=False, random_state=np.random.RandomState(42))
    for i in range(2):
        _check('rand{}'.format(i), m.layers[2 * i], structure)


def test_random_degrees_int_seed(structure):
    torch.manual_seed(0)
    m = MAF(12, n_flows=2, units=8, depth=2, sequential=False, random_state=7)
    for i in range(2):
        _check('seed{}'.format(i), m.layers[2 * i], structure)


def test_energy_two_variables(structure):
    torch.manual_seed(0)
    m = MAF(2, n_flows=10, units=128, batch_norm=False)
    assert len(m.layers) == 10
    for i in range(2):
        _check('energy{}'.format(i), m.layers[i], structure)


def test_state_dict_layout_and_initial_values(structure):
    torch.manual_seed(0)
    m = MAF(10, n_flows=2, units=8, depth=2)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in structure['sd_keys']]
    assert [','.join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in structure['sd_shapes']]
    # MaskedLinear is an nn.Linear: the same draws from torch's generator as the reference
    for k, v in sd.items():
        np.testing.assert_array_equal(v.numpy(), structure['sd.' + k])


def test_reference_state_dict_loads_strict(structure):
    m = MAF(10, n_flows=2, units=8, depth=2)
    sd = {k[3:]: torch.from_numpy(np.asarray(structure[k])) for k in structure.files if k.startswith('sd.')}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.layers[0].network[2].weight, sd['layers.0.network.2.weight'])
    assert 'layers.0.scale_act.weight' in sd


@pytest.mark.parametrize('kw', [dict(n_flows=0), dict(depth=0), dict(units=0)])
def test_maf_value_errors(kw):
    with pytest.raises(ValueError):
        MAF(8, **kw)


def test_layer_value_errors():
    with pytest.raises(ValueError):
        AutoregressiveLayer(8, 0, 8, 'relu')
    with pytest.raises(ValueError):
        AutoregressiveLayer(8, 1, 0, 'relu')
    with pytest.raises(ValueError):
        AutoregressiveLayer(8, 1, 8, 'relu', sequential=False, random_state=None)
    with pytest.raises(ValueError):
        AutoregressiveLayer(8, 1, 8, 'relu', sequential=False, random_state=3)
    with pytest.raises(ValueError):
        AutoregressiveLayer(8, 1, 8, 'gelu')
    with pytest.raises(ValueError):
        MAF(8, activation='swish')


def test_masked_linear():
    with pytest.raises(ValueError):
        MaskedLinear(4, 3, np.ones((4, 3)))
    torch.manual_seed(5)
    lin = MaskedLinear(4, 3, np.ones((3, 4)))
    torch.manual_seed(5)
    ref = torch.nn.Linear(4, 3)
    assert isinstance(lin, torch.nn.Linear)
    assert torch.equal(lin.weight, ref.weight) and torch.equal(lin.bias, ref.bias)
    assert lin.mask.dtype == torch.float32 and tuple(lin.mask.shape) == (3, 4)


def test_host_tensor_raises():
    from deeprob.hip import HipError
    m = MAF(6, n_flows=1, units=8)
    with pytest.raises(HipError):
        m(torch.randn(3, 6))
