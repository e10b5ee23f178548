"""Golden vectors for the masked autoregressive flow (MAF).  Needs the reference on PYTHONPATH:

    PYTHONPATH=/root/reference python3 tools/gen_golden_maf.py

Every fixture is data only: seeded inputs, degrees / masks, and what the reference computes on the CPU in fp32 and,
for the same model converted to float64, in float64.  Models with more than a few thousand weights are rebuilt by the
tests from the seeds (torch.manual_seed, then tests/util.randomise_flow) instead of shipping their weights.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import _np, _save          # noqa: E402
from gen_golden_flows import _randomise_flow   # noqa: E402

# name -> (constructor kwargs, in_features, torch seed, perturbation seed, rows)
CASES = {
    'maf192_bn': (dict(), 192, 3, 4, 32),
    'maf192_nobn': (dict(batch_norm=False), 192, 3, 4, 32),
    'maf192_rand8': (dict(sequential=False, units=8, random_state=42), 192, 3, 4, 32),
    'maf192_logit': (dict(logit=0.01), 192, 3, 4, 32),
    'maf784_seq': (dict(), 784, 10, 11, 16),
    'maf784_rand': (dict(sequential=False, random_state=42), 784, 10, 11, 16),
    'maf2_energy': (dict(n_flows=10, batch_norm=False), 2, 5, 6, 64),
    'maf20_depth2': (dict(depth=2, units=48, n_flows=3), 20, 7, 8, 24),
    'maf20_depth3': (dict(depth=3, units=40, n_flows=2, activation='tanh'), 20, 7, 8, 24),
    'maf33_leaky': (dict(activation='leaky-relu', units=40, n_flows=2), 33, 9, 1, 24),
    'maf33_softplus': (dict(activation='softplus', units=40, n_flows=2), 33, 9, 1, 24),
    'maf33_tanh': (dict(activation='tanh', units=40, n_flows=2), 33, 9, 1, 24),
    'maf33_sigmoid': (dict(activation='sigmoid', units=40, n_flows=2), 33, 9, 1, 24),
    'maf33_relu_u70': (dict(units=70, n_flows=2), 33, 9, 1, 24),
    'maf12_units200': (dict(units=200, n_flows=2), 12, 2, 3, 24),
}


def _x(D, rows, logit):
    g = torch.Generator().manual_seed(123)
    return torch.rand(rows, D, generator=g) * 0.98 + 0.01 if logit else torch.randn(rows, D, generator=g)


def _eval_arrays(model, x):
    out = {}
    with torch.no_grad():
        out['ll'] = _np(model(x))
        u, ildj = model.apply_backward(x if model.logit is None else model.preprocess(x)[0])
        out['u'], out['ildj'] = _np(u), _np(ildj)
        xr, ldj = model.apply_forward(u)
        out['x_rec'], out['ldj'] = _np(xr), _np(ldj)
        h = x if model.logit is None else model.preprocess(x)[0]
        for i, layer in enumerate(model.layers):
            h, d = layer.apply_backward(h)
            if i < 2:
                out['layer{}.u'.format(i)] = _np(h)
                out['layer{}.ildj'.format(i)] = _np(d)
    return out


def gen_eval():
    from deeprob.flows.models.maf import MAF
    for name, (kw, D, seed, pseed, rows) in CASES.items():
        torch.manual_seed(seed)
        m = MAF(D, **kw)
        _randomise_flow(m, pseed)
        m.eval()
        x = _x(D, rows, kw.get('logit') is not None)
        arrays = {'x': _np(x)}
        arrays.update(_eval_arrays(m, x))
        m64 = m.double()
        with torch.no_grad():
            arrays['ll64'] = m64(x.double()).numpy().copy()
        _save('maf_' + name, **arrays)


def gen_structure():
    """Degrees, orderings, masks and state_dict layout of small layers / flows."""
    from deeprob.flows.models.maf import MAF
    from deeprob.flows.layers.autoregressive import AutoregressiveLayer
    arrays = {}

    def put(tag, layer):
        arrays[tag + '.ordering'] = np.asarray(layer.ordering)
        arrays[tag + '.inv_ordering'] = np.asarray(layer.inv_ordering)
        for k, v in layer.state_dict().items():
            if k.endswith('mask'):
                arrays[tag + '.' + k] = _np(v)

    torch.manual_seed(0)
    m = MAF(10, n_flows=3, units=8, depth=2)
    for i in range(3):
        put('seq{}'.format(i), m.layers[2 * i])
    torch.manual_seed(0)
    m = MAF(12, n_flows=2, units=8, sequential=False, random_state=np.random.RandomState(42))
    for i in range(2):
        put('rand{}'.format(i), m.layers[2 * i])
    torch.manual_seed(0)
    m = MAF(12, n_flows=2, units=8, depth=2, sequential=False, random_state=7)
    for i in range(2):
        put('seed{}'.format(i), m.layers[2 * i])
    torch.manual_seed(0)
    m = MAF(2, n_flows=10, units=128, batch_norm=False)
    for i in range(2):
        put('energy{}'.format(i), m.layers[i])
    torch.manual_seed(0)
    m = MAF(10, n_flows=2, units=8, depth=2)
    sd = m.state_dict()
    arrays['sd_keys'] = np.array(list(sd.keys()))
    arrays['sd_shapes'] = np.array([','.join(str(s) for s in v.shape) for v in sd.values()])
    for k, v in sd.items():
        arrays['sd.' + k] = _np(v)
    _save('maf_structure', **arrays)
    del AutoregressiveLayer


def gen_train():
    """One density-direction training step (train- and eval-mode batch norm) and rsample gradients."""
    from deeprob.flows.models.maf import MAF
    from deeprob.flows.layers.autoregressive import AutoregressiveLayer
    for tag, kw, train in [('d1_train', dict(n_flows=2, units=24, activation='tanh'), True),
                           ('d2_train', dict(n_flows=2, units=24, depth=2, activation='tanh'), True),
                           ('d1_eval', dict(n_flows=2, units=24, activation='tanh'), False)]:
        torch.manual_seed(21)
        m = MAF(10, **kw)
        _randomise_flow(m, 22)
        arrays = {'sd.' + k: _np(v) for k, v in m.state_dict().items()}
        m.train(train)
        x = torch.randn(48, 10, generator=torch.Generator().manual_seed(23)).requires_grad_(True)
        loss = -m(x).mean()
        loss.backward()
        arrays['x'] = _np(x)
        arrays['loss'] = _np(loss.reshape(1))
        arrays['grad.x'] = _np(x.grad)
        for k, p in m.named_parameters():
            if p.grad is not None:
                arrays['grad.' + k] = _np(p.grad)
        for k, b in m.named_buffers():
            if 'running' in k:
                arrays['after.' + k] = _np(b)
        _save('maf_train_' + tag, **arrays)
    # apply_forward under autograd (what rsample differentiates)
    torch.manual_seed(31)
    layer = AutoregressiveLayer(6, 1, 16, 'tanh', reverse=True)
    with torch.no_grad():
        for k, p in layer.named_parameters():
            p.add_(0.3 * torch.randn(p.shape, generator=torch.Generator().manual_seed(32 + len(k))))
    arrays = {'sd.' + k: _np(v) for k, v in layer.state_dict().items()}
    u = torch.randn(9, 6, generator=torch.Generator().manual_seed(33)).requires_grad_(True)
    x, ldj = layer.apply_forward(u)
    (x.square().sum() + 0.5 * ldj.sum()).backward()
    arrays.update({'u': _np(u), 'x': _np(x), 'ldj': _np(ldj), 'grad.u': _np(u.grad)})
    for k, p in layer.named_parameters():
        arrays['grad.' + k] = _np(p.grad)
    _save('maf_rsample_grad', **arrays)


if __name__ == '__main__':
    gen_structure()
    gen_eval()
    gen_train()
