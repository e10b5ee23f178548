"""MAF on the HIP path against the reference's goldens (tools/gen_golden_maf.py) and a float64 restatement
(tests/maf_cases.py): the fused density kernel, the sampling kernel, the chained / autograd routes, the step loop."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.util import rel_err, grad_err, state_to_model
from tests import maf_cases as mc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = torch.device('cuda', 0)

# name -> (constructor kwargs, D, torch seed, perturbation seed): tools/gen_golden_maf.py CASES
CASES = {
    'maf192_bn': (dict(), 192, 3, 4),
    'maf192_nobn': (dict(batch_norm=False), 192, 3, 4),
    'maf192_rand8': (dict(sequential=False, units=8, random_state=42), 192, 3, 4),
    'maf192_logit': (dict(logit=0.01), 192, 3, 4),
    'maf784_seq': (dict(), 784, 10, 11),
    'maf784_rand': (dict(sequential=False, random_state=42), 784, 10, 11),
    'maf2_energy': (dict(n_flows=10, batch_norm=False), 2, 5, 6),
    'maf20_depth2': (dict(depth=2, units=48, n_flows=3), 20, 7, 8),
    'maf20_depth3': (dict(depth=3, units=40, n_flows=2, activation='tanh'), 20, 7, 8),
    'maf33_leaky': (dict(activation='leaky-relu', units=40, n_flows=2), 33, 9, 1),
    'maf33_softplus': (dict(activation='softplus', units=40, n_flows=2), 33, 9, 1),
    'maf33_tanh': (dict(activation='tanh', units=40, n_flows=2), 33, 9, 1),
    'maf33_sigmoid': (dict(activation='sigmoid', units=40, n_flows=2), 33, 9, 1),
    'maf33_relu_u70': (dict(units=70, n_flows=2), 33, 9, 1),
    'maf12_units200': (dict(units=200, n_flows=2), 12, 2, 3),
}


def _model(name):
    kw, D, seed, pseed = CASES[name]
    return mc.build(kw, D, seed, pseed).to(DEV)


@pytest.mark.parametrize('name', sorted(CASES))
def test_golden_eval(name):
    g = np.load(os.path.join(GOLD, 'maf_' + name + '.npz'))
    m = _model(name)
    x = torch.from_numpy(g['x']).to(DEV)
    with torch.no_grad():
        ll = m(x).cpu().numpy()
        h = m.preprocess(x)[0] if m.logit is not None else x
        u, ildj = m.apply_backward(h)
        xr, ldj = m.apply_forward(torch.from_numpy(g['u']).to(DEV))
        hl = h
        for i, layer in enumerate(list(m.layers)[:2]):
            hl, d = layer.apply_backward(hl)
            assert rel_err(hl.cpu().numpy(), g['layer{}.u'.format(i)]) <= 1e-5, (name, i)
            assert rel_err(d.cpu().numpy(), g['layer{}.ildj'.format(i)]) <= 1e-5, (name, i)
    # log-likelihood: distance to float64 within max(1e-4, 2 x the reference's own fp32 distance)
    ref_dist = rel_err(g['ll'], g['ll64'])
    assert rel_err(ll, g['ll64']) <= max(1e-4, 2 * ref_dist), (name, rel_err(ll, g['ll64']), ref_dist)
    assert rel_err(ll, g['ll']) <= 1e-5
    assert rel_err(u.cpu().numpy(), g['u']) <= 1e-5
    assert rel_err(ildj.cpu().numpy(), g['ildj']) <= 1e-5
    assert rel_err(xr.cpu().numpy(), g['x_rec']) <= 1e-5
    assert rel_err(ldj.cpu().numpy(), g['ldj']) <= 1e-5


def _assert_flow_inverse(flow, data):
    target, ildj = flow.apply_backward(data)
    orig, ldj = flow.apply_forward(target)
    assert torch.allclose(ildj, -ldj, atol=5e-7)
    assert torch.allclose(orig, data, atol=5e-7)


def test_reference_round_trip_and_rsample():
    from deeprob.flows.models import MAF
    data = torch.rand(32, 192, generator=torch.Generator().manual_seed(0)).to(DEV)
    shape = torch.Size([192])
    for kw in [dict(batch_norm=True), dict(batch_norm=False), dict(batch_norm=True, units=8, sequential=False, random_state=42),
               dict(batch_norm=False, units=8, sequential=False, random_state=42)]:
        _assert_flow_inverse(MAF(shape, **kw).to(DEV).eval(), data)
        with torch.no_grad():
            _assert_flow_inverse(MAF(shape, **kw).to(DEV).eval(), data)
    maf = MAF(shape, batch_norm=True, dequantize=True, logit=0.01).to(DEV).eval()
    _assert_flow_inverse(maf, data)
    with torch.enable_grad():
        samples = maf.rsample(64)
        assert samples.requires_grad
        samples.mean().backward()
    assert maf.layers[0].network[0].weight.grad is not None


def _layer(D, units, depth=1, act='relu', seed=0, sequential=True, scale=0.3):
    from deeprob.flows.layers.autoregressive import AutoregressiveLayer
    torch.manual_seed(seed)
    layer = AutoregressiveLayer(D, depth, units, act, reverse=seed % 2 == 1, sequential=sequential,
                                random_state=np.random.RandomState(seed))
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        layer.scale_act.weight.fill_(0.5)
        for m in layer.network:
            if hasattr(m, 'mask'):
                m.weight.add_(scale * torch.randn(m.weight.shape, generator=g) / np.sqrt(m.weight.shape[1]))
    return layer.to(DEV)


@pytest.mark.parametrize('B,D,seq', [(1, 784, True), (63, 784, False), (65, 784, True), (4097, 50, False),
                                     (65536, 96, True)])
def test_sampling_kernel_vs_float64_step_loop(B, D, seq):
    layer = _layer(D, 128, seed=3 + B % 7, sequential=seq)
    u = torch.randn(B, D, generator=torch.Generator().manual_seed(B)).to(DEV)
    with torch.no_grad():
        x, ldj = layer.apply_forward(u)
    rows = np.random.RandomState(0).choice(B, size=min(B, 256), replace=False)
    want, wl = mc.sample_step_loop64(layer, 'relu', u[rows].cpu().numpy())
    assert rel_err(x[rows].cpu().numpy(), want) <= 1e-4
    assert rel_err(ldj[rows].cpu().numpy(), wl) <= 1e-4


def test_sampling_kernel_custom_mask_zero_fill():
    # a depth-1 mask that is NOT autoregressive in the layer's order: the kernel must follow the reference's semantics
    # (the conditioner sees the variables produced so far, the others zero)
    layer = _layer(24, 40, seed=5)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for m in layer.network:
            if hasattr(m, 'mask'):
                m.mask.copy_((torch.rand(m.mask.shape, generator=g) < 0.6).float().to(DEV))
    u = torch.randn(70, 24, generator=g).to(DEV)
    with torch.no_grad():
        x, ldj = layer.apply_forward(u)
        xs, ls = __import__('deeprob.hip.ops_maf', fromlist=['x']).step_loop(u, layer)
    want, wl = mc.sample_step_loop64(layer, 'relu', u.cpu().numpy())
    assert rel_err(x.cpu().numpy(), want) <= 1e-4 and rel_err(ldj.cpu().numpy(), wl) <= 1e-4
    assert rel_err(xs.cpu().numpy(), want) <= 1e-4 and rel_err(ls.cpu().numpy(), wl) <= 1e-4


def test_depth2_custom_mask_takes_step_loop():
    layer = _layer(10, 16, depth=2, act='tanh', seed=2)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for m in layer.network:
            if hasattr(m, 'mask'):
                m.mask.copy_((torch.rand(m.mask.shape, generator=g) < 0.7).float().to(DEV))
    u = torch.randn(33, 10, generator=g).to(DEV)
    from deeprob.hip import ops_maf
    assert ops_maf.deep_schedule(layer) is None and not ops_maf.deep_sample_envelope(layer)
    calls = []
    deep, ops_maf.sample_deep_kernel = ops_maf.sample_deep_kernel, lambda *a: calls.append(1)
    try:
        with torch.no_grad():
            x, ldj = layer.apply_forward(u)
    finally:
        ops_maf.sample_deep_kernel = deep
    assert not calls
    want, wl = mc.sample_step_loop64(layer, 'tanh', u.cpu().numpy())
    assert rel_err(x.cpu().numpy(), want) <= 1e-4 and rel_err(ldj.cpu().numpy(), wl) <= 1e-4


@pytest.mark.parametrize('D,units,depth,act,seq,B', [(10, 16, 2, 'tanh', True, 33), (50, 64, 2, 'relu', False, 65),
                                                     (784, 128, 2, 'relu', True, 100), (40, 48, 3, 'sigmoid', False, 200),
                                                     (30, 24, 2, 'softplus', True, 4097)])
def test_deep_sampling_kernel_one_launch(D, units, depth, act, seq, B):
    # masks built from degrees are autoregressive in the layer's order: one launch of the deep sampling kernel
    from deeprob.hip import ops_maf, load_library
    layer = _layer(D, units, depth=depth, act=act, seed=4, sequential=seq)
    assert ops_maf.deep_sample_envelope(layer)
    lib = load_library()
    launches = []
    real = lib.dpk_maf_sample_deep_forward

    class Counting:
        def __getattr__(self, name):
            return getattr(lib, name)

        def dpk_maf_sample_deep_forward(self, *a):
            launches.append(1)
            return real(*a)
    loop, ops_maf.step_loop = ops_maf.step_loop, None          # (the step loop must not be taken)
    ops_maf.load_library = lambda: Counting()
    try:
        u = torch.randn(B, D, generator=torch.Generator().manual_seed(B)).to(DEV)
        with torch.no_grad():
            x, ldj = layer.apply_forward(u)
    finally:
        ops_maf.step_loop = loop
        ops_maf.load_library = load_library
    assert launches == [1]
    rows = np.random.RandomState(1).choice(B, size=min(B, 40), replace=False)
    want, wl = mc.sample_step_loop64(layer, act, u[rows].cpu().numpy())
    assert rel_err(x[rows].cpu().numpy(), want) <= 1e-4 and rel_err(ldj[rows].cpu().numpy(), wl) <= 1e-4


def test_masked_linear_forward_backward():
    from deeprob.torch.utils import MaskedLinear
    g = torch.Generator().manual_seed(6)
    mask = (torch.rand(9, 13, generator=g) < 0.5).numpy()
    for bias in (True, False):
        lin = MaskedLinear(13, 9, mask)
        if not bias:
            lin.bias = None
        lin = lin.to(DEV)
        x = torch.randn(3, 5, 13, generator=g).to(DEV).requires_grad_(True)
        y = lin(x)
        gy = torch.randn(3, 5, 9, generator=g).to(DEV)
        y.backward(gy)
        w = (lin.weight.detach() * lin.mask).double().cpu().numpy()
        xn, gyn = x.detach().double().cpu().numpy().reshape(-1, 13), gy.double().cpu().numpy().reshape(-1, 9)
        want = xn @ w.T + (lin.bias.detach().double().cpu().numpy() if bias else 0.0)
        assert tuple(y.shape) == (3, 5, 9)
        assert rel_err(y.detach().cpu().numpy().reshape(-1, 9), want) <= 1e-5
        assert grad_err(x.grad.cpu().numpy().reshape(-1, 13), gyn @ w) <= 1e-5
        gw = lin.weight.grad.cpu().numpy()
        assert grad_err(gw, (gyn.T @ xn) * mask) <= 1e-5 and np.all(gw[~mask] == 0)
        if bias:
            assert grad_err(lin.bias.grad.cpu().numpy(), gyn.sum(0)) <= 1e-5


def test_fused_density_folded_batch_norm_and_accumulate():
    from deeprob.hip import ops_maf
    layer = _layer(64, 96, act='tanh', seed=2)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(150, 64, generator=g).to(DEV)
    sc, sh = (torch.rand(64, generator=g) + 0.5).to(DEV), torch.randn(64, generator=g).to(DEV)
    acc = torch.randn(150, generator=g).to(DEV)
    with torch.no_grad():
        u, ildj = ops_maf.density_fused(x, layer, in_affine=(sc, sh), ildj=acc.clone())
    xa = x.double().cpu().numpy() * sc.double().cpu().numpy() + sh.double().cpu().numpy()
    wm, a = mc.layer_params(layer)
    z = mc.conditioner64(wm, 'tanh', xa)
    s_ = a * np.tanh(z[:, 64:])
    assert rel_err(u.cpu().numpy(), (xa - z[:, :64]) * np.exp(-s_)) <= 1e-5
    assert rel_err(ildj.cpu().numpy(), acc.double().cpu().numpy() - s_.sum(1)) <= 1e-5


def test_maf_eval_folds_batch_norms_into_the_fused_kernel():
    # MAF.apply_backward in eval mode without a graph: batch norms folded, same numbers as the per-layer route
    from deeprob.flows.models import MAF
    from deeprob.flows.models.base import NormalizingFlow
    from deeprob.hip import ops_maf
    m = mc.build(dict(units=64, n_flows=3), 48, 1, 2).to(DEV)
    assert all(ops_maf.fused_route(l, 48) for l in m.layers if hasattr(l, 'network'))
    x = torch.randn(90, 48, generator=torch.Generator().manual_seed(5)).to(DEV)
    calls = []
    fused = ops_maf.density_fused
    ops_maf.density_fused = lambda *a, **k: (calls.append(k.get('in_affine') is not None), fused(*a, **k))[1]
    try:
        with torch.no_grad():
            u, ildj = m.apply_backward(x)
            u0, ildj0 = NormalizingFlow.apply_backward(m, x)
    finally:
        ops_maf.density_fused = fused
    assert calls.count(True) == 2            # the layers behind the first two batch norms took them in
    assert rel_err(u.cpu().numpy(), u0.cpu().numpy()) <= 1e-5
    assert rel_err(ildj.cpu().numpy(), ildj0.cpu().numpy()) <= 1e-5
    assert isinstance(m, MAF)


def test_density_route_by_measured_cost():
    from deeprob.hip import ops_maf
    assert ops_maf.fused_route(_layer(784, 128, seed=0, sequential=True), 784)
    assert ops_maf.fused_route(_layer(784, 128, seed=1, sequential=True), 784)        # reversed degrees
    assert not ops_maf.fused_route(_layer(784, 128, seed=0, sequential=False), 784)    # random degrees: chained


@pytest.mark.parametrize('act', ['relu', 'leaky-relu', 'softplus', 'tanh', 'sigmoid'])
def test_fused_density_vs_float64(act):
    from deeprob.hip import ops_maf
    layer = _layer(77, 100, act=act, seed=1, sequential=False)
    x = torch.randn(130, 77, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        u, ildj = ops_maf.density_fused(x, layer)
        uc, ic = ops_maf.density_chain(x, layer)
    wm, a = mc.layer_params(layer)
    z = mc.conditioner64(wm, act, x.cpu().numpy())
    s = a * np.tanh(z[:, 77:])
    want = (x.cpu().numpy() - z[:, :77]) * np.exp(-s)
    for got, gi in ((u, ildj), (uc, ic)):
        assert rel_err(got.cpu().numpy(), want) <= 1e-5
        assert rel_err(gi.cpu().numpy(), -s.sum(1)) <= 1e-5


@pytest.mark.parametrize('tag', ['d1_train', 'd2_train', 'd1_eval'])
def test_training_goldens(tag):
    from deeprob.flows.models import MAF
    g = np.load(os.path.join(GOLD, 'maf_train_' + tag + '.npz'))
    kw = dict(n_flows=2, units=24, activation='tanh', depth=2 if tag.startswith('d2') else 1)
    m = state_to_model(MAF(10, **kw), g, DEV)
    m.train(tag.endswith('train'))
    x = torch.from_numpy(g['x']).to(DEV).requires_grad_(True)
    loss = -m(x).mean()
    loss.backward()
    assert rel_err(loss.detach().cpu().numpy().reshape(1), g['loss']) <= 1e-5
    assert grad_err(x.grad.cpu().numpy(), g['grad.x']) <= 1e-4
    for k, p in m.named_parameters():
        if 'grad.' + k in g.files:
            assert grad_err(p.grad.cpu().numpy(), g['grad.' + k]) <= 1e-4, k
            if '.network.' in k and k.endswith('.weight'):
                mask = dict(m.named_buffers())[k[:-len('weight')] + 'mask'].cpu().numpy()
                assert np.all(p.grad.cpu().numpy()[mask == 0] == 0), k
    for k, b in m.named_buffers():
        if 'after.' + k in g.files:
            assert rel_err(b.cpu().numpy(), g['after.' + k]) <= 1e-5, k


@pytest.mark.parametrize('act', ['tanh', 'relu'])
@pytest.mark.parametrize('depth,seq', [(1, False), (2, True)], ids=['depth1-random', 'depth2-sequential'])
def test_chain_backward_multi_tile_vs_float64(depth, seq, act):
    """The chained route and its backward where the matrix products span several tiles and split K (D = 150, 136 units,
    B = 200: dW = dOut^T In is 300 x 136 over K = 200, 15 tiles; dIn = dOut Wm accumulates into grad_x under split-K):
    float32 autograd through ops_maf.autoregressive_backward, and density_chain directly, against the float64 torch
    restatement (maf_cases.density64_torch) and its autograd.  Bars: 1e-5 relative on u / ildj, 1e-4 of the tensor's
    largest magnitude on gradients; a masked weight's gradient is exactly zero."""
    from deeprob.hip import ops_maf
    from tests.util import report_measured
    D, units, B = 150, 136, 200
    layer = _layer(D, units, depth=depth, act=act, seed=6, sequential=seq)
    gen = torch.Generator().manual_seed(11)
    x, wu, wl = torch.randn(B, D, generator=gen), torch.randn(B, D, generator=gen), torch.randn(B, generator=gen)
    u64, ildj64, x64, a64, params64 = mc.density64_torch(layer, act, x)
    ((u64 * wu.double()).sum() + (ildj64 * wl.double()).sum()).backward()
    xg = x.to(DEV).requires_grad_(True)
    u, ildj = ops_maf.autoregressive_backward(xg, layer)
    ((u * wu.to(DEV)).sum() + (ildj * wl.to(DEV)).sum()).backward()
    with torch.no_grad():
        uc, ic = ops_maf.density_chain(xg.detach(), layer)
    lins = [m for m in layer.network if hasattr(m, 'mask')]
    checks = [('u', u, u64), ('ildj', ildj, ildj64), ('density_chain u', uc, u64), ('density_chain ildj', ic, ildj64),
              ('grad.x', xg.grad, x64.grad), ('grad.scale_act.weight', layer.scale_act.weight.grad.reshape(-1), a64.grad.reshape(-1))]
    for i, (m, (w64, b64)) in enumerate(zip(lins, params64)):
        checks += [('grad.W%d' % i, m.weight.grad, w64.grad), ('grad.b%d' % i, m.bias.grad, b64.grad)]
        assert np.all(m.weight.grad.cpu().numpy()[m.mask.cpu().numpy() == 0] == 0), i
    failed = []
    for name, got, want in checks:
        is_grad = name.startswith('grad.')
        err = (grad_err if is_grad else rel_err)(got.detach().cpu().numpy(), want.detach().numpy())
        bar = 1e-4 if is_grad else 1e-5
        report_measured('test_chain_backward_multi_tile_vs_float64[depth %d, %s, %s] %s'
                        % (depth, 'sequential' if seq else 'random degrees', act, name), err, bar)
        if err > bar:
            failed.append((name, err, bar))
    assert not failed, failed


def test_training_step_lowers_loss():
    from deeprob.flows.models import MAF
    torch.manual_seed(0)
    m = MAF(16, n_flows=2, units=32).to(DEV).train()
    x = torch.randn(256, 16, generator=torch.Generator().manual_seed(1)).to(DEV) * 0.5 + 1.0
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    first = None
    for _ in range(5):
        opt.zero_grad()
        loss = m.loss(m(x))
        loss.backward()
        opt.step()
        first = float(loss) if first is None else first
    assert float(m.loss(m(x))) < first


def test_rsample_gradient_golden():
    from deeprob.flows.layers.autoregressive import AutoregressiveLayer
    g = np.load(os.path.join(GOLD, 'maf_rsample_grad.npz'))
    layer = state_to_model(AutoregressiveLayer(6, 1, 16, 'tanh', reverse=True), g, DEV)
    u = torch.from_numpy(g['u']).to(DEV).requires_grad_(True)
    x, ldj = layer.apply_forward(u)
    (x.square().sum() + 0.5 * ldj.sum()).backward()
    assert rel_err(x.detach().cpu().numpy(), g['x']) <= 1e-5
    assert grad_err(u.grad.cpu().numpy(), g['grad.u']) <= 1e-4
    for k, p in layer.named_parameters():
        assert grad_err(p.grad.cpu().numpy(), g['grad.' + k]) <= 1e-4, k


def test_fresh_parameters_after_data_writes():
    layer = _layer(40, 64, seed=7)
    x = torch.randn(100, 40, generator=torch.Generator().manual_seed(7)).to(DEV)
    with torch.no_grad():
        u0, _ = layer.apply_backward(x)
        s0, _ = layer.apply_forward(x)
        layer.network[2].weight.data.mul_(1.5)
        u1, _ = layer.apply_backward(x)
        s1, _ = layer.apply_forward(x)
        layer.network[0].mask.data.zero_()
        u2, _ = layer.apply_backward(x)
        s2, _ = layer.apply_forward(x)
    assert not torch.equal(u0, u1) and not torch.equal(s0, s1)
    assert not torch.equal(u1, u2) and not torch.equal(s1, s2)
    wm, a = mc.layer_params(layer)
    z = mc.conditioner64(wm, 'relu', x.cpu().numpy())
    want = (x.cpu().numpy() - z[:, :40]) * np.exp(-a * np.tanh(z[:, 40:]))
    assert rel_err(u2.cpu().numpy(), want) <= 1e-5
    assert rel_err(s2.cpu().numpy(), mc.sample_step_loop64(layer, 'relu', x.cpu().numpy())[0]) <= 1e-4


def test_abi_errors():
    from deeprob.hip import load_library, HipError
    lib = load_library()
    assert lib.dpk_maf_density_workspace_bytes(1, 8) == -1
    assert lib.dpk_maf_density_workspace_bytes(8, 300) == -4
    assert lib.dpk_maf_sample_workspace_bytes(8, 129) == -4
    t = torch.zeros(64, device=DEV)
    p = t.data_ptr()
    args = [p, 4, 8, p, p, p, p, p, p, 8, 0, p, None, None, p, p, p, p, p, 0, p, 16, None]
    assert lib.dpk_maf_density_forward(*args) == -2                       # short workspace
    bad = list(args); bad[3] = None
    assert lib.dpk_maf_density_forward(*bad) == -1                        # null weight
    bad = list(args); bad[2] = 1
    assert lib.dpk_maf_density_forward(*bad) == -1                        # D < 2
    sargs = [p, 4, 8, p, p, p, p, p, p, 8, 0, p, p, p, p, p, 16, None]
    assert lib.dpk_maf_sample_forward(*sargs) == -2
    bad = list(sargs); bad[9] = 0
    assert lib.dpk_maf_sample_forward(*bad) == -1
    w = (ctypes.c_int32 * 1)(8)
    assert lib.dpk_maf_chain_workspace_bytes(4, 0, 1, w, 1) == -1
    assert lib.dpk_maf_chain_workspace_bytes(4, 8, 1, w, 3) == -1
    assert 0 < lib.dpk_maf_chain_workspace_bytes(4, 8, 1, w, 0) < lib.dpk_maf_chain_workspace_bytes(4, 8, 1, w, 1) < \
        lib.dpk_maf_chain_workspace_bytes(4, 8, 1, w, 2)
    w2 = (ctypes.c_int32 * 2)(300, 300)
    assert lib.dpk_maf_sample_deep_workspace_bytes(8, 2, w2) == -4         # more than 512 hidden units
    w2 = (ctypes.c_int32 * 2)(8, 8)
    assert lib.dpk_maf_sample_deep_workspace_bytes(8, 1, w2) == -1
    arr = (ctypes.c_void_p * 3)(p, p, p)
    dargs = [p, 4, 8, 2, arr, arr, arr, w2, 0, p, p, p, p, p, p, p, 16, None]
    assert lib.dpk_maf_sample_deep_forward(*dargs) == -2
    bad = list(dargs); bad[11] = None
    assert lib.dpk_maf_sample_deep_forward(*bad) == -1
    layer = _layer(8, 16)
    with pytest.raises(HipError):
        layer.cpu().apply_backward(torch.randn(2, 8))
