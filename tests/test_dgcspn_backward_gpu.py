"""The DGC-SPN backward kernels (csrc/dgcspn.hip) against fp64 autograd of the oracle, layer by layer and at the example
model's 16 / 32 channels (examples/dgcspn_mnist.py): the generic sum backward across its blocks of 16 output channels and
its dispatch boundary, the 8-channel kernel on both sides of its exp-domain / exact switch (plain and tap-reading), the
product backward kernels on geometries the models do not reach, the fused level's backward against fp64 directly, and the
example model in training mode (plain, marginalised, with dropout, MPE).

Bars: gradients 1e-4 of the reference tensor's largest magnitude (tests.util.grad_err), values 1e-5 (rel_err); the
depthwise product backward 1e-6 (a sum of at most four addends).  The model-level bars are max(1e-4, 4 x the error of the
fp32 CPU oracle against the fp64 one), computed inside the test and written out by report_measured where they exceed 1e-4
(profiles/dgcspn_backward_measured_errors.txt)."""
import numpy as np
import pytest
import torch

from oracle import dgcspn_oracle as dorc
from tests.util import rel_err, grad_err, report_measured, randomise_dgc, dropout_mask

pytestmark = pytest.mark.gpu

LL_TOL = 1e-5
GRAD_TOL = 1e-4
NINF = float('-inf')


def sum_layer(weight):
    """A SpatialSumLayer with this weight [Cout, Cin, H, W].  The layer's initialiser keeps the reference's axis swap and so
    fills square maps only; the kernels take any H x W, so the layer is built on a 1 x 1 map and handed its weight."""
    from deeprob.spn.layers.dgcspn import SpatialSumLayer
    cout, cin, h, w = weight.shape
    layer = SpatialSumLayer((cin, 1, 1), cout)
    layer.in_features, layer.out_features = (cin, h, w), (cout, h, w)
    layer.weight = torch.nn.Parameter(weight.clone())
    return layer


# ---- 1. the generic sum backward across its block and dispatch boundaries ---------------------------------------------------
SUM_CASES = [(16, 32, (7, 7), 37), (32, 32, (5, 9), 19),       # the example model's levels
             (8, 9, (6, 6), 17), (9, 8, (6, 6), 17),           # the generic side of the Cin <= 8 && Cout <= 8 dispatch
             (12, 16, (4, 4), 33), (12, 17, (4, 4), 16),       # exactly one block of 16 outputs; a second block of one
             (16, 33, (3, 5), 48),                             # a third block
             (40, 3, (4, 4), 5)]                               # Cin > 32: the forward kernel without register exponentials


def sum_layer_case(cin, cout, hw, B):
    """Inputs of the extreme-weights test at these sizes and their fp64 reference: x ~ 3 N(0,1), channel 1 raised by 100
    under a weight row of -200, sample 1 with every other channel at log 0, sample 0 entirely log 0.  fp64 autograd of
    logsumexp is NaN for sample 0, so the gradients are those of samples 1.. (its own input gradient must be 0)."""
    gen = torch.Generator().manual_seed(1000 * cin + cout)
    h, w = hw
    x = torch.randn(B, cin, h, w, generator=gen) * 3
    x[:, 1] += 100.0
    x[1, ::2] = NINF
    x[0] = NINF
    e = -torch.log(torch.rand(cout, cin, h, w, generator=gen))          # log of Dirichlet(1) rows: the layer's own start
    weight = torch.log(e / e.sum(1, keepdim=True))
    weight[0, 1] = -200.0
    layer = sum_layer(weight)
    go = torch.randn(B, cout, h, w, generator=gen)
    x64 = x[1:].double().requires_grad_(True)
    w64 = layer.weight.detach().double().requires_grad_(True)
    out64 = dorc.spatial_sum(x64, w64)
    out64.backward(go[1:].double())
    return layer, x, go, out64.detach().numpy(), x64.grad.numpy(), w64.grad.numpy()


@pytest.mark.parametrize('cin,cout,hw,B', SUM_CASES)
def test_generic_sum_backward_blocks_and_dispatch(cin, cout, hw, B):
    """SpatialSumLayer forward and backward: spatial_sum_bwd_kernel walks the outputs in blocks of 16 and adds into gx
    from the second block on; batches 17, 19, 33 and 37 leave a ragged last slice of 16 samples.  Then with only x and
    with only the weight requiring a gradient (the null grad_weight / grad_x pointers of dpk_spatial_sum_backward)."""
    layer, x, go, out64, gx64, gw64 = sum_layer_case(cin, cout, hw, B)
    layer = layer.cuda()
    errs = {}
    for need_x, need_w in ((True, True), (True, False), (False, True)):
        layer.weight.requires_grad_(need_w)
        layer.weight.grad = None
        xd = x.cuda().requires_grad_(need_x)
        y = layer(xd)
        y.backward(go.cuda())
        tag = ('x' if need_x else '') + ('w' if need_w else '')
        yc = y.detach().cpu()
        assert torch.equal(yc[0], torch.full_like(yc[0], NINF))
        errs[tag + ':out'] = rel_err(yc[1:].numpy(), out64) / LL_TOL
        if need_x:
            assert not xd.grad[0].any(), 'the all-log-0 sample has a non-zero input gradient'
            errs[tag + ':gx'] = grad_err(xd.grad[1:].cpu().numpy(), gx64) / GRAD_TOL
        else:
            assert xd.grad is None
        if need_w:
            errs[tag + ':gw'] = grad_err(layer.weight.grad.cpu().numpy(), gw64) / GRAD_TOL
        else:
            assert layer.weight.grad is None
    print('sum backward {}->{} {}x{} B={}: error / bar {}'.format(
        cin, cout, hw[0], hw[1], B, ' '.join('{} {:.3f}'.format(k, v) for k, v in errs.items())))
    assert max(errs.values()) <= 1.0, errs


# ---- 2. the exp-domain / exact switch of the 8-channel kernel --------------------------------------------------------------
SWITCH_WL = (-60.0, -63.9, -64.5, -75.0, -79.0, -79.9, -80.5, -95.0, -120.0)   # the switch: 64 (80 until it lost terms)
SW_H, SW_W, SW_B = 8, 9, 21           # HW = 72: a full column of 64 pixels and a ragged one; three sample slices of 8


def switch_sites(cin, cout):
    """(wl, o, c0, c1, pixel, samples): two groups of two pixels per wl, c1 once in each half of the input channels."""
    sites = []
    for k, wl in enumerate(SWITCH_WL):
        for v, (o, c0, c1) in enumerate(((cout - 1, 1, 2), (2, 2, cin - 1))):
            j = 2 * k + v
            for p in (4 * j, 4 * j + 1):
                sites.append((wl, o, c0, c1, p, (j % SW_B, (j + 7) % SW_B, (j + 14) % SW_B)))
    assert max(s[4] for s in sites) < SW_H * SW_W and len({s[4] for s in sites}) == len(sites)
    return sites


def switch_case(cin, cout, taps):
    """Background N(0,1); at every site x[c0] = 100 under weight[o, c0] = wl, weight[o, c1] = 0, the rest of the row
    -300, x[c1] = 100 + wl - 7.6 and the cotangent g[o] = 1.5: m - out_o ~ -wl, and c1 holds a responsibility of
    e^-7.6 ~ 5e-4 for output o whose exp-domain factor e^{x_c1 - m} leaves the normal fp32 range from wl = -79.8 down.
    taps: the sum layer reads a 'full', dilation-2 depthwise product of a 6 x 7 map, the values planted on the product
    map through one tap each.  Returns the product layer (or None), the input, weight, cotangent, per wl the input
    elements that carry its sites' c1 values, and the fp64 values, input gradient and weight gradient."""
    from deeprob.spn.layers.dgcspn import SpatialProductLayer
    gen = torch.Generator().manual_seed(100 * cin + cout + (7 if taps else 0))
    sites = switch_sites(cin, cout)
    weight = torch.randn(cout, cin, SW_H, SW_W, generator=gen)
    go = torch.randn(SW_B, cout, SW_H, SW_W, generator=gen) * 0.3
    want, wl_of = {}, {}                                         # (b, c, oh, ow) -> value of the sum layer's input
    for wl, o, c0, c1, p, samples in sites:
        oh, ow = divmod(p, SW_W)
        weight[o, :, oh, ow] = -300.0
        weight[o, c0, oh, ow] = wl
        weight[o, c1, oh, ow] = 0.0
        for b in samples:
            go[b, o, oh, ow] = 1.5
            want[(b, c0, oh, ow)] = 100.0
            want[(b, c1, oh, ow)] = 100.0 + wl - 7.6
            wl_of[(b, c1, oh, ow)] = wl
    carriers = {wl: [] for wl in SWITCH_WL}                      # wl -> the elements of x that hold its sites' c1 values
    if not taps:
        prod = None
        x = torch.randn(SW_B, cin, SW_H, SW_W, generator=gen)
        for (b, c, oh, ow), v in want.items():
            x[b, c, oh, ow] = v
            if (b, c, oh, ow) in wl_of:
                carriers[wl_of[(b, c, oh, ow)]].append((b, c, oh, ow))
    else:
        prod = SpatialProductLayer((cin, SW_H - 2, SW_W - 2), 2, 'full', 1, 2, depthwise=True)
        assert prod.out_features == (cin, SW_H, SW_W) and prod.pad == [2, 2, 2, 2]
        x = (torch.randn(SW_B, cin, SW_H - 2, SW_W - 2, generator=gen) * 0.5).double()
        for (b, c, oh, ow), v in want.items():
            # product[oh, ow] = sum of x[oh - 2 + 2 th, ow - 2 + 2 tw] over the taps inside the map: move one of them
            inside = [(ih, iw) for ih in (oh, oh - 2) for iw in (ow, ow - 2) if 0 <= ih < SW_H - 2 and 0 <= iw < SW_W - 2]
            ih, iw = inside[0]
            x[b, c, ih, iw] += v - sum(x[b, c, i, j] for i, j in inside)
            if (b, c, oh, ow) in wl_of:
                carriers[wl_of[(b, c, oh, ow)]].append((b, c, ih, iw))
        x = x.float()
    x64 = x.double().requires_grad_(True)
    w64 = weight.double().requires_grad_(True)
    z64 = dorc.spatial_product(x64, prod.pad, 1, 2, True) if taps else x64
    for (b, c, oh, ow), v in want.items():                       # (a later site must not have moved an earlier one)
        assert abs(z64[b, c, oh, ow].item() - v) < 1e-3, (b, c, oh, ow)
    out64 = dorc.spatial_sum(z64, w64)
    for wl, o, c0, c1, p, samples in sites:
        oh, ow = divmod(p, SW_W)
        for b in samples:
            assert abs(100.0 - out64[b, o, oh, ow].item() + wl) < 0.01
    out64.backward(go.double())
    return prod, x, weight, go, carriers, out64.detach().numpy(), x64.grad.numpy(), w64.grad.numpy()


@pytest.mark.parametrize('taps', [False, True], ids=['layer', 'taps'])
@pytest.mark.parametrize('cin,cout', [(8, 8), (5, 7)])
def test_sum_backward8_switch_between_exp_domain_and_exact(cin, cout, taps):
    """spatial_sum_bwd8_kernel<false> (through SpatialSumLayer) and <true> (through spatial_prodsum_autograd) around the
    value of m - out_o at which the kernel leaves the exp-domain product for the exact log-domain expression.  That was
    80: just below it e^{x_c - m} is under the smallest normal fp32, where __expf returns 0, while the responsibility
    W e^{x_c - out_o} is still 5e-4 -- the wl = -79.9 sites were off by 1.4e-4 to 2.1e-4 of max|gx| on an MI355X (the
    bar: 1e-4).  The switch is at 64 now, where a lost term is below 1e-10; -63.9 and -64.5 sit on either side of it."""
    from deeprob.hip import ops_spatial
    prod, x, weight, go, carriers, out64, gx64, gw64 = switch_case(cin, cout, taps)
    layer = sum_layer(weight).cuda()
    xd = x.cuda().requires_grad_(True)
    if taps:
        y = ops_spatial.spatial_prodsum_autograd(xd, prod.cuda(), layer.weight, layer._ws)
        assert y is not None
    else:
        y = layer(xd)
    y.backward(go.cuda())
    gx, gw = xd.grad.cpu().numpy(), layer.weight.grad.cpu().numpy()
    for wl in SWITCH_WL:
        err = max(abs(float(gx[e]) - float(gx64[e])) for e in carriers[wl])
        print('switch {}->{} {} wl {:7.1f}: input-gradient error where its c1 values sit / max|gx| {:.3e}'.format(
            cin, cout, 'taps' if taps else 'layer', wl, err / float(np.max(np.abs(gx64)))))
    ex, ew = grad_err(gx, gx64), grad_err(gw, gw64)
    print('switch {}->{} {}: gx {:.3e} gw {:.3e} (bar {:.0e})'.format(cin, cout, 'taps' if taps else 'layer', ex, ew, GRAD_TOL))
    assert rel_err(y.detach().cpu().numpy(), out64) <= LL_TOL
    assert ex <= GRAD_TOL and ew <= GRAD_TOL, (ex, ew)


# ---- 3. the product backward kernels on their own --------------------------------------------------------------------------
def _product_backward(shape, padding, stride, dil, depthwise, B):
    from deeprob.spn.layers.dgcspn import SpatialProductLayer
    gen = torch.Generator().manual_seed(31 * shape[1] + shape[2] + B)
    layer = SpatialProductLayer(shape, 2, padding, stride, dil, depthwise=depthwise)
    x = torch.randn(B, *shape, generator=gen)
    go = torch.randn(B, *layer.out_features, generator=gen)
    x64 = x.double().requires_grad_(True)
    dorc.spatial_product(x64, layer.pad, stride, dil, depthwise).backward(go.double())
    xd = x.cuda().requires_grad_(True)
    layer.cuda()(xd).backward(go.cuda())
    return xd.grad.cpu().numpy(), x64.grad.numpy()


@pytest.mark.parametrize('B', [1, 37])
@pytest.mark.parametrize('shape,padding,stride,dil', [
    ((5, 7, 9), 'full', 1, 3), ((3, 6, 6), 'final', 1, 4),
    ((4, 17, 23), 'full', 1, 5),                  # HW = 391: two columns of the 256-pixel grid
    ((3, 16, 16), 'valid', 2, 1),
    ((3, 9, 9), 'valid', 2, 1),                   # odd size: the last row and column are read by no output
    ((1, 5, 5), 'valid', 2, 1)])                  # with B = 1: fewer planes than the minimum slice of 4
def test_depthwise_product_backward_against_fp64(shape, padding, stride, dil, B):
    """spatial_product_bwd_dw_kernel against fp64 autograd of the oracle's product; every value is a sum of at most four
    addends, hence the bar of the forward sweep (1e-6)."""
    got, want = _product_backward(shape, padding, stride, dil, True, B)
    if shape == (3, 9, 9):
        assert not want[:, :, 8, :].any() and not want[:, :, :, 8].any()
        assert not got[:, :, 8, :].any() and not got[:, :, :, 8].any()
    assert grad_err(got, want) <= 1e-6


@pytest.mark.parametrize('B', [1, 37])
@pytest.mark.parametrize('shape,padding,stride,dil,oc', [((2, 9, 9), 'valid', 2, 1, 16), ((3, 11, 5), 'full', 1, 2, 81),
                                                        ((2, 5, 7), 'full', 1, 2, 16)])
def test_combinatorial_product_backward_against_fp64(shape, padding, stride, dil, oc, B):
    """spatial_product_bwd_kernel, non-depthwise: an input gradient sums up to 4 x 27 cotangents."""
    from deeprob.spn.layers.dgcspn import SpatialProductLayer
    assert SpatialProductLayer(shape, 2, padding, stride, dil, depthwise=False).out_features[0] == oc
    got, want = _product_backward(shape, padding, stride, dil, False, B)
    assert grad_err(got, want) <= GRAD_TOL


# ---- 4. the fused level's backward against fp64 directly -------------------------------------------------------------------
def _fused_level_fp64(x, weight, gout, pad, stride, dil, device, chunk):
    """fp64 values and gradients of spatial_sum(spatial_product(x)) for samples 1.. (sample 0 is log 0 throughout), in
    batch chunks on ``device``."""
    w64 = weight.detach().to(device).double().requires_grad_(True)
    vals, gx = [], []
    for i in range(1, x.shape[0], chunk):
        xc = x[i:i + chunk].to(device).double().requires_grad_(True)
        y = dorc.spatial_sum(dorc.spatial_product(xc, pad, stride, dil, True), w64)
        y.backward(gout[i:i + chunk].to(device).double())
        vals.append(y.detach())
        gx.append(xc.grad)
    return torch.cat(vals).cpu().numpy(), torch.cat(gx).cpu().numpy(), w64.grad.cpu().numpy()


@pytest.mark.parametrize('shape,padding,stride,dil,cout,B', [
    ((8, 9, 9), 'full', 1, 2, 8, 21), ((5, 12, 12), 'valid', 2, 1, 7, 9), ((3, 7, 7), 'full', 1, 4, 4, 300),
    ((8, 16, 16), 'final', 1, 4, 8, 40),
    ((8, 59, 59), 'full', 1, 1, 8, 601)])         # the only shape here at which a thread walks more than 8 samples
def test_fused_level_autograd_against_fp64(shape, padding, stride, dil, cout, B):
    """ops_spatial.spatial_prodsum_autograd (fused forward, spatial_sum_bwd8_kernel<true> + the product backward) against
    fp64 spatial_sum(spatial_product(x)): values, input gradient, weight gradient.  The large case takes its fp64
    reference from torch's operators on the device, in batch chunks."""
    from deeprob.spn.layers.dgcspn import SpatialProductLayer, SpatialSumLayer
    from deeprob.hip import ops_spatial
    gen = torch.Generator().manual_seed(9)
    prod = SpatialProductLayer(shape, 2, padding, stride, dil, depthwise=True).cuda()
    ssum = SpatialSumLayer(prod.out_features, cout).cuda()
    with torch.no_grad():
        ssum.weight.copy_(torch.randn(ssum.weight.shape, generator=gen) * 2)
    x = torch.randn(B, *shape, generator=gen) * 3
    x[0] = NINF
    gout = torch.randn(B, cout, *prod.out_features[1:], generator=gen)
    big = B * int(np.prod(prod.out_features)) > (1 << 22)
    out64, gx64, gw64 = _fused_level_fp64(x, ssum.weight, gout, prod.pad, stride, dil, 'cuda' if big else 'cpu',
                                          48 if big else B)
    xd = x.cuda().requires_grad_(True)
    y = ops_spatial.spatial_prodsum_autograd(xd, prod, ssum.weight, ssum._ws)
    assert y is not None
    gx, gw = torch.autograd.grad(y, [xd, ssum.weight], gout.cuda())
    yc = y.detach().cpu()
    assert torch.equal(yc[0], torch.full_like(yc[0], NINF))
    assert not gx[0].any(), 'the all-log-0 sample has a non-zero input gradient'
    ev, ex, ew = rel_err(yc[1:].numpy(), out64), grad_err(gx[1:].cpu().numpy(), gx64), grad_err(gw.cpu().numpy(), gw64)
    print('fused level {} {} B={}: values {:.3e} gx {:.3e} gw {:.3e}'.format(shape, padding, B, ev, ex, ew))
    assert ev <= LL_TOL
    assert ex <= GRAD_TOL and ew <= GRAD_TOL, (ex, ew)


# ---- 5. the example model in training mode ---------------------------------------------------------------------------------
EX_SHAPE, EX_K, EX_S, EX_POOL = (1, 28, 28), 16, 32, 2


class _Seeds:
    """Replaces deeprob.hip.ops.draw_seed (as in test_dropout_gpu.py): hands out a fixed sequence and records it."""

    def __init__(self, start=7654321):
        self.next = start
        self.used = []

    def __call__(self):
        self.next = (self.next * 6364136223846793005 + 1442695040888963407) % (2 ** 62)
        self.used.append(self.next)
        return self.next


def example_model(classes, seed, **kw):
    from deeprob.spn.models import DgcSpn
    torch.manual_seed(seed)
    model = DgcSpn(EX_SHAPE, out_classes=classes, n_batch=EX_K, sum_channels=EX_S, depthwise=True, n_pooling=EX_POOL, **kw)
    randomise_dgc(model, seed)
    return model


def example_inputs(B, classes, seed, marginalised):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, *EX_SHAPE, generator=gen)
    cot = torch.randn(B, classes, generator=gen)
    if marginalised:
        x[torch.rand(x.shape, generator=gen) < 0.3] = float('nan')
        x[B // 2] = float('nan')
    return x, cot


def oracle_forward(sd, x, dtype, drops=None):
    """The CPU oracle in ``dtype``.  Marginalised pixels: the oracle's leaf goes through nan_to_num, whose autograd is NaN
    there, so the leaf map is restated with the double where of direct_spatial_gaussian_backward and handed over as z."""
    plan = dorc.schedule(EX_SHAPE, EX_K, EX_S, True, EX_POOL)
    seen = ~torch.isnan(x)
    xo = torch.where(seen, x, torch.zeros_like(x)).to(dtype).requires_grad_(True)
    if bool(seen.all()):
        return xo, dorc.dgcspn_forward(sd, xo, plan, drops=drops)
    assert drops is None
    lp = torch.distributions.Normal(sd['base_layer.loc'], sd['base_layer.scale']).log_prob(xo[:, None])
    z = torch.where(seen[:, None], lp, torch.zeros_like(lp)).sum(2)
    return xo, dorc.dgcspn_forward(sd, xo, plan, z=z)


def oracle_gradients(model, x, cot, dtype, drops=None):
    """Values and gradients of (out * cot).sum() / B by the CPU oracle in ``dtype``: {'x': ..., parameter name: ...}."""
    sd = {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.cpu()) for k, v in model.state_dict().items()}
    names = [k for k, p in model.named_parameters() if p.requires_grad]
    for k in names:
        sd[k].requires_grad_(True)
    xo, out = oracle_forward(sd, x, dtype, drops)
    ((out * cot.to(dtype)).sum() / x.shape[0]).backward()
    grads = {k: sd[k].grad.numpy() for k in names}
    grads['x'] = xo.grad.numpy()
    return out.detach().numpy(), grads


def check_example_gradients(label, model, x, cot, drops_of=None):
    """One training-mode forward / backward of the HIP model under the linear loss against the fp64 oracle; per tensor the
    bar of test_gradients_golden, max(GRAD_TOL, 4 x the fp32 CPU oracle's own error)."""
    B = x.shape[0]
    model = model.cuda()
    xd = x.cuda().requires_grad_(True)
    out = model(xd)
    ((out * cot.cuda()).sum() / B).backward()
    drops = drops_of(model) if drops_of is not None else None
    out64, g64 = oracle_gradients(model, x, cot, torch.float64, drops)
    _, g32 = oracle_gradients(model, x, cot, torch.float32, drops)
    got = {k: p.grad.cpu().numpy() for k, p in model.named_parameters() if p.requires_grad}
    got['x'] = xd.grad.cpu().numpy()
    assert set(got) == set(g64) and len(got) >= 8
    assert np.isfinite(got['x']).all()
    assert not got['x'][torch.isnan(x).numpy()].any(), 'marginalised pixels have a non-zero gradient'
    failed = []
    for k in sorted(got):
        noise = grad_err(g32[k], g64[k])
        err, bar = grad_err(got[k], g64[k]), max(GRAD_TOL, 4 * noise)
        print('{} {:24s} error {:.3e}  fp32 oracle {:.3e}  bar {:.3e}'.format(label, k, err, noise, bar))
        if bar > GRAD_TOL:
            report_measured('test_dgcspn_backward_gpu {} grad {}'.format(label, k), err, bar,
                            '4 x fp32 CPU oracle vs fp64 ({:.3e})'.format(noise))
        if not err <= bar:
            failed.append((k, err, bar))
    assert rel_err(out.detach().cpu().numpy(), out64) <= LL_TOL
    assert not failed, failed


@pytest.mark.parametrize('B,classes', [(8, 10), (65, 3)])
def test_example_model_gradients(B, classes):
    """examples/dgcspn_mnist.py's model: every level through the layer chain, the sums on spatial_sum_bwd_kernel at
    16 -> 32 and 32 -> 32 channels."""
    x, cot = example_inputs(B, classes, 40 + B, False)
    check_example_gradients('example[B={},classes={}]'.format(B, classes), example_model(classes, 50 + B), x, cot)


def test_example_model_gradients_with_marginalised_inputs():
    """30 % of the pixels and one whole image marginalised: their input gradient is exactly 0."""
    x, cot = example_inputs(8, 10, 61, True)
    check_example_gradients('example[marginalised]', example_model(10, 62), x, cot)


def test_example_model_gradients_with_its_dropout_rates(monkeypatch):
    """in_dropout = sum_dropout = 0.2 in .train(), the masks replayed by the oracle from the recorded seeds."""
    from deeprob.hip import ops
    seeds = _Seeds()
    monkeypatch.setattr(ops, 'draw_seed', seeds)
    B = 8
    x, cot = example_inputs(B, 10, 71, False)
    model = example_model(10, 72, in_dropout=0.2, sum_dropout=0.2).train()

    def drops_of(m):
        used = list(seeds.used)
        drops = {'leaf': dropout_mask(used.pop(0), (B, EX_K) + EX_SHAPE, 0.2)}
        for i, layer in enumerate(m.layers):
            if not hasattr(layer, 'pad'):
                drops['layers.{}'.format(i)] = dropout_mask(used.pop(0), (B,) + tuple(layer.in_features), 0.2)
        assert not used
        return drops

    check_example_gradients('example[dropout]', model, x, cot, drops_of)


def test_example_model_mpe():
    """DgcSpn.mpe (the layer chain's backward down to the leaf map) on the marginalised batch against the fp64 oracle, by
    the rule of test_mpe_golden: max(1e-5, 4 x the fp32 CPU oracle's error); observed pixels come back bit for bit."""
    x, _ = example_inputs(8, 10, 61, True)
    model = example_model(10, 62)
    plan = dorc.schedule(EX_SHAPE, EX_K, EX_S, True, EX_POOL)
    sd32 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd32.items()}
    mpe64 = dorc.dgcspn_mpe(sd64, x.double(), plan).numpy()
    noise = float(np.max(np.abs(dorc.dgcspn_mpe(sd32, x, plan).numpy() - mpe64)))
    model = model.cuda()
    with torch.enable_grad():
        mpe = model.mpe(x.cuda()).cpu().numpy()
    seen = ~np.isnan(x.numpy())
    assert np.array_equal(mpe[seen], x.numpy()[seen])
    err, bar = float(np.max(np.abs(mpe - mpe64))), max(1e-5, 4 * noise)
    print('example[mpe] error {:.3e}  fp32 oracle {:.3e}  bar {:.3e}'.format(err, noise, bar))
    if bar > 1e-5:
        report_measured('test_dgcspn_backward_gpu example[mpe] completion', err, bar,
                        '4 x fp32 CPU oracle vs fp64 ({:.3e})'.format(noise))
    assert err <= bar
