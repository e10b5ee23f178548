"""BernoulliRatSpn at the shapes that reach every DIST = 1 instantiation of the RAT-SPN leaf kernels: the case table, seeded
models and evidence, and the float64 references the device tests compare with.  Everything here runs on the host.

Routes (csrc/ratspn_fwd.hip::leaf_forward_dispatch, csrc/ratspn_layers.hip::leaf_backward_common), R = regions, I = channels,
d = variables per region, QB = leaf_group(R) = 4 if R % 4 == 0 else 2, CB = channel_block(I) = largest of 8, 4, 2, 1 dividing I:
  forward   ratspn_leaf_kernel<1, QB, CB, SPL>; SPL = 1 only when I % 8 == 0 and B <= 32768;
  backward  leaf_bwd_moment_kernel<1, false>     B <= 2048, 32 % I == 0, R I % 32 == 0;
            leaf_bwd_param_lds_kernel<1, CBK>    otherwise, B <= 1024 (16-sample tiles staged in LDS, `passes` per work-group);
            leaf_bwd_param_kernel<1, CBK>        otherwise, B > 1024 (64-sample tiles); CBK = largest of 4, 2, 1 dividing I.

A helper module (no tests in it)."""
import functools

import numpy as np
import torch

from oracle import ratspn_oracle as orc

#: name -> (constructor kwargs, R, d, pad) as BernoulliRatSpn(random_state=3, **kwargs) builds them; None = not pinned
CASES = {
    # CB 8, SPL 1; 13 chunks of 64 features per region, the last 16 wide (d = 196); moment kernel with the vector loads, 25
    # column tiles, the last ragged (784 = 24 * 32 + 16), 32 / I = 4 regions per row tile, no padding
    'mnist8': (dict(in_features=784, rg_depth=2, rg_repetitions=4, rg_batch=8, rg_sum=8), 16, 196, 0),
    # QB 2 (R % 4 != 0); two CB-8 blocks; moment kernel with 2 regions per row tile; classes
    'wide16_d1': (dict(in_features=100, rg_depth=1, rg_repetitions=3, rg_batch=16, rg_sum=4, out_classes=3), 6, 50, 0),
    # CB 2, padded; R I = 80: staged / 64-sample kernels with CBK 2; D % 4 != 0: the scalar staging copy
    'pad2': (dict(in_features=61, rg_depth=3, rg_repetitions=5, rg_batch=2, rg_sum=3), 40, 8, 3),
    # CB 1, CBK 1, odd d; staged kernel, 64-sample kernel above 1024 samples
    'odd3': (dict(in_features=130, rg_depth=2, rg_repetitions=7, rg_batch=3, rg_sum=5, out_classes=2), 28, 33, 2),
    # one channel; staged kernel with the float4 staging copy (D % 4 == 0)
    'one': (dict(in_features=64, rg_depth=2, rg_repetitions=4, rg_batch=1, rg_sum=2), 16, 16, 0),
    # CB 4, the widest binary benchmark; moment kernel WITH padding (gradients zeroed first), 49 column tiles
    'ad4': (dict(in_features=1556, rg_depth=4, rg_repetitions=3, rg_batch=4, rg_sum=4), 48, 98, 12),
    # pad >= d: the per_rep reasoning of leaf_backward_common for d/dx
    'heavy_pad': (dict(in_features=9, rg_depth=3, rg_repetitions=5, rg_batch=2, rg_sum=2), None, None, None),
    # 16 region groups x 3 channel blocks: at 1024 samples the staged kernel's `passes` loop (ratspn_layers.hip, "tiles per
    # work-group of the staged kernel") reaches 4 on 256 compute units: cdiv(1024, 32) * 16 * 3 = 1536 >= 512 and
    # cdiv(1024, 64) * 48 = 768 >= 512, then cdiv(1024, 128) * 48 = 384 < 512 -- the 8 repetitions of the table are enough
    'many_groups': (dict(in_features=61, rg_depth=3, rg_repetitions=8, rg_batch=3, rg_sum=2), 64, None, None),
    # 40000 samples > 32768: CB 8 with two samples per lane
    'two_per_lane': (dict(in_features=16, rg_depth=1, rg_repetitions=2, rg_batch=8, rg_sum=8), 4, 8, 0),
}
SEED = 3
_NAME_SEED = {name: 100 + i for i, name in enumerate(sorted(CASES))}


def staged_passes(name: str, B: int, cus: int = 256) -> int:
    """Tiles per work-group the staged kernel takes for this case: the formula of leaf_backward_common restated."""
    kw = CASES[name][0]
    I = kw['rg_batch']
    R = kw['rg_repetitions'] * 2 ** kw['rg_depth']
    G = R // (4 if R % 4 == 0 else 2)
    cbk = 4 if I % 4 == 0 else (2 if I % 2 == 0 else 1)
    cdiv = lambda a, b: -(-a // b)
    passes = 1
    while passes < 8 and cdiv(B, 16 * passes * 2) * G * (I // cbk) >= 2 * cus:
        passes *= 2
    return passes


def make_model(name: str):
    """The case's BernoulliRatSpn on the host, in eval mode: logits 3 * randn, 2 % of them at +-40 (both ends of the
    softplus), a handful exactly 0, and no other logit with a magnitude below 1e-3 (the one-ulp zone of sigmoid(l) >= 0.5 is
    not probed).  Asserts the region graph of the table."""
    from deeprob.spn.models import BernoulliRatSpn
    kw, R, d, pad = CASES[name]
    gen = torch.Generator().manual_seed(_NAME_SEED[name])
    torch.manual_seed(_NAME_SEED[name])                 # (the sum weights' Dirichlet initialiser)
    model = BernoulliRatSpn(random_state=SEED, **kw).eval()
    base = model.base_layer
    assert R is None or base.in_regions == R, (name, base.in_regions)
    assert d is None or base.dimension == d, (name, base.dimension)
    assert pad is None or base.pad == pad, (name, base.pad)
    if name == 'heavy_pad':
        assert base.pad >= base.dimension, (base.pad, base.dimension)
    with torch.no_grad():
        lg = 3.0 * torch.randn(base.logits.shape, generator=gen)
        small = lg.abs() < 1e-3
        lg[small] = torch.where(lg[small] < 0, torch.tensor(-1e-3), torch.tensor(1e-3))
        flat = lg.view(-1)
        n = flat.numel()
        perm = torch.randperm(n, generator=gen)
        n40 = max(2, n // 50)
        flat[perm[:n40:2]] = 40.0
        flat[perm[1:n40:2]] = -40.0
        flat[perm[n40:n40 + min(5, max(1, n // 20))]] = 0.0
        base.logits.copy_(lg)
    return model


def make_evidence(name: str, B: int, kind: str, nan_frac: float = 0.2, inf_rows: bool = True):
    """[B, D] float32.  'binary': clean 0 / 1.  'nan': `nan_frac` NaN, row 0 all NaN, row 1 fully observed, and (B >= 4,
    `inf_rows`) rows 2 and 3 with one +inf and one -inf entry each, in two variables that share no leaf region.  'soft': the
    finite non-binary values 0.3, 2.0, -1.0 mixed in (-BCEWithLogits is linear in x)."""
    D = CASES[name][0]['in_features']
    gen = torch.Generator().manual_seed(1000 * _NAME_SEED[name] + B)
    x = (torch.rand(B, D, generator=gen) < 0.5).float()
    if kind == 'binary':
        return x
    if kind == 'soft':
        pick = torch.rand(B, D, generator=gen)
        x[pick < 0.10] = 0.3
        x[(pick >= 0.10) & (pick < 0.15)] = 2.0
        x[(pick >= 0.15) & (pick < 0.20)] = -1.0
        return x
    assert kind == 'nan', kind
    x[torch.rand(B, D, generator=gen) < nan_frac] = float('nan')
    x[0] = float('nan')
    if B > 1:
        x[1] = (torch.rand(D, generator=gen) < 0.5).float()
    if inf_rows and B >= 4:
        together = _same_region(name)
        for row in (2, 3):
            # the two entries never share a leaf region: a region that holds both sums nan_to_num's +max and -max with its
            # finite terms, and which of those survive depends on the ORDER of the reference's own summation
            for _ in range(1000):
                f = torch.randperm(D, generator=gen)[:2]
                if not together[f[0], f[1]]:
                    break
            else:
                raise AssertionError('no pair of variables of %s in different regions of every repetition' % name)
            x[row, f[0]] = float('inf')
            x[row, f[1]] = float('-inf')
    return x


@functools.lru_cache(maxsize=None)
def _same_region(name: str) -> torch.Tensor:
    """[D, D] bool: the two variables share a leaf region in some repetition."""
    D = CASES[name][0]['in_features']
    mask = make_model(name).base_layer.mask                                          # [R, d]
    member = torch.zeros(mask.shape[0], D)
    member.scatter_(1, mask, 1.0)
    return (member.t() @ member) > 0


def inf_row_mask(x: torch.Tensor) -> torch.Tensor:
    return torch.isinf(x).any(dim=1)


def forward_reference(sd_f64, x):
    """(log-likelihoods [B, C], leaf layer output [B, R, I]) of the oracle as float64 arrays: evaluated in float64 -- except
    the rows with +-inf evidence, which are evaluated in float32, the reference's own format.  There the reference's
    nan_to_num (ratspn.py:103) turns a +-inf leaf term into the LARGEST FINITE NUMBER OF THE FORMAT, and that number is part
    of the result: 3.4e38 in the reference, 1.8e308 in a float64 restatement, which no float32 kernel can return.  (What such
    a row gives -- +inf where two such terms meet in a product, the bare clamp, or a log-likelihood in which they cancelled
    -- is the reference's to say, and the same in both formats wherever it is not the clamp itself.)"""
    def run(sd, xx):
        leaf = orc.bernoulli_leaf(xx, sd['base_layer.mask'], sd.get('base_layer.pad_mask'), sd['base_layer.logits'])
        return orc.ratspn_forward(sd, xx).double().numpy(), leaf.double().numpy()

    ll, leaf = run(sd_f64, x.double())
    planted = inf_row_mask(x)
    if planted.any():
        sd_f32 = {k: (v.float() if v.is_floating_point() else v) for k, v in sd_f64.items()}
        ll32, leaf32 = run(sd_f32, x[planted].float())
        ll[planted.numpy()], leaf[planted.numpy()] = ll32, leaf32
    return ll, leaf


def sd_as(model, dtype):
    return {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu().clone())
            for k, v in model.state_dict().items()}


def sd64(model):
    """The model's state dict in float64 (integer / boolean buffers as they are)."""
    return sd_as(model, torch.float64)


def param_names(sd):
    return [k for k, v in sd.items() if v.is_floating_point()]


def reference_grads(sd, x, y=None, dtype=torch.float64):
    """Plain autograd of the oracle in `dtype`: gradients of ratspn_loss w.r.t. every floating-point entry of `sd` and x."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    names = param_names(sd)
    for k in names:
        sd[k] = sd[k].clone().requires_grad_(True)
    xo = x.to(dtype).clone().requires_grad_(True)
    with torch.enable_grad():
        orc.ratspn_loss(orc.ratspn_forward(sd, xo), y).backward()
    out = {k: sd[k].grad.double().numpy() for k in names}
    out['x'] = xo.grad.double().numpy()
    return out


def masked_reference_grads(sd, x, nan_mask, dtype=torch.float64, y=None):
    """The masked gradient (the HIP path's, see test_gradients_with_marginalised_inputs): the same forward value, the
    marginalised leaf terms cut out of the graph through drops={'leaf': ...} of the oracle's forward -- the reference's own
    backward computes 0 * NaN there and returns NaN.  `x` may hold NaN exactly where `nan_mask` is set."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    names = param_names(sd)
    for k in names:
        sd[k] = sd[k].clone().requires_grad_(True)
    mask = sd['base_layer.mask']
    I = sd['base_layer.logits'].shape[1]
    drop = nan_mask[:, mask].unsqueeze(2).expand(-1, -1, I, -1)                      # [B, R, I, d]
    xf = torch.where(nan_mask, torch.zeros_like(x), x).to(dtype).requires_grad_(True)
    with torch.enable_grad():
        orc.ratspn_loss(orc.ratspn_forward(sd, xf, drops={'leaf': drop}), y).backward()
    out = {k: sd[k].grad.double().numpy() for k in names}
    out['x'] = xf.grad.double().numpy()
    return out


def labels(name: str, B: int):
    C = CASES[name][0].get('out_classes', 1)
    return (torch.arange(B) % C) if C > 1 else None
