"""Float64 restatement of the MAF pieces the GPU tests compare against (our own wording of the reference's
autoregressive layer: deeprob/flows/layers/autoregressive.py), and the seeded model builder of the MAF fixtures."""
import numpy as np
import torch

from tests.util import randomise_flow

ACTS = {
    'relu': lambda h: np.maximum(h, 0.0),
    'leaky-relu': lambda h: np.where(h > 0.0, h, 0.01 * h),
    'softplus': lambda h: np.where(h > 20.0, h, np.log1p(np.exp(np.minimum(h, 20.0)))),
    'tanh': np.tanh,
    'sigmoid': lambda h: 1.0 / (1.0 + np.exp(-h)),
}


def layer_params(layer):
    """[(W * M, b)] of the conditioner's masked layers, float64, plus the ScaledTanh weight."""
    lins = [m for m in layer.network if hasattr(m, 'mask')]
    wm = [((m.weight.detach().double() * m.mask.detach().double()).cpu().numpy(), m.bias.detach().double().cpu().numpy())
          for m in lins]
    return wm, float(layer.scale_act.weight.detach().double().cpu().item())


def conditioner64(wm, act, x):
    h = np.asarray(x, dtype=np.float64)
    for i, (w, b) in enumerate(wm):
        h = h @ w.T + b
        if i + 1 < len(wm):
            h = ACTS[act](h)
    return h


TORCH_ACTS = {
    'relu': torch.relu,
    'leaky-relu': lambda h: torch.nn.functional.leaky_relu(h, negative_slope=0.01),
    'softplus': lambda h: torch.nn.functional.softplus(h, beta=1, threshold=20),
    'tanh': torch.tanh,
    'sigmoid': torch.sigmoid,
}


def masked_linears(layer):
    return [m for m in layer.network if hasattr(m, 'mask')]


def set_masks(layer, masks, through_data=False):
    """Overwrite the masks of the conditioner's masked layers with the boolean patterns `masks` (one per layer, None
    keeps a layer's mask).  through_data writes through `.data`: the buffer's contents change, its version counter does
    not, so whatever the operators cache per (address, version) is stale afterwards."""
    lins = masked_linears(layer)
    assert len(masks) == len(lins)
    with torch.no_grad():
        for m, pattern in zip(lins, masks):
            if pattern is None:
                continue
            new = torch.as_tensor(np.asarray(pattern, dtype=np.float32)).to(m.mask.device)
            assert new.shape == m.mask.shape, (tuple(new.shape), tuple(m.mask.shape))
            (m.mask.data if through_data else m.mask).copy_(new)


def shift_biases(layer, up=(1, 6), down=(2, 5), by=25.0):
    """Saturate a few units of the first hidden layer: bias + `by` on the units `up`, bias - `by` on the units `down`.
    With by = 25 the `up` units sit beyond Softplus's threshold of 20 (its identity branch) and where a float32 sigmoid
    rounds to 1, the `down` units where softplus and sigmoid are about 1e-11."""
    first = masked_linears(layer)[0]
    with torch.no_grad():
        first.bias[list(up)] += by
        first.bias[list(down)] -= by
    return list(up), list(down)


def density64_torch(layer, act, x):
    """apply_backward of an AutoregressiveLayer restated in float64 torch, so that its autograd gives reference gradients:
    h <- act(F.linear(h, W o M, b)) per hidden layer, (t, s) = the halves of the last linear layer's output,
    u = (x - t) exp(-a tanh s), ildj = -sum a tanh s.  Returns (u, ildj, x64, a64, [(W64, b64)]) with the last three
    requiring grad."""
    lins = [m for m in layer.network if hasattr(m, 'mask')]
    params = [(m.weight.detach().double().cpu().requires_grad_(True), m.bias.detach().double().cpu().requires_grad_(True))
              for m in lins]
    a = layer.scale_act.weight.detach().double().cpu().requires_grad_(True)
    x = torch.as_tensor(x).detach().double().cpu().requires_grad_(True)
    h = x
    for i, (m, (w, b)) in enumerate(zip(lins, params)):
        h = torch.nn.functional.linear(h, w * m.mask.detach().double().cpu(), b)
        if i + 1 < len(lins):
            h = TORCH_ACTS[act](h)
    D = x.shape[1]
    s = a * torch.tanh(h[:, D:])
    return (x - h[:, :D]) * torch.exp(-s), -s.sum(dim=1), x, a, params


def sample_step_loop64(layer, act, u):
    """x_i = u_i exp(a tanh(s_i)) + t_i, one variable per step in the order of inv_ordering, the conditioner evaluated
    on the current x (entries not produced yet are zero)."""
    wm, a = layer_params(layer)
    u = np.asarray(u, dtype=np.float64)
    B, D = u.shape
    x = np.zeros_like(u)
    ldj = np.zeros(B)
    depth1 = len(wm) == 2
    if depth1:       # for one hidden layer the pre-activations can be carried along: the same numbers, D times cheaper
        h = np.repeat(wm[0][1][None, :], B, axis=0)
    for i in np.asarray(layer.inv_ordering):
        if depth1:
            z = np.stack([ACTS[act](h) @ wm[1][0][i] + wm[1][1][i], ACTS[act](h) @ wm[1][0][D + i] + wm[1][1][D + i]], 1)
            t, s = z[:, 0], z[:, 1]
        else:
            z = conditioner64(wm, act, x)
            t, s = z[:, i], z[:, D + i]
        s = a * np.tanh(s)
        x[:, i] = u[:, i] * np.exp(s) + t
        ldj += s
        if depth1:
            h = h + np.outer(x[:, i], wm[0][0][:, i])
    return x, ldj


def sample64_torch(layer, act, u):
    """apply_forward of an AutoregressiveLayer restated in float64 torch, so that its autograd gives the reference
    gradients of rsample: the variables are produced one per step in the order of inv_ordering, each from the whole
    conditioner evaluated on the x produced so far (the other entries zero), x_i = u_i exp(a tanh s_i) + t_i, and
    ldj = sum_i a tanh s_i.  Returns (x, ldj, u64, a64, [(W64, b64)]) with the last three requiring grad."""
    lins = masked_linears(layer)
    params = [(m.weight.detach().double().cpu().requires_grad_(True), m.bias.detach().double().cpu().requires_grad_(True))
              for m in lins]
    masks = [m.mask.detach().double().cpu() for m in lins]
    a = layer.scale_act.weight.detach().double().cpu().requires_grad_(True)
    u = torch.as_tensor(u).detach().double().cpu().requires_grad_(True)
    B, D = u.shape
    cols = [torch.zeros(B, dtype=torch.float64) for _ in range(D)]
    scales = []
    for i in np.asarray(layer.inv_ordering):
        h = torch.stack(cols, dim=1)
        for k, (mask, (w, b)) in enumerate(zip(masks, params)):
            h = torch.nn.functional.linear(h, w * mask, b)
            if k + 1 < len(lins):
                h = TORCH_ACTS[act](h)
        s = a * torch.tanh(h[:, D + i])
        cols[i] = u[:, i] * torch.exp(s) + h[:, i]
        scales.append(s)
    return torch.stack(cols, dim=1), torch.stack(scales, dim=1).sum(dim=1), u, a, params


def build(kw, D, seed, pseed):
    """The fixture's model: the same torch RNG stream as the reference's construction, then the shared perturbation."""
    from deeprob.flows.models import MAF
    torch.manual_seed(seed)
    m = MAF(D, **kw)
    randomise_flow(m, pseed)
    return m.eval()
