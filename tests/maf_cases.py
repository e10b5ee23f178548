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


TORCH_ACTS = {'relu': torch.relu, 'tanh': torch.tanh}


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


def build(kw, D, seed, pseed):
    """The fixture's model: the same torch RNG stream as the reference's construction, then the shared perturbation."""
    from deeprob.flows.models import MAF
    torch.manual_seed(seed)
    m = MAF(D, **kw)
    randomise_flow(m, pseed)
    return m.eval()
