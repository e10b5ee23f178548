"""The reference of tests/test_ratspn_level_backward_gpu.py (tests/ratspn_level_ref.py), pinned on the host before any device
run: the closed form IS float64 autograd through the oracle's layers wherever autograd is defined, and where it is not -- a
sum node all of whose inputs are -inf -- it states this project's convention: such a node passes no gradient, neither to its
inputs (exactly 0) nor to its weights.  torch's logsumexp backward returns NaN there, for the dead inputs and for EVERY weight
of the node (one sample's NaN is summed over the batch) -- the whole weight tensor of a root."""
import numpy as np
import pytest
import torch

from oracle import ratspn_oracle as orc
from tests import ratspn_level_ref as ref
from tests.util import grad_err, rel_err

# kind, P, N, S, B: every kind, one / several partitions, N = 2 (two live weights have exactly two places to be) ... 16
SHAPES = [('sum', 3, 2, 2, 9), ('sum', 3, 8, 8, 9), ('sum', 2, 16, 8, 6), ('root', 5, 4, 9, 9), ('root', 3, 2, 1, 9),
          ('sum_layer', 3, 9, 5, 9), ('root_layer', 1, 70, 3, 9)]
EXACT = 1e-12      # float64 against float64: two orders of summation of the same terms


def oracle_autograd(kind, x, w, g):
    """(out, gx, gW) by float64 autograd through oracle.ratspn_oracle's layers."""
    x = x.double().clone().requires_grad_(True)
    w = w.double().clone().requires_grad_(True)
    with torch.enable_grad():
        h = orc.product_layer(x) if kind in ('sum', 'root') else x
        out = orc.root_layer(h, w) if kind in ('root', 'root_layer') else orc.sum_layer(h, w)
        gx, gw = torch.autograd.grad(out, [x, w], g.double())
    return out.detach().numpy(), gx.numpy(), gw.numpy()


def closed_form(kind, x, w, g):
    fn = {'sum': lambda: ref.level(x, w, g, False), 'root': lambda: ref.level(x, w, g, True),
          'sum_layer': lambda: ref.sum_layer(x, w, g), 'root_layer': lambda: ref.root_layer(x, w, g)}[kind]
    return tuple(t.numpy() for t in fn())


@pytest.mark.parametrize('regime', ['plain', 'offset', 'two_live'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '-'.join(map(str, s)))
def test_closed_form_is_oracle_autograd(shape, regime):
    kind = shape[0]
    x, w, g = ref.make_inputs(*shape, regime)
    want = oracle_autograd(kind, x, w, g)
    got = closed_form(kind, x, w, g)
    assert rel_err(got[0], want[0]) <= EXACT
    assert grad_err(got[1], want[1]) <= EXACT
    assert grad_err(got[2], want[2]) <= EXACT
    assert np.abs(want[2]).max() > 1e-3              # (a weight gradient to speak of: not the single-live-weight zero)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '-'.join(map(str, s)))
def test_regimes_are_what_they_say(shape):
    kind, P, N, S, B = shape
    lvl = kind in ('sum', 'root')
    x, w, g = ref.make_inputs(*shape, 'offset')
    out = closed_form(kind, x, w, g)[0].reshape(B, -1)
    for b in range(B):
        assert np.abs(out[b] - ref.OFFSETS[b % 4]).max() < 60.0
    x, w, g = ref.make_inputs(*shape, 'two_live')
    rows = w.reshape(-1, w.shape[-1])
    assert ((rows == 0).sum(1) == 1).all() and ((rows == -1).sum(1) == 1).all() and ((rows == -200).sum(1) == rows.shape[1] - 2).all()
    # the +60 node of sample 0 sits under dead weights only: the inputs of a partition that see it are the first N / first one
    n_in = N * N if lvl else N
    cols = torch.arange(rows.shape[1]) % n_in < (N if lvl else 1)
    assert (rows[:, cols] == -200).all() and (x[0] == 60).sum() == P and ((x[0] < -30) & (x[0] > -70)).sum() == x[0].numel() - P
    x, w, g = ref.make_inputs(*shape, 'dead')
    assert (x[0, 0] == float('-inf')).all() and (x[1, :, 0] == float('-inf')).all() and (x[2] == -1.0e4).all()
    assert torch.isfinite(x[3:]).all() and torch.isfinite(x[1, :, 1:]).all()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '-'.join(map(str, s)))
def test_dead_region_convention(shape):
    """x[0, 0, :] = -inf.  Autograd: NaN.  Closed form: exactly 0 for the dead inputs, finite everywhere, and the gradient
    of the same function with the dead nodes' incoming gradient set to 0 (-1e300 in place of -inf keeps autograd defined:
    exp(-1e300 - anything) is exactly 0 as well)."""
    kind = shape[0]
    x, w, g = ref.make_inputs(*shape, 'dead')
    _, ax, aw = oracle_autograd(kind, x, w, g)
    mask = ref.dead_input_mask(x, kind).numpy()
    assert mask[0, 0].all() and not mask[1:].any()
    out, gx, gW = closed_form(kind, x, w, g)
    dead_out = np.isneginf(out)
    if dead_out.any():       # a sum node died (the root of a level with several partitions lives on through the others)
        assert np.isnan(ax[0, 0]).all() and np.isnan(aw if aw.ndim == 2 else aw[0]).all()
    assert np.isfinite(gx).all() and np.isfinite(gW).all()
    assert (gx[mask] == 0.0).all()
    x2 = torch.where(torch.from_numpy(mask), torch.full_like(x, -1e300, dtype=torch.float64), x.double())
    g2 = torch.where(torch.from_numpy(dead_out), torch.zeros((), dtype=torch.float64), g.double())
    o2, ax2, aw2 = oracle_autograd(kind, x2, w, g2)
    assert np.isfinite(ax2).all() and np.isfinite(aw2).all()
    assert rel_err(out[~dead_out], o2[~dead_out]) <= EXACT
    assert grad_err(gx, ax2) <= EXACT and (ax2[mask] == 0.0).all()
    assert grad_err(gW, aw2) <= EXACT
    # the rest of the dead sample, entry for entry (not only against the tensor's largest magnitude)
    rest = ~mask[0]
    assert np.allclose(gx[0][rest], ax2[0][rest], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '-'.join(map(str, s)))
def test_single_dead_nodes_agree_with_autograd(shape):
    """x[b, :, 0] = -inf (node 0 of every region): every sum node keeps live inputs, autograd is defined and agrees."""
    kind = shape[0]
    x, w, g = ref.make_inputs(*shape, 'dead')
    x, g = x[1:2].contiguous(), g[1:2].contiguous()
    want = oracle_autograd(kind, x, w, g)
    got = closed_form(kind, x, w, g)
    assert np.isfinite(want[1]).all() and np.isfinite(want[2]).all()
    assert rel_err(got[0], want[0]) <= EXACT
    assert grad_err(got[1], want[1]) <= EXACT and grad_err(got[2], want[2]) <= EXACT
    assert (got[1][0, :, 0] == 0.0).all() and (want[1][0, :, 0] == 0.0).all()


@pytest.mark.parametrize('N', [3, 5, 32])
def test_product_backward_is_oracle_autograd(N):
    gen = torch.Generator().manual_seed(N)
    gp = torch.randn(5, 3, N * N, generator=gen)
    x = torch.zeros(5, 6, N, dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():
        want, = torch.autograd.grad(orc.product_layer(x), [x], gp.double())
    assert grad_err(ref.product_backward(gp, N).numpy(), want.numpy()) <= EXACT


def test_reference_is_cached_and_read_only():
    a = ref.reference('sum', 3, 2, 2, 9, 'offset')
    assert ref.reference('sum', 3, 2, 2, 9, 'offset') is a
    assert not a[3]['gx'].flags.writeable
    # the float32 evaluation of the plain formula loses the offset regime's gradients to the rounding of `out` (half an ulp
    # of 1e4 is 5e-4): the distance the device kernels are measured next to
    assert 1e-5 < a[4]['gx'] < 2e-3 and ref.reference('sum', 3, 2, 2, 9, 'plain')[4]['gx'] < 1e-5
