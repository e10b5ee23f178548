"""The slice kernel's K-step after its f16 split went to one v_fma_mix_f32 per low half (split8_mix,
csrc/ratspn_gemm_common.h): per-sample log-likelihoods held, BIT for bit, to what the build before that change computed.

The fixtures (tests/golden/slice_kstep_bits.npz, written by tools/record_slice_kstep_golden.py from that earlier build on
an MI355X) are the outputs of the headline model on seeded inputs, on the slice mapping forced at small batches:
B = 33 (a ragged last block), 96 and 257 (several work-groups, a ragged one), and 577 samples stated to run on 15 lanes
(a share of 17 compute units: 19 blocks on 10 work-groups, so that work-groups walk a SECOND block -- the steady K loop; at
the smaller sizes every work-group has one block, the unrolled first-block loop), each with
  normal   N(0, 1);
  tiny     magnitudes 1e-6 .. 1e-4 (f16 subnormals: the mixed instruction reads its f16 operand under the f16 denormal mode)
           with zeros of both signs mixed in;
  edge     N(0, 1) with entries of +-999 (the envelope's edge, |x| <= 1e3), at most one per K-step's 8 values of a sample so
           that the K-step stays under its bound and on the fast path, and two rows of 999 throughout (these leave it);
  special  N(0, 1) with one row holding NaNs and one holding +inf: the exact route, which never enters the split.
in frozen and in default mode.  x - float(rn16(x)) is exact in fp32 whichever instruction forms it, so nothing may move."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'slice_kstep_bits.npz')
D = 784
BATCHES = [33, 96, 257, 577]
LANES = {577: 15}                     # (stated lane count of a size's plan; not listed: nothing stated, the whole chip)
KINDS = ['normal', 'tiny', 'edge', 'special']
MODES = ['frozen', 'default']


def inputs(kind, B):
    """The seeded input of a case (host tensor, float32)."""
    g = torch.Generator().manual_seed(1000 * KINDS.index(kind) + B)
    x = torch.randn(B, D, generator=g)
    if kind == 'tiny':
        mag = 10.0 ** (-6.0 + 2.0 * torch.rand(B, D, generator=g))            # 1e-6 .. 1e-4
        sign = torch.where(torch.rand(B, D, generator=g) < 0.5, -1.0, 1.0)
        x = (mag * sign).float()
        pick = torch.rand(B, D, generator=g)
        x[pick < 0.10] = 0.0
        x[(pick >= 0.10) & (pick < 0.20)] = -0.0
        x[0, :8] = torch.tensor([6.1e-5, -6.1e-5, 6.2e-5, 5.96e-8, -5.96e-8, 2.9e-8, 1e-40, -1e-40])   # (around the f16 normal / subnormal edges)
    elif kind == 'edge':
        col = torch.randint(0, 8, (B, D // 8), generator=g)                   # one entry per group of 8 values
        on = torch.rand(B, D // 8, generator=g) < 0.25
        sign = torch.where(torch.rand(B, D // 8, generator=g) < 0.5, -999.0, 999.0)
        xg = x.view(B, D // 8, 8)
        rows, groups = torch.nonzero(on, as_tuple=True)
        xg[rows, groups, col[rows, groups]] = sign[rows, groups]
        x[5, :] = 999.0
        x[B - 1, :] = -999.0
    elif kind == 'special':
        x[3, 100:140] = float('nan')
        x[B - 2, 17] = float('inf')
    return x.contiguous()


def evaluate(kind, B, mode):
    """(first launch of a fresh model's plan, a second launch of it or None) as host int32 bit patterns.  A NaN in the
    first launch moves later ones to the mapping built for marginalised evidence: no second launch there."""
    from deeprob.spn.models import GaussianRatSpn
    torch.manual_seed(0)
    model = GaussianRatSpn(D, rg_depth=2, rg_repetitions=8, rg_batch=2, rg_sum=2, random_state=42).eval().cuda()
    x = inputs(kind, B).cuda()
    with torch.no_grad():
        plan = model.fused_plan(x, static_params=(mode == 'frozen'), lanes=LANES.get(B))
        assert plan is not None
        first = plan.out.clone()
        again = None if kind == 'special' else plan.run().clone()
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int32).cpu().numpy()
    return bits(first), (None if again is None else bits(again))


def CUS():
    return torch.cuda.get_device_properties(0).multi_processor_count


def key(kind, B, mode):
    return '{}_{}_{}'.format(kind, B, mode)


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture
def slice_everywhere():
    from deeprob.hip import load_library, slice as sl
    lib = load_library()
    prev = lib.dpk_ratspn_slice_batch_min(0)
    prev_lanes = sl.lanes(0)
    yield sl
    sl.lanes(prev_lanes)
    lib.dpk_ratspn_slice_batch_min(prev)


@pytest.mark.gpu
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kind', KINDS)
def test_bits_of_the_build_before_the_mixed_split(slice_everywhere, golden, kind, mode, B):
    sl = slice_everywhere
    want = golden[key(kind, B, mode)]
    first, again = evaluate(kind, B, mode)
    lanes = LANES.get(B, 1)                                              # (the slice mapping ran, on the grid of its share)
    assert sl.last_lanes() == lanes and sl.last_grid() in (sl.grid(-(-B // 32), CUS(), lanes, 0), sl.grid(-(-B // 32), CUS(), lanes, 13))
    assert want.shape == first.shape == (B, 1)
    diff = np.nonzero(first != want)[0]
    assert diff.size == 0, (kind, mode, B, diff[:8], first[diff[:8], 0], want[diff[:8], 0])
    if again is not None:
        assert np.array_equal(again, want), (kind, mode, B)
    ll = torch.from_numpy(first.copy()).view(torch.float32)
    if kind == 'special':
        assert torch.isfinite(ll[3]).all()                               # (NaN entries are marginalised)
    elif kind != 'edge':
        assert torch.isfinite(ll).all()


def test_inputs_cover_what_they_claim():
    """(host only) the generated inputs hold f16 subnormals, both zeros, the envelope's edge under the K-step bound."""
    t = inputs('tiny', 96)
    assert ((t.abs() > 0) & (t.abs() < 6.1e-5)).any() and (t.abs() <= 1.01e-4).all()
    z = t[t == 0].view(torch.int32)
    assert (z == 0).any() and (z != 0).any()
    e = inputs('edge', 96)
    body = torch.cat([e[:5], e[6:-1]])
    assert (body.abs() == 999.0).any() and body.abs().max() == 999.0
    assert (body.view(-1, 8).pow(2).sum(1) < 1.0e6).all() and (e[5] == 999.0).all() and (e[-1] == -999.0).all()
    s = inputs('special', 33)
    assert torch.isnan(s[3]).sum() == 40 and torch.isinf(s[31]).sum() == 1
