"""The Gaussian RAT-SPN leaf layer on the HIP path across the envelope of its kernels (tests/ratspn_gaussian_cases.py: which
case reaches which DIST = 0 route), against the oracle's leaf layer in float64.  Every call goes through model.base_layer
alone (GaussianLeafFn / LeafDropoutFn): no log-sum-exp sits above the leaf, so a leaf error cannot hide behind one.

Bars: LL_TOL = 1e-5 (tests.util.rel_err) on outputs; per gradient tensor grad_err(got, ref64) <= max(GRAD_TOL,
2 * grad_err(ref32, ref64)) with GRAD_TOL = 1e-4 -- the second term comes from the reference alone.  The parameter lists are
module constants: tests/test_ratspn_gaussian_host.py reads them for its route-coverage check."""
import functools

import numpy as np
import pytest
import torch

from tests import ratspn_gaussian_cases as gc
from tests.ratspn_gaussian_cases import LL_TOL, GRAD_TOL
from tests.util import rel_err, grad_err, report_measured, dropout_mask

pytestmark = pytest.mark.gpu

# ---- the parametrisations (read by the host test) -----------------------------------------------------------------------------
FWD_NAMES = [n for n in sorted(gc.CASES) if n != 'two_per_lane']
FWD_BATCHES = [1, 31, 33, 65, 300]           # the GEMM route's waves hold 32 samples, the VALU tiles 64 or 128
FWD_KINDS = ['clean', 'nan', 'huge', 'inf']
HINT_NAMES = ['mnist8', 'pad2', 'one']
HINT_BATCH = 65
MFMA_OFF_NAMES = ['mnist8', 'wide16_d1', 'ad4']
MFMA_OFF_BATCH = 65
TWO_PER_LANE = ('two_per_lane', 40000)

BWD_PAIRS = [('mnist8', 300), ('mnist8', 2048), ('wide16_d1', 300), ('ad4', 300), ('beyond_gemm', 300),   # moment kernel
             ('mnist8', 2049),                                              # the first batch on the 64-sample kernel
             ('pad2', 300), ('odd3', 300), ('one', 300), ('six', 300), ('many_groups', 1024),             # staged kernel
             ('pad2', 1100), ('odd3', 1100), ('six', 1100),                 # 64-sample kernel
             ('long_rows', 70),                                             # the non-staged 16-sample tile
             ('heavy_pad', 37)]                                             # d/dx with pad >= d
BWD_PARAMS = [pytest.param(name, variant, B, kind, sign, x_grad,
                           id='%s-%s-%d-%s-%s-%s' % (name, variant, B, kind, sign, 'dx' if x_grad else 'nodx'))
              for name, B in BWD_PAIRS for variant in gc.VARIANTS for kind in ('clean', 'nan')
              for sign in ('mixed', 'negative') for x_grad in (True, False) if x_grad or name != 'heavy_pad']
MISALIGNED_NAMES = ['mnist8', 'ad4']
MISALIGNED_BATCH = 300
MISALIGNED_WHAT = ['x', 'g', 'both']
ILL_NAMES = ['mnist8', 'ad4']
ILL_BATCHES = [512, 2048]
ILL_MODES = [('clean', 'mixed'), ('nan', 'negative')]
DROPOUT_NAMES = ['pad2', 'odd3', 'ad4']
DROPOUT_BATCHES = [70, 1100]
DROPOUT_RATE = 0.2


# ---- shared, unchanged once made ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_model(name, variant, regime='plain'):
    return gc.make_model(name, variant, regime)


@functools.lru_cache(maxsize=None)
def device_layer(name, variant, regime='plain'):
    return gc.make_model(name, variant, regime).cuda().base_layer


@functools.lru_cache(maxsize=None)
def state64(name, variant, regime='plain'):
    return gc.leaf_state(host_model(name, variant, regime))


@functools.lru_cache(maxsize=4)
def backward_reference(name, variant, B, kind, sign):
    """(x, g, ref64, ref32) of one backward case; the input gradient is always part of it."""
    st = state64(name, variant)
    x, g = gc.make_evidence(name, B, kind), gc.make_upstream(name, B, sign)
    return x, g, gc.reference_grads(st, x, g, torch.float64), gc.reference_grads(st, x, g, torch.float32)


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _aligned(*tensors):
    return all(t.data_ptr() % 16 == 0 for t in tensors)


def _on_mfma(layer, x, out):
    from deeprob.hip import load_library, DPK_FLAG_UNIT_SCALE
    flags = 0 if layer.scale.requires_grad else DPK_FLAG_UNIT_SCALE
    c = layer._leaf_ctx
    return bool(load_library().dpk_gaussian_leaf_forward_on_mfma(x.data_ptr(), out.data_ptr(), c.D, c.R, c.I, c.d, flags))


def _check_forward(tag, got, want):
    err = rel_err(got.cpu().numpy(), want)               # (asks for the same non-finite pattern)
    report_measured(tag, err, LL_TOL)
    assert err <= LL_TOL, (tag, err)


def _run_backward(layer, x, g, x_grad):
    """out = base_layer(x); out.backward(g): (out, {'loc', 'scale' (or None), 'x' (or None)}) on the host.  The operator's
    backward must be handed g itself (a copy would be aligned again: the misaligned cases would test nothing)."""
    layer.loc.grad = None
    layer.scale.grad = None
    xg = x.detach().requires_grad_(x_grad)
    with torch.enable_grad():
        out = layer(xg)
        handed = []
        out.register_hook(lambda grad: handed.append(grad.data_ptr()))
        out.backward(g)
    torch.cuda.synchronize()
    assert handed == [g.data_ptr()]
    grads = dict(loc=layer.loc.grad.cpu().numpy(),
                 scale=None if layer.scale.grad is None else layer.scale.grad.cpu().numpy(),
                 x=xg.grad.cpu().numpy() if x_grad else None)
    layer.loc.grad = None
    layer.scale.grad = None
    return out.detach(), grads


def _check_grads(tag, layer, variant, got, ref64, ref32, x_host):
    """The bar of this file on loc, scale and x; finite; x.grad == 0 at NaN entries; padded positions exactly 0."""
    assert (got['scale'] is None) == (variant == 'unit'), 'scale.grad must be None exactly for a frozen scale'
    pad = None
    if layer.pad > 0:
        pad = layer.pad_mask.cpu().expand(-1, layer.out_channels, -1).numpy()
    failed = []
    for k in ('loc', 'scale', 'x'):
        if got[k] is None:
            continue
        assert np.isfinite(got[k]).all(), (tag, k)
        own = grad_err(ref32[k], ref64[k])
        tol = max(GRAD_TOL, 2.0 * own)
        err = grad_err(got[k], ref64[k])
        report_measured('%s grad.%s vs fp64' % (tag, k), err, tol, '(oracle fp32 vs fp64 = %.2e)' % own)
        if err > tol:
            failed.append((k, err, tol))
        if k == 'x':
            assert (got['x'][torch.isnan(x_host).numpy()] == 0).all(), (tag, 'x.grad at marginalised entries')
        elif pad is not None:
            assert (got[k][pad] == 0).all(), (tag, k, 'gradient at a padded position')
    assert not failed, (tag, failed)


# ---- forward ----------------------------------------------------------------------------------------------------------------
def _slice_for(name, variant, B, kind, x):
    """Rows [lo:hi] whose evaluation alone must give the bits of the full batch, or None.  Both calls take the same route
    (forward_route of B and of hi - lo with the slice's own alignment).  Clean evidence: any rows -- no tile or wave leaves
    the fast path, and a sample's arithmetic does not depend on its lane.  Other evidence sends whole tiles (64 or 128
    samples of the VALU kernels) or waves (32 samples of the matrix-core route) to their exact paths, so only a slice made of
    whole tiles, [128:256], keeps every sample in the company it had; the compact-record kernel further picks one of two
    builds from what recent launches met, which no restatement of the dispatch predicts: left out."""
    if kind == 'clean':
        lo = min(5, B - 1)
        hi = max(lo + 1, B - 3)
    elif B >= 256:
        lo, hi = 128, 256
    else:
        return None
    part = x[lo:hi]
    full = gc.forward_route(name, variant, B, _aligned(x))
    if full != gc.forward_route(name, variant, hi - lo, _aligned(part)):
        return None
    if kind != 'clean' and full[0] == 'valu' and full[5]:
        return None
    return lo, hi


@pytest.mark.parametrize('kind', FWD_KINDS)
@pytest.mark.parametrize('B', FWD_BATCHES)
@pytest.mark.parametrize('variant', gc.VARIANTS)
@pytest.mark.parametrize('name', FWD_NAMES)
def test_leaf_forward_vs_float64(name, variant, B, kind):
    """The leaf layer's output against the float64 oracle (rows with +-inf evidence: the float32 oracle, see
    ratspn_gaussian_cases.forward_reference) with the same non-finite pattern; the all-NaN row gives exactly 0; a row slice
    gives the bits of the full batch (_slice_for); the library's own route answer is what forward_route predicts.  NaN
    evidence is evaluated twice: the second launch of the compact-record kernel may take its other build."""
    layer = device_layer(name, variant)
    x = gc.make_evidence(name, B, kind)
    want = gc.forward_reference(state64(name, variant), x)
    xc = x.cuda()
    tag = 'test_leaf_forward_vs_float64[%s-%s-%d-%s]' % (name, variant, B, kind)
    with torch.no_grad():
        got = layer(xc)
        torch.cuda.synchronize()      # (the hint that picks the next launch's build is read by the host without waiting)
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
        route = gc.forward_route(name, variant, B, _aligned(xc, got))
        assert _on_mfma(layer, xc, got) == (route[0] == 'gemm'), route
        _check_forward(tag, got, want)
        if kind in ('nan', 'inf'):
            assert (got[0] == 0).all(), 'the all-NaN row'
            again = layer(xc)
            torch.cuda.synchronize()
            _check_forward(tag + ' second launch', again, want)
            assert (again[0] == 0).all()
        rows = _slice_for(name, variant, B, kind, xc)
        if rows is not None:
            lo, hi = rows
            part = layer(xc[lo:hi])
            assert torch.equal(part, got[lo:hi]), 'rows %d:%d alone differ from the full batch' % (lo, hi)


@pytest.mark.parametrize('name', HINT_NAMES)
def test_leaf_forward_far_means_and_wrong_hint(name):
    """The unit variant (a) with 5 % of the means at +-8, beyond kExpandBound: those regions lose their eligibility and are
    evaluated exactly; (b) with scale overwritten by 0.5 + rand while requires_grad stays False: the unit-scale hint is then
    wrong, and the check on the device must catch it."""
    B = HINT_BATCH
    for kind in ('clean', 'nan'):
        x = gc.make_evidence(name, B, kind)
        xc = x.cuda()
        layer = device_layer(name, 'unit', 'far_means')
        with torch.no_grad():
            got = layer(xc)
        _check_forward('test_leaf_forward_far_means_and_wrong_hint[%s] far means, %s' % (name, kind), got,
                       gc.forward_reference(state64(name, 'unit', 'far_means'), x))

        model = gc.make_model(name, 'unit')
        with torch.no_grad():
            model.base_layer.scale.copy_(0.5 + torch.rand(model.base_layer.scale.shape, generator=torch.Generator().manual_seed(77)))
        assert not model.base_layer.scale.requires_grad
        st = gc.leaf_state(model)
        layer = model.cuda().base_layer
        with torch.no_grad():
            got = layer(xc)
            assert _on_mfma(layer, xc, got) == (gc.forward_route(name, 'unit', B, _aligned(xc, got))[0] == 'gemm')
        _check_forward('test_leaf_forward_far_means_and_wrong_hint[%s] wrong hint, %s' % (name, kind), got,
                       gc.forward_reference(st, x))


@pytest.mark.parametrize('name', MFMA_OFF_NAMES)
def test_leaf_forward_with_mfma_route_off(name):
    """dpk_ratspn_mfma_route(0): the VALU unit-scale kernels at CB 8 and 4 at shapes the matrix-core route normally takes;
    the same bar, and within LL_TOL of the matrix-core route's result."""
    from deeprob.hip import load_library
    lib = load_library()
    B = MFMA_OFF_BATCH
    layer = device_layer(name, 'unit')
    for kind in ('clean', 'nan'):
        x = gc.make_evidence(name, B, kind)
        want = gc.forward_reference(state64(name, 'unit'), x)
        xc = x.cuda()
        with torch.no_grad():
            on = layer(xc)
            assert _on_mfma(layer, xc, on)
            prev = lib.dpk_ratspn_mfma_route(0)
            try:
                off = layer(xc)
                assert not _on_mfma(layer, xc, off)
                torch.cuda.synchronize()
            finally:
                lib.dpk_ratspn_mfma_route(prev)
        assert gc.forward_route(name, 'unit', B, mfma=False)[0] == 'valu'
        tag = 'test_leaf_forward_with_mfma_route_off[%s] %s' % (name, kind)
        _check_forward(tag + ' vs fp64', off, want)
        _check_forward(tag + ' vs the GEMM route', off, on.cpu().numpy().astype(np.float64))


@pytest.mark.parametrize('variant', gc.VARIANTS)
def test_leaf_forward_two_samples_per_lane(variant):
    """40000 samples > 32768: 'scaled' takes the 8-channel blocks with two samples per lane ('unit' stays on the matrix
    cores).  A scattered subset against float64, and the first 300 rows evaluated alone (one sample per lane) against the
    full launch -- to LL_TOL, not bit for bit: the two mappings sum in different orders."""
    name, B = TWO_PER_LANE
    layer = device_layer(name, variant)
    x = gc.make_evidence(name, B, 'nan')
    rows = torch.randint(0, B, (512,), generator=torch.Generator().manual_seed(8))
    rows[:6] = torch.tensor([0, 1, 63, 64, B - 2, B - 1])
    want = gc.forward_reference(state64(name, variant), x[rows])
    xc = x.cuda()
    with torch.no_grad():
        big = layer(xc)
        small = layer(xc[:300])
    tag = 'test_leaf_forward_two_samples_per_lane[%s]' % variant
    _check_forward(tag + ' 512 rows vs fp64', big[rows.cuda()], want)
    assert (big[0] == 0).all()
    _check_forward(tag + ' first 300 rows alone vs the full launch', small, big[:300].cpu().numpy().astype(np.float64))


# ---- backward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,variant,B,kind,sign,x_grad', BWD_PARAMS)
def test_leaf_backward_vs_float64(name, variant, B, kind, sign, x_grad):
    """out = base_layer(x); out.backward(g): d/dloc, d/dscale ('scaled') and d/dx against float64 autograd of the oracle's leaf
    layer, marginalised terms cut out of the graph."""
    layer = device_layer(name, variant)
    x, g, ref64, ref32 = backward_reference(name, variant, B, kind, sign)
    tag = 'test_leaf_backward_vs_float64[%s-%s-%d-%s-%s-%s]' % (name, variant, B, kind, sign, 'dx' if x_grad else 'nodx')
    if name == 'many_groups':       # (the staged kernel's passes follow the device's compute units: the host test assumes 256)
        assert gc.backward_route(name, variant, B, variant == 'scaled', cus=_cus()) == ('staged', 1, variant == 'scaled', 4)
    out, got = _run_backward(layer, x.cuda(), g.cuda(), x_grad)
    _check_forward(tag + ' out', out, ref64['out'])
    _check_grads(tag, layer, variant, got, ref64, ref32, x)


@pytest.mark.parametrize('what', MISALIGNED_WHAT)
@pytest.mark.parametrize('name', MISALIGNED_NAMES)
def test_leaf_backward_misaligned_operands(name, what):
    """x and / or g as contiguous views at storage offset 1 of a larger buffer, 4-byte aligned only.  'x': the moment kernel
    takes its scalar x path.  'g': the moment kernel is declined -- mnist8 reaches the staged kernel with CBK 4, ad4 (whose
    16 rows of D + 4 R floats exceed 80 KB) the 16-sample kernel with CBK 4.  'both': the staged kernel is declined too.  The
    bar of test_leaf_backward_vs_float64, and agreement with the aligned call to 2e-5 of the tensor's largest magnitude: the
    bar of test_leaf_parameter_gradients_of_a_batch_are_the_sum_over_its_halves, which compares two summation orders of the
    same fp32 terms."""
    B, variant = MISALIGNED_BATCH, 'scaled'
    layer = device_layer(name, variant)
    x, g, ref64, ref32 = backward_reference(name, variant, B, 'nan', 'mixed')
    xc, gd = x.cuda(), g.cuda()
    assert _aligned(xc, gd)
    _, base = _run_backward(layer, xc, gd, True)
    xm = gc.misaligned(xc) if what in ('x', 'both') else xc
    gm = gc.misaligned(gd) if what in ('g', 'both') else gd
    assert _aligned(xm) == (what == 'g') and _aligned(gm) == (what == 'x')
    tag = 'test_leaf_backward_misaligned_operands[%s-%s]' % (name, what)
    out, got = _run_backward(layer, xm, gm, True)
    _check_forward(tag + ' out', out, ref64['out'])
    _check_grads(tag, layer, variant, got, ref64, ref32, x)
    for k in ('loc', 'scale', 'x'):
        top = np.abs(base[k]).max()
        diff = np.abs(got[k] - base[k]).max() / top
        report_measured('%s grad.%s vs the aligned call' % (tag, k), diff, 2e-5)
        assert top > 0 and diff <= 2e-5, (k, diff)


@pytest.mark.parametrize('kind,sign', ILL_MODES)
@pytest.mark.parametrize('B', ILL_BATCHES)
@pytest.mark.parametrize('regime', gc.ILL_REGIMES)
@pytest.mark.parametrize('name', ILL_NAMES)
def test_leaf_backward_ill_conditioned_mixed_sign(name, regime, B, kind, sign):
    """The moment kernel on data where the raw moments cancel (|mu| / s large), with an upstream gradient of mixed sign, and
    with a one-signed one on marginalised evidence: both take the `mixed` branch of the per-tile conditioning detector, which
    no whole-model test reaches on such data (a loss hands down one sign)."""
    model, x = gc.make_ill_case(name, regime, B, kind)
    st = gc.leaf_state(model)
    g = gc.make_upstream(name, B, sign)
    ref64, ref32 = gc.reference_grads(st, x, g, torch.float64), gc.reference_grads(st, x, g, torch.float32)
    assert gc.backward_route(name, 'scaled', B, True) == ('moment', True)
    layer = model.cuda().base_layer
    tag = 'test_leaf_backward_ill_conditioned_mixed_sign[%s-%s-%d-%s-%s]' % (name, regime, B, kind, sign)
    out, got = _run_backward(layer, x.cuda(), g.cuda(), True)
    _check_forward(tag + ' out', out, ref64['out'])
    _check_grads(tag, layer, 'scaled', got, ref64, ref32, x)


class _Seeds:
    """Replaces deeprob.hip.ops.draw_seed, as in test_dropout_gpu.py: hands out a fixed sequence and records it."""

    def __init__(self, start=7654321):
        self.next = start
        self.used = []

    def __call__(self):
        self.used.append(self.next)
        self.next += 1000003
        return self.used[-1]


@pytest.mark.parametrize('B', DROPOUT_BATCHES)
@pytest.mark.parametrize('name', DROPOUT_NAMES)
def test_leaf_dropout_backward_channel_blocks(name, B, monkeypatch):
    """base_layer.train() with input dropout 0.2 (LeafDropoutFn): the mask rebuilt from the pinned seed and fed to the
    oracle's drop=.  Dropout keeps the parameter gradients on leaf_bwd_param_kernel: CBK 2, 1 and 4 on the 16-sample tile
    (B = 70) and on the 64-sample tile (B = 1100)."""
    from deeprob.hip import ops
    seeds = _Seeds()
    monkeypatch.setattr(ops, 'draw_seed', seeds)
    variant = 'scaled'
    model = gc.make_model(name, variant)
    st = gc.leaf_state(model)
    layer = model.cuda().base_layer
    _, R, I, d, _ = gc.geometry(name)
    x, g = gc.make_evidence(name, B, 'nan'), gc.make_upstream(name, B, 'mixed')
    layer.dropout = DROPOUT_RATE
    layer.train()
    out, got = _run_backward(layer, x.cuda(), g.cuda(), True)
    assert len(seeds.used) == 1
    drop = dropout_mask(seeds.used[0], (B, R, I, d), DROPOUT_RATE)
    ref64 = gc.reference_grads(st, x, g, torch.float64, drop=drop)
    ref32 = gc.reference_grads(st, x, g, torch.float32, drop=drop)
    tag = 'test_leaf_dropout_backward_channel_blocks[%s-%d]' % (name, B)
    assert gc.backward_route(name, variant, B, True, dropout=True) == ('plain', {2: 2, 3: 1, 4: 4}[I], 16 if B <= 1024 else 64)
    _check_forward(tag + ' out', out, ref64['out'])
    _check_grads(tag, layer, variant, got, ref64, ref32, x)
