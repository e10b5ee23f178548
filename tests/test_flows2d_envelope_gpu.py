"""The RealNVP-2D evaluation kernels (csrc/flows2d.hip) driven one by one across the shapes where dpk_conv2d_forward
changes hands, against float64 restatements on the CPU.

Convolutions: every row of tests/flows2d_cases.py::CASES (tests/test_flows2d_envelope_host.py proves which template
instance each one reaches) against `conv_ref`, tests.util.rel_err <= 1e-5, the parity bar of the project; a row that
exceeded it by rounding alone would be held to four times the error of torch's own fp32 CPU convolution instead and say so
in its record.  The routes behind DPK_CONV_MFMA3 / DPK_CONV_VALU / DPK_CONV_LDS are read once per process and run in a child
(tests/_conv2d_route_cases.py).  The small kernels (coupling2d, bn2d bijector, space-to-depth) through the C ABI.

Every measured error is recorded with report_measured (group E: convolution rows, S: switched routes, K: small kernels).

No test asserts which route ran: they assert results at shapes where the code, as written, takes it."""
import functools
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util import rel_err, report_measured
from tests import flows2d_cases as fc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BAR = 1e-5
U = 2.0 ** -24            # unit roundoff of fp32


@functools.lru_cache(maxsize=None)
def _evaluated(name):
    """(case, inputs, device result on the CPU, whole output buffer on the CPU or None), computed once per row."""
    case = fc.BY_NAME[name]
    inp = fc.make_inputs(case)
    got, whole = fc.run(case, inp, DEV)
    return case, inp, got.cpu(), None if whole is None else whole.cpu()


# ---- convolutions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c.name for c in fc.CASES])
def test_row_against_float64(name):
    case, inp, got, _ = _evaluated(name)
    err, bound, note = fc.check_row(case, inp, got)
    print('{}: rel_err {:.3e} bound {:.3e} {}'.format(name, err, bound, note))
    report_measured('E %s [%s]' % (name, fc.instantiation(case)), err, bound, note)
    assert err <= bound, (name, err, bound)


@pytest.mark.parametrize('name', [c.name for c in fc.CASES if c.sliced])
def test_outside_of_the_output_slice_is_bit_unchanged(name):
    """One sliced row per route: the buffer around the output slice was pre-filled with a sentinel; the channels in front
    of and behind the slice hold its bits afterwards, in every sample."""
    case, _, got, whole = _evaluated(name)
    lo = fc.PADS['out'][0]
    assert whole.shape[1] == case.Cout + sum(fc.PADS['out']) and torch.equal(whole[:, lo:lo + case.Cout], got)
    assert not bool((got == fc.SENTINEL).any())
    assert fc.outside_untouched(case, whole)


@pytest.mark.parametrize('name,rows', [('lds_6x6_b30_g28', (1, 29)), ('lds_6x6_b30_g28', (28, 30)),
                                       ('lds_16x16_b9_g4', (3, 7)), ('mfma_px257', (0, 1)),
                                       ('mfma_px189_slices', (1, 3))])
def test_batch_independence(name, rows):
    """Samples k .. k+G evaluated alone give the same bits as inside the batch: the LDS route groups G samples per
    work-group (other groups, another tile count alone), the MFMA route cuts the flattened [B, H*W] axis into 64-pixel runs
    (a sample starts in the middle of one)."""
    case, inp, full, _ = _evaluated(name)
    alone, _ = fc.run(case, inp, DEV, rows=slice(*rows))
    assert alone.shape[0] == rows[1] - rows[0]
    assert torch.equal(alone.cpu(), full[rows[0]:rows[1]])


@pytest.mark.parametrize('name', ['lds_7x9_cin9', 'lds_7x9_cin9_fold'])
def test_lds_padded_channels_are_zeros_not_copies(name):
    """Cin = 9: the last staged chunk of conv3x3_lds_kernel holds one real channel and three padded ones, which it must
    write as ZEROS.  On finite data the zero-filled weights of a padded channel hide a copy of channel Cin - 1 in its place
    (x * 0 = 0); an infinite activation in that channel does not (inf * 0 = NaN): the nine outputs per channel that see it
    are +-inf with the sign of their weight, as in float64, and everything else is unchanged."""
    case, inp, clean, _ = _evaluated(name)
    b, ci, y, x = 2, case.Cin - 1, 3, 4
    hot = dict(inp, x=inp['x'].clone())
    hot['x'][b, ci, y, x] = float('inf')
    got, _ = fc.run(case, hot, DEV)
    cold = dict(inp, x=inp['x'].clone())
    cold['x'][b, ci, y, x] = 0.0
    want = fc.reference(case, cold)
    # (the fold maps +inf to +inf: its scale is positive)
    w = inp['v'].double() * inp['g'].double()
    for ky in range(3):
        for kx in range(3):
            want[b, :, y + 1 - ky, x + 1 - kx] = torch.sign(w[:, ci, ky, kx]) * float('inf')
    assert int(torch.isinf(want).sum()) == 9 * case.Cout
    assert rel_err(got.cpu().numpy(), want.numpy()) <= BAR
    finite = torch.isfinite(want)
    assert torch.equal(got.cpu()[finite], clean[finite])


def test_routes_behind_the_environment_switches():
    """conv2d_mfma_kernel<3, *> (DPK_CONV_MFMA3=1), conv2d_kernel on the wide layers (DPK_CONV_VALU=1) and on the wide 3x3
    layers of at most 1024 pixels (DPK_CONV_LDS=0): one child process per switch, one after the other; the first child that
    exits non-zero ends the test and no further one is started."""
    from tests import _conv2d_route_cases as rc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = {k: v for k, v in os.environ.items() if k not in fc.SWITCH_ROWS}
    base['PYTHONPATH'] = os.pathsep.join([os.path.join(root, 'deeprob-kit_amd'), root, os.environ.get('PYTHONPATH', '')])
    for var, (value, _, names) in fc.SWITCH_ROWS.items():
        r = subprocess.run([sys.executable, '-X', 'faulthandler', '-m', 'tests._conv2d_route_cases'], cwd=root,
                           env=dict(base, **{var: value}), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
        out, err = r.stdout.decode(errors='replace'), r.stderr.decode(errors='replace')
        lines = [l for l in out.splitlines() if l.startswith(rc.MARK)]
        assert r.returncode == 0 and len(lines) == 1, '{}={}: child failed (rc {}):\n{}\n{}'.format(
            var, value, r.returncode, out[-2000:], err[-4000:])
        got = json.loads(lines[0][len(rc.MARK):])
        assert got['switch'] == var and sorted(got['errors']) == sorted(names)
        for name, (e, bound) in got['errors'].items():
            report_measured('S %s=%s %s [%s]' % (var, value, name, fc.instantiation(fc.BY_NAME[name], {var: value})), e, bound,
                            '' if bound == BAR else 'above 1e-5: bound = 4 x the error of fp32 CPU F.conv2d')
        bad = {n: eb for n, eb in got['errors'].items() if not eb[0] <= eb[1]}
        assert not bad, (var, bad)


# ---- small kernels through the C ABI ----------------------------------------------------------------------------------------
def _abi():
    from deeprob.hip import load_library, call, ptr, stream_ptr
    return load_library(), call, ptr, stream_ptr(DEV)


def _checker(H, W):
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    return ((yy + xx) % 2).float().reshape(-1)


def _coupling_ref(x, z, scale, inv_mask, affine, reverse, inverse, ldj_in):
    """float64: (out, ldj, sum |s| per sample).  Checkerboard: t, s masked by inv_mask on all C channels; channel-wise: the
    first half of the channels is transformed (reverse: the second), conditioned on z, the other half passes through."""
    x, z = x.double(), z.double()
    B, C, H, W = x.shape
    chw = inv_mask is None
    Ch = C // 2 if chw else C
    m = 1.0 if chw else inv_mask.double().reshape(1, 1, H, W)
    t = z[:, :Ch] * m
    s = scale.double().reshape(1, Ch, 1, 1) * torch.tanh(z[:, Ch:]) * m if affine else torch.zeros_like(t)
    sel = slice(None) if not chw else (slice(Ch, C) if reverse else slice(0, Ch))
    out = x.clone()
    out[:, sel] = x[:, sel] * torch.exp(s) + t if inverse else (x[:, sel] - t) * torch.exp(-s)
    tot = s.sum(dim=(1, 2, 3))
    ldj = (0.0 if ldj_in is None else ldj_in.double()) + (tot if inverse else -tot)
    return out, ldj, s.abs().sum(dim=(1, 2, 3))


def _coupling(x, z, scale, inv_mask, affine, reverse, inverse, ldj_in):
    lib, call, ptr, st = _abi()
    B, C, H, W = x.shape
    out = torch.full_like(x, fc.SENTINEL)
    ldj = torch.full((B,), fc.SENTINEL, device=DEV)
    call(lib.dpk_coupling2d_transform, ptr(x), ptr(z), ptr(scale), ptr(inv_mask), B, C, H, W, int(affine), int(reverse),
         int(inverse), ptr(ldj_in), ptr(out), ptr(ldj), st)
    torch.cuda.synchronize()
    return out, ldj


def _sum_bound(terms_per_thread, abs_sum, ldj_in, total, term_ulps=8):
    """Forward-error bound of an fp32 sum as the kernels form it: every term carries `term_ulps` ulps (2 U each) of its own,
    a thread adds `terms_per_thread` of them in turn, nine more additions join the partial sums, one adds ldj_in."""
    carry = 0.0 if ldj_in is None else np.abs(ldj_in.double().cpu().numpy())
    return U * ((terms_per_thread + 9 + 2 * term_ulps) * abs_sum + 2.0 * (carry + np.abs(total)))


@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('shape', [(2, 1, 1), (4, 3, 5), (6, 7, 9), (12, 16, 16)], ids=lambda s: 'x'.join(map(str, s)))
def test_coupling2d_transform(shape, B):
    """dpk_coupling2d_transform: checkerboard and channel-wise (both halves), additive and affine, both directions, with and
    without an incoming log-determinant.  u / x at the parity bar; the log-determinant under the forward-error bound of its
    fp32 sum (`_sum_bound`); the channel-wise pass-through half bit-equal; inverse(forward(x)) = x within 1e-6 max|x|.
    Element counts per sample: 1, 2, 30 .. 3072 (none but the last a multiple of 256)."""
    C, H, W = shape
    g = torch.Generator().manual_seed(1000 * B + C * H * W)
    x = torch.randn(B, C, H, W, generator=g).to(DEV)
    ldj0 = torch.randn(B, generator=g).to(DEV)
    failed = []
    for chw, reverse, affine in itertools.product((False, True), (False, True), (False, True)):
        if reverse and not chw:
            continue                      # (reverse orders the halves of the channel-wise coupling only)
        Ch = C // 2 if chw else C
        z = (0.5 * torch.randn(B, (2 if affine else 1) * Ch, H, W, generator=g)).to(DEV)
        scale = (0.2 + 0.3 * torch.rand(Ch, generator=g)).to(DEV) if affine else None
        inv_mask = None if chw else _checker(H, W).to(DEV)
        tag = 'coupling2d %s B=%d %s%s %s' % ('x'.join(map(str, shape)), B, 'channel-wise' if chw else 'checkerboard',
                                              ' reverse' if reverse else '', 'affine' if affine else 'additive')
        worst_out = worst_ldj = 0.0
        for inverse, ldj_in in itertools.product((False, True), (None, ldj0)):
            out, ldj = _coupling(x, z, scale, inv_mask, affine, reverse, inverse, ldj_in)
            want, want_ldj, abs_s = _coupling_ref(x.cpu(), z.cpu(), None if scale is None else scale.cpu(),
                                                  None if chw else inv_mask.cpu(), affine, reverse, inverse,
                                                  None if ldj_in is None else ldj_in.cpu())
            name = '%s %s%s' % (tag, 'inverse' if inverse else 'density', '' if ldj_in is None else ' +ldj')
            e = rel_err(out.cpu().numpy(), want.numpy())
            bound = _sum_bound(-(-(Ch * H * W) // 256), abs_s.numpy(), ldj_in, want_ldj.numpy())
            el = np.abs(ldj.cpu().double().numpy() - want_ldj.numpy())
            # (additive without an incoming value: the bound is 0 and the result must be exactly 0)
            ratio = float(np.max(np.where(el <= bound, el / np.maximum(bound, 1e-300), np.inf)))
            worst_out, worst_ldj = max(worst_out, e), max(worst_ldj, ratio)
            if not e <= BAR or not ratio <= 1.0:
                failed.append((name, e, el.tolist(), bound.tolist()))
            if chw:
                keep = slice(0, Ch) if reverse else slice(Ch, C)
                assert torch.equal(out[:, keep], x[:, keep]), name + ': pass-through half'
            else:       # t = s = 0 where the mask is 0: those pixels pass through
                still = (inv_mask == 0).reshape(1, 1, H, W).expand_as(x)
                assert torch.equal(out[still], x[still]), name + ': masked pixels'
        report_measured('K ' + tag + ' out, worst of 4 calls', worst_out, BAR)
        report_measured('K ' + tag + ' ldj |err| / fp32 sum bound, worst of 4 calls', worst_ldj, 1.0)
        # round trip: the sampling direction applied to the density direction's result
        u, l1 = _coupling(x, z, scale, inv_mask, affine, reverse, False, ldj0)
        back, l2 = _coupling(u, z, scale, inv_mask, affine, reverse, True, l1)
        rt = float((back - x).abs().max()) / float(x.abs().max())
        report_measured('K ' + tag + ' round trip / max|x|', rt, 1e-6)
        if not rt <= 1e-6:
            failed.append((tag + ' round trip', rt))
    assert not failed, failed


@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('shape', [(2, 1, 1), (4, 3, 5), (6, 7, 9), (12, 16, 16)], ids=lambda s: 'x'.join(map(str, s)))
def test_bn2d_bijector(shape, B):
    """dpk_bn2d_bijector in both directions: u / x at the parity bar, the log-determinant against
    HW * sum(w - 0.5 log(var + eps)) in float64 under the forward-error bound of its C-term fp32 sum, and the round trip."""
    lib, call, ptr, st = _abi()
    C, H, W = shape
    g = torch.Generator().manual_seed(2000 * B + C * H * W)
    x = torch.randn(B, C, H, W, generator=g)
    w, bias, mean = 0.3 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)
    var, eps = 0.5 + torch.rand(C, generator=g), 1e-5
    ldj0 = torch.randn(B, generator=g)
    dv = [t.to(DEV) for t in (w, bias, mean, var)]

    def launch(xin, inverse, ldj_in):
        out, ldj = torch.full_like(xin, fc.SENTINEL), torch.full((B,), fc.SENTINEL, device=DEV)
        call(lib.dpk_bn2d_bijector, ptr(xin), ptr(dv[0]), ptr(dv[1]), ptr(dv[2]), ptr(dv[3]), eps, B, C, H, W, int(inverse),
             ptr(ldj_in), ptr(out), ptr(ldj), st)
        torch.cuda.synchronize()
        return out, ldj

    v = lambda t: t.double().reshape(1, C, 1, 1)   # noqa: E731
    sd = torch.sqrt(v(var) + eps)
    terms = w.double() - 0.5 * torch.log(var.double() + eps)
    total = float(H * W * terms.sum())
    failed = []
    for inverse, ldj_in in itertools.product((False, True), (None, ldj0)):
        got, ldj = launch(x.to(DEV), inverse, None if ldj_in is None else ldj_in.to(DEV))
        if inverse:
            want = (x.double() - v(bias)) * torch.exp(-v(w)) * sd + v(mean)
        else:
            want = (x.double() - v(mean)) / sd * torch.exp(v(w)) + v(bias)
        want_ldj = (0.0 if ldj_in is None else ldj_in.double()) + torch.full((B,), -total if inverse else total, dtype=torch.float64)
        name = 'bn2d %s B=%d %s%s' % ('x'.join(map(str, shape)), B, 'inverse' if inverse else 'density',
                                      '' if ldj_in is None else ' +ldj')
        e = rel_err(got.cpu().numpy(), want.numpy())
        report_measured('K ' + name + ' out', e, BAR)
        # C terms added in turn by one thread, each with the ulps of logf and a subtraction, then scaled by HW
        bound = _sum_bound(C, H * W * float(terms.abs().sum()), ldj_in, want_ldj.numpy(), term_ulps=4)
        el = np.abs(ldj.cpu().double().numpy() - want_ldj.numpy())
        report_measured('K ' + name + ' ldj (abs)', float(el.max()), float(np.min(bound)))
        if not e <= BAR or not bool((el <= bound).all()):
            failed.append((name, e, el.tolist(), np.asarray(bound).tolist()))
    u, l1 = launch(x.to(DEV), False, ldj0.to(DEV))
    back, l2 = launch(u, True, l1)
    rt = float((back.cpu() - x).abs().max()) / float(x.abs().max())
    report_measured('K bn2d %s B=%d round trip / max|x|' % ('x'.join(map(str, shape)), B), rt, BAR)
    assert rt <= BAR and not failed, (rt, failed)


@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('shape', [(1, 2, 2), (3, 4, 6), (5, 6, 10)], ids=lambda s: 'x'.join(map(str, s)))
def test_space_to_depth_and_back(shape, B):
    """dpk_space_to_depth / dpk_depth_to_space with a seeded random permutation table and the split Ca = 1, 2C, 4C: exact
    against index arithmetic, and an exact round trip (element counts 4 .. 1500: only one block, a partial block, several)."""
    lib, call, ptr, st = _abi()
    C, H, W = shape
    rs = np.random.RandomState(C * H * W + B)
    table = rs.permutation(4 * C).astype(np.int32)
    while np.array_equal(table, np.arange(4 * C)):       # (4 entries: one draw in 24 is the identity)
        table = rs.permutation(4 * C).astype(np.int32)
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(int(rs.randint(1 << 30))))
    xn = x.numpy()
    want = np.empty((B, 4 * C, H // 2, W // 2), np.float32)
    for o, e in enumerate(table):
        want[:, o] = xn[:, e >> 2, ((e >> 1) & 1)::2, (e & 1)::2]
    want = torch.from_numpy(want)
    xd, td = x.to(DEV), torch.from_numpy(table).to(DEV)
    for Ca in (1, 2 * C, 4 * C):
        a = torch.full((B, Ca, H // 2, W // 2), fc.SENTINEL, device=DEV)
        b = None if Ca == 4 * C else torch.full((B, 4 * C - Ca, H // 2, W // 2), fc.SENTINEL, device=DEV)
        call(lib.dpk_space_to_depth, ptr(xd), B, C, H, W, ptr(td), ptr(a), Ca, ptr(b), st)
        torch.cuda.synchronize()
        assert torch.equal(a.cpu(), want[:, :Ca]), (shape, B, Ca)
        assert b is None or torch.equal(b.cpu(), want[:, Ca:]), (shape, B, Ca)
        back = torch.full_like(xd, fc.SENTINEL)
        call(lib.dpk_depth_to_space, ptr(a), Ca, ptr(b), B, C, H, W, ptr(td), ptr(back), st)
        torch.cuda.synchronize()
        assert torch.equal(back, xd), (shape, B, Ca)
