"""Cases, float64 reference and dispatch restatement for the RealNVP-2D evaluation kernels (csrc/flows2d.hip), shared by
tests/test_flows2d_envelope_host.py, tests/test_flows2d_envelope_gpu.py and the child tests/_conv2d_route_cases.py.

No tests here and no device use at import: the functions that launch kernels take the device as an argument.

  conv_ref      the convolution of dpk_conv2d_forward in float64 on the CPU
  make_inputs   seeded inputs of a case (BatchNorm shifts of both signs: see there)
  route         dpk_conv2d_forward's choice of kernel, restated in Python (with the 64 KB guard of the LDS route)
  CASES         the table: every row names the route and the geometry it is meant to hit
  SWITCH_ROWS   the rows the child process evaluates under each environment switch
"""
import collections
import zlib

import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-5
K_LDS_PIX = 1024          # kLdsPix
K_LDS_CC = 4              # kLdsCC
LDS_LIMIT = 64 * 1024     # what a kernel gets without raising hipFuncAttributeMaxDynamicSharedMemorySize


# ---- float64 reference ---------------------------------------------------------------------------------------------------
def conv_ref(x, v, g, bias, bn, mask, res, ks):
    """``conv(mask * relu(bn(x))) + res`` in float64 on the CPU: weights ``g * v / ||v||`` per output channel, `bn` =
    (weight, bias, running_mean, running_var, eps) of an eval-mode BatchNorm2d or None (then no ReLU either), `mask`
    [H, W] or None, "same" zero padding (the padding is applied AFTER the fold: padded operands are zero)."""
    d = lambda t: None if t is None else t.detach().cpu().double()   # noqa: E731
    x, v, g, bias, mask, res = d(x), d(v), d(g), d(bias), d(mask), d(res)
    cout = v.shape[0]
    w = v * (g.reshape(cout) / v.reshape(cout, -1).norm(dim=1)).reshape(cout, 1, 1, 1)
    if bn is not None:
        bw, bb, mean, var = (d(t).reshape(1, -1, 1, 1) for t in bn[:4])
        x = torch.relu((x - mean) / torch.sqrt(var + float(bn[4])) * bw + bb)
    if mask is not None:
        x = x * mask.reshape(1, 1, x.shape[2], x.shape[3])
    y = F.conv2d(x, w, bias, padding=ks // 2)
    return y if res is None else y + res


# ---- dispatch restatement -----------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _on(env, name, char):
    return (env or {}).get(name, '')[:1] == char


def route(B, Cin, Cout, H, W, ks, masked, env=None):
    """The kernel dpk_conv2d_forward launches: dict(route='lds' | 'mfma' | 'valu', ...).  Whenever the LDS route was
    considered (wide unmasked 3x3, at most 1024 pixels, no switch against it) the dict carries G, ntile, TW and lds_bytes,
    also when the 64 KB guard then turned it down (route != 'lds').  `env`: the DPK_CONV_* switches (a mapping)."""
    force_valu, mfma3, no_lds = _on(env, 'DPK_CONV_VALU', '1'), _on(env, 'DPK_CONV_MFMA3', '1'), _on(env, 'DPK_CONV_LDS', '0')
    wide = not masked and Cin >= 8 and Cout >= 16
    geom = {}
    if wide and ks == 3 and not force_valu and not mfma3 and not no_lds and H * W <= K_LDS_PIX:
        plane = (H + 2) * (W + 2)
        G = min(max(1, min(K_LDS_PIX // (H * W), 2048 // plane)), B)
        ntile = _cdiv(G * H * W, 32)
        geom = dict(G=G, ntile=ntile, TW=6 if ntile <= 24 else 7 if ntile <= 28 else 8,
                    lds_bytes=2 * K_LDS_CC * G * plane * 4)
        if geom['lds_bytes'] <= LDS_LIMIT:
            return dict(route='lds', **geom)
    if wide and not force_valu and (ks == 1 or mfma3):
        return dict(route='mfma', **geom)
    return dict(route='valu', **geom)


def instantiation(case, env=None):
    """The template instance a row runs, as written in flows2d.hip."""
    r = route(case.B, case.Cin, case.Cout, case.H, case.W, case.ks, case.mask, env)
    t = lambda b: 'true' if b else 'false'   # noqa: E731
    if r['route'] == 'lds':
        return 'conv3x3_lds_kernel<%s, 4, %d>' % (t(case.fold), r['TW'])
    if r['route'] == 'mfma':
        return 'conv2d_mfma_kernel<%d, %s>' % (case.ks, t(case.fold))
    return 'conv2d_kernel<%d, %s, %s>' % (case.ks, t(case.fold), t(case.mask))


# ---- the table -------------------------------------------------------------------------------------------------------------
# fold: eval-mode BatchNorm2d + ReLU in front; mask: checkerboard on the operand; sliced: input, output and residual are
# channel slices of larger tensors (three different batch strides), the output buffer pre-filled with a sentinel;
# abi: through dpk_conv2d_prepare / dpk_conv2d_forward (fold and mask together); want: what `route` must say.
Case = collections.namedtuple('Case', 'name B Cin Cout H W ks fold mask res bias sliced abi want')


def _c(name, B, Cin, Cout, H, W, ks, fold=False, mask=False, res=False, bias=True, sliced=False, abi=False, **want):
    return Case(name, B, Cin, Cout, H, W, ks, fold, mask, res, bias, sliced, abi, want)


CASES = [
    # -- conv3x3_lds_kernel: the tile-count cuts (TW = 6 up to 24 tiles, 7 up to 28, 8 above) --
    _c('lds_24x32_b1_nt24', 1, 8, 16, 24, 32, 3, fold=True, route='lds', G=1, ntile=24, TW=6),
    _c('lds_16x16_b3_nt24', 3, 12, 17, 16, 16, 3, res=True, route='lds', G=3, ntile=24, TW=6),
    _c('lds_28x28_nt25', 2, 9, 33, 28, 28, 3, fold=True, route='lds', G=1, ntile=25, TW=7),
    _c('lds_28x32_nt28', 1, 10, 16, 28, 32, 3, bias=False, route='lds', G=1, ntile=28, TW=7),
    _c('lds_30x30_nt29', 2, 8, 48, 30, 30, 3, fold=True, res=True, route='lds', G=1, ntile=29, TW=8),
    _c('lds_32x32_nt32', 1, 11, 17, 32, 32, 3, route='lds', G=1, ntile=32, TW=8),
    # G = 4 with a ragged last group of 1; G = 28: samples straddle the 32-pixel tiles, last group of 2
    _c('lds_16x16_b9_g4', 9, 16, 32, 16, 16, 3, fold=True, route='lds', G=4, ntile=32, TW=8),
    _c('lds_6x6_b30_g28', 30, 19, 33, 6, 6, 3, fold=True, res=True, route='lds', G=28, ntile=32, TW=8),
    # Cin mod 4 = 0, 1, 2, 3, 0 on one small image: the last staged chunk holds 4, 1, 2, 3, 4 real channels
    _c('lds_7x9_cin8', 5, 8, 16, 7, 9, 3, fold=True, route='lds', G=5, ntile=10, TW=6),
    _c('lds_7x9_cin9', 5, 9, 16, 7, 9, 3, route='lds', G=5, ntile=10, TW=6),
    _c('lds_7x9_cin9_fold', 5, 9, 17, 7, 9, 3, fold=True, route='lds', G=5, ntile=10, TW=6),
    _c('lds_7x9_cin10', 5, 10, 16, 7, 9, 3, fold=True, route='lds', G=5, ntile=10, TW=6),
    _c('lds_7x9_cin11', 5, 11, 16, 7, 9, 3, route='lds', G=5, ntile=10, TW=6),
    _c('lds_7x9_cin12', 5, 12, 48, 7, 9, 3, fold=True, res=True, route='lds', G=5, ntile=10, TW=6),
    _c('lds_10x6_slices', 7, 10, 20, 10, 6, 3, fold=True, res=True, sliced=True, route='lds', G=7, ntile=14, TW=6),
    _c('lds_64ch', 2, 64, 64, 5, 5, 3, fold=True, res=True, route='lds', G=2, ntile=2, TW=6),
    # -- conv2d_mfma_kernel<1, *>: B*H*W = 20 (partial wave), 189 (partial work-group), 257 (one pixel into a second one) --
    _c('mfma_px20', 5, 9, 17, 2, 2, 1, fold=True, route='mfma'),
    _c('mfma_px189_slices', 3, 8, 33, 7, 9, 1, res=True, sliced=True, route='mfma'),
    _c('mfma_px257', 1, 13, 16, 1, 257, 1, fold=True, res=True, route='mfma'),
    _c('mfma_px189_cin63', 3, 63, 64, 9, 7, 1, fold=True, bias=False, route='mfma'),
    # -- conv2d_kernel: narrow layers, masks, fold + mask, wide 3x3 above 1024 pixels, thin images --
    _c('valu_narrow_cin3', 2, 3, 20, 5, 7, 3, fold=True, route='valu'),
    _c('valu_narrow_cout5_1x1', 2, 12, 5, 5, 7, 1, route='valu'),
    _c('valu_narrow_cin4_1x1_fold', 3, 4, 16, 6, 6, 1, fold=True, res=True, route='valu'),
    _c('valu_mask_cin12_slices', 2, 12, 16, 8, 8, 3, mask=True, res=True, sliced=True, route='valu'),
    _c('valu_mask_1x1', 2, 8, 16, 5, 6, 1, mask=True, route='valu'),
    _c('valu_fold_mask_3x3', 3, 6, 18, 6, 5, 3, fold=True, mask=True, res=True, abi=True, route='valu'),
    _c('valu_fold_mask_1x1', 3, 12, 16, 4, 6, 1, fold=True, mask=True, abi=True, route='valu'),
    _c('valu_34x32_above_1024px', 1, 8, 16, 34, 32, 3, route='valu'),
    _c('valu_33x33_above_1024px', 2, 9, 17, 33, 33, 3, fold=True, res=True, route='valu'),
    _c('valu_w1', 3, 5, 6, 4, 1, 3, fold=True, route='valu'),
    _c('valu_w2', 3, 5, 6, 4, 2, 3, route='valu'),
    _c('valu_w3', 3, 5, 6, 4, 3, 3, fold=True, res=True, route='valu'),
    _c('valu_w5', 3, 5, 6, 4, 5, 3, route='valu'),
    _c('valu_h1', 3, 4, 8, 1, 9, 3, fold=True, route='valu'),
    # -- thin images: the padded plane is above 2048 floats, G = 1 would ask for more than 64 KB of LDS --
    _c('thin_2x512', 2, 8, 16, 2, 512, 3, fold=True, route='valu', G=1, lds_bytes=65792),
    _c('thin_1x700', 2, 8, 16, 1, 700, 3, res=True, route='valu', G=1, lds_bytes=67392),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# rows of the child process under each switch (read once per process by the library), and the route they must take there
_WIDE3 = ['lds_16x16_b3_nt24', 'lds_28x28_nt25', 'lds_32x32_nt32', 'lds_6x6_b30_g28', 'lds_7x9_cin9', 'lds_7x9_cin9_fold',
          'lds_10x6_slices']
SWITCH_ROWS = {
    # conv2d_mfma_kernel<3, *>: fold on and off, odd Cin (9, 11, 19), Cout = 17; the rows above 1024 pixels too
    'DPK_CONV_MFMA3': ('1', 'mfma', _WIDE3 + ['valu_33x33_above_1024px', 'valu_34x32_above_1024px']),
    'DPK_CONV_VALU': ('1', 'valu', _WIDE3 + ['mfma_px20', 'mfma_px189_slices', 'mfma_px257']),
    'DPK_CONV_LDS': ('0', 'valu', _WIDE3),
}


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def make_inputs(case):
    """Seeded fp32 CPU tensors of a row (a pure function of its name): x ~ N(0, 1), weight norms g in [0.5, 1.5] (results of
    order one, so that rel_err is an absolute error on most elements), BatchNorm scale in [0.8, 1.2].

    The BatchNorm shift ``beta - mean * gamma / sqrt(var + eps)`` is positive on the even channels and negative on the odd
    ones, 0.3 .. 0.8 in magnitude (asserted: at least a third of each sign).  A kernel that applies the fold to the zero
    padding is wrong by relu(shift) > 0 at the border of the positive channels; one that skips the ReLU is wrong in the
    interior wherever bn(x) < 0, which the negative shifts make the majority there."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()) % (2 ** 31))
    B, Cin, Cout, H, W, ks = case.B, case.Cin, case.Cout, case.H, case.W, case.ks
    d = dict(x=torch.randn(B, Cin, H, W, generator=g), v=0.3 * torch.randn(Cout, Cin, ks, ks, generator=g),
             g=0.5 + torch.rand(Cout, 1, 1, 1, generator=g), bias=None, bn=None, mask=None, res=None)
    if case.bias:
        d['bias'] = 0.5 * torch.randn(Cout, generator=g)
    if case.fold:
        gamma, var = 0.8 + 0.4 * torch.rand(Cin, generator=g), 0.5 + torch.rand(Cin, generator=g)
        mean = 0.3 * torch.randn(Cin, generator=g)
        shift = (0.3 + 0.5 * torch.rand(Cin, generator=g)) * (1.0 - 2.0 * (torch.arange(Cin) % 2))
        beta = shift + mean * gamma / torch.sqrt(var + BN_EPS)
        d['bn'] = (gamma, beta, mean, var, BN_EPS)
        got = beta.double() - mean.double() * gamma.double() / torch.sqrt(var.double() + BN_EPS)
        third = _cdiv(Cin, 3)
        assert int((got > 0.25).sum()) >= third and int((got < -0.25).sum()) >= third, (case.name, got)
    if case.mask:
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
        d['mask'] = ((yy + xx) % 2).float()
    if case.res:
        d['res'] = torch.randn(B, Cout, H, W, generator=g)
    return d


def reference(case, inp, rows=None):
    sl = slice(None) if rows is None else rows
    res = None if inp['res'] is None else inp['res'][sl]
    return conv_ref(inp['x'][sl], inp['v'], inp['g'], inp['bias'], inp['bn'], inp['mask'], res, case.ks)


# ---- running a row on the device --------------------------------------------------------------------------------------
SENTINEL = -7.0e30
# channels in front of / behind the slice of x, out, res: batch strides (Cin + 5) HW, (Cout + 7) HW, (Cout + 2) HW
PADS = dict(x=(2, 3), out=(3, 4), res=(1, 1))


def _embed(t, pad, dev, fill):
    """`t` [B, C, H, W] as a channel slice of a larger device tensor; (slice, whole)."""
    B, C, H, W = t.shape
    whole = torch.full((B, pad[0] + C + pad[1], H, W), fill, dtype=torch.float32, device=dev)
    part = whole[:, pad[0]:pad[0] + C]
    part.copy_(t)
    return part, whole


def place(case, inp, dev, rows=None):
    """Device tensors of a row: (x, res, out, whole output buffer or None)."""
    sl = slice(None) if rows is None else rows
    x = inp['x'][sl]
    res = None if inp['res'] is None else inp['res'][sl]
    if not case.sliced:
        return x.to(dev), None if res is None else res.to(dev), None, None
    xs, _ = _embed(x, PADS['x'], dev, 3.0e4)
    rs = None if res is None else _embed(res, PADS['res'], dev, -3.0e4)[0]
    blank = torch.empty(x.shape[0], case.Cout, case.H, case.W)
    out, whole = _embed(blank.fill_(SENTINEL), PADS['out'], dev, SENTINEL)
    return xs, rs, out, whole


def modules(case, inp, dev):
    """The package's own WeightNormConv2d (and the BatchNorm2d in front of it) holding the row's parameters."""
    from torch import nn
    from deeprob.torch.utils import WeightNormConv2d
    conv = WeightNormConv2d(case.Cin, case.Cout, case.ks, padding=case.ks // 2, bias=case.bias)
    bn = None
    with torch.no_grad():
        conv.conv.weight_v.copy_(inp['v'])
        conv.conv.weight_g.copy_(inp['g'])
        if case.bias:
            conv.conv.bias.copy_(inp['bias'])
        if case.fold:
            bn = nn.BatchNorm2d(case.Cin, eps=inp['bn'][4])
            for dst, src in zip((bn.weight, bn.bias, bn.running_mean, bn.running_var), inp['bn'][:4]):
                dst.copy_(src)
            bn = bn.eval().to(dev)
    return conv.eval().to(dev), bn


def run(case, inp, dev, rows=None):
    """Evaluates the row (or its samples `rows`, a slice) on `dev`: (result [B, Cout, H, W], whole output buffer or None).
    Through ops_flows2d.conv2d; rows with `abi` through the C ABI itself."""
    from deeprob.hip import ops_flows2d, load_library, call, ptr, stream_ptr
    x, res, out, whole = place(case, inp, dev, rows)
    mask = None if inp['mask'] is None else inp['mask'].to(dev)
    if not case.abi:
        conv, bn = modules(case, inp, dev)
        with torch.no_grad():
            y = ops_flows2d.conv2d(x, conv, bn, in_mask=mask, res=res, out=out)
        assert out is None or y.data_ptr() == out.data_ptr()
    else:
        lib = load_library()
        B, Cin, Cout, ks = x.shape[0], case.Cin, case.Cout, case.ks
        v, g = inp['v'].to(dev), inp['g'].to(dev)
        bias = None if inp['bias'] is None else inp['bias'].to(dev)
        bnp = [None] * 4 if inp['bn'] is None else [t.to(dev) for t in inp['bn'][:4]]
        wpack = torch.empty(lib.dpk_conv2d_pack_floats(Cout, Cin, ks), dtype=torch.float32, device=dev)
        pre = None if inp['bn'] is None else torch.empty(2 * Cin, dtype=torch.float32, device=dev)
        y = out if out is not None else torch.empty(B, Cout, case.H, case.W, dtype=torch.float32, device=dev)
        call(lib.dpk_conv2d_prepare, ptr(v), ptr(g), Cout, Cin, ks, ptr(bnp[0]), ptr(bnp[1]), ptr(bnp[2]), ptr(bnp[3]),
             BN_EPS if inp['bn'] is None else float(inp['bn'][4]), ptr(wpack), ptr(pre), stream_ptr(dev))
        call(lib.dpk_conv2d_forward, ptr(x), x.stride(0), B, Cin, case.H, case.W, ptr(wpack), Cout, ks, ptr(pre), ptr(mask),
             ptr(bias), ptr(res), 0 if res is None else res.stride(0), ptr(y), y.stride(0), stream_ptr(dev))
    torch.cuda.synchronize(dev)
    return y, whole


def outside_untouched(case, whole):
    """Every element of the output buffer outside the slice still holds the sentinel's bits."""
    lo, n = PADS['out'][0], case.Cout
    keep = torch.cat([whole[:, :lo], whole[:, lo + n:]], dim=1).cpu()
    return bool((keep.view(torch.int32) == torch.tensor(SENTINEL).view(torch.int32)).all())


def fp32_cpu_error(case, inp):
    """rel_err of torch's own fp32 CPU convolution on the same inputs against the float64 reference: the yardstick of a row
    whose error exceeds the parity bar by rounding alone (the bound is then four times this)."""
    from tests.util import rel_err
    f = lambda t: None if t is None else t.float()   # noqa: E731
    x, v, g = inp['x'], inp['v'], inp['g']
    w = v * (g.reshape(-1) / v.reshape(v.shape[0], -1).norm(dim=1)).reshape(-1, 1, 1, 1)
    if inp['bn'] is not None:
        bw, bb, mean, var = (t.reshape(1, -1, 1, 1) for t in inp['bn'][:4])
        x = torch.relu((x - mean) / torch.sqrt(var + inp['bn'][4]) * bw + bb)
    if inp['mask'] is not None:
        x = x * inp['mask']
    y = F.conv2d(x, w, f(inp['bias']), padding=case.ks // 2)
    if inp['res'] is not None:
        y = y + inp['res']
    return rel_err(y.numpy(), reference(case, inp).numpy())


def check_row(case, inp, got, name=None, rows=None):
    """(error, bound, note) of a device result against the float64 reference: the parity bar 1e-5; a row above it is held
    to four times the error of torch's fp32 CPU convolution on the same inputs instead, and says so."""
    from tests.util import rel_err
    err = rel_err(got.detach().cpu().numpy(), reference(case, inp, rows).numpy())
    bound, note = 1e-5, ''
    if not err <= bound:
        bound, note = 4.0 * fp32_cpu_error(case, inp), 'above 1e-5: bound = 4 x the error of fp32 CPU F.conv2d'
    return err, bound, note
