"""The case table of tests/flows2d_cases.py against the dispatch of dpk_conv2d_forward restated in Python, and the
float64 reference against torch: what tests/test_flows2d_envelope_gpu.py relies on, checked without a device."""
import re

import pytest
import torch
import torch.nn.functional as F

from tests import flows2d_cases as fc

IDS = [c.name for c in fc.CASES]


def _route(c, env=None):
    return fc.route(c.B, c.Cin, c.Cout, c.H, c.W, c.ks, c.mask, env)


@pytest.mark.parametrize('case', fc.CASES, ids=IDS)
def test_row_lands_where_it_claims(case):
    got = _route(case)
    assert case.want and 'route' in case.want
    for key, want in case.want.items():
        assert got.get(key) == want, (case.name, key, got)
    if case.want['route'] == 'lds':
        assert set(case.want) == {'route', 'G', 'ntile', 'TW'} and got['lds_bytes'] <= fc.LDS_LIMIT
    assert case.B <= 30 and max(case.Cin, case.Cout) <= 64
    assert not case.abi or (case.fold and case.mask)
    assert case.name.split('_')[0] in ('lds', 'mfma', 'valu', 'thin')
    if case.sliced:   # three different batch strides
        strides = {case.Cin + sum(fc.PADS['x']), case.Cout + sum(fc.PADS['out'])}
        if case.res:
            strides.add(case.Cout + sum(fc.PADS['res']))
        assert len(strides) == 2 + case.res


def test_rows_cover_every_instantiation():
    inst = {fc.instantiation(c) for c in fc.CASES}
    b = ('true', 'false')
    for pre in b:
        for tw in (6, 7, 8):
            assert 'conv3x3_lds_kernel<%s, 4, %d>' % (pre, tw) in inst
        assert 'conv2d_mfma_kernel<1, %s>' % pre in inst
        for ks in (1, 3):
            for mask in b:
                assert 'conv2d_kernel<%d, %s, %s>' % (ks, pre, mask) in inst
    assert len(inst) == 6 + 2 + 8


def test_instantiation_names_are_the_ones_dispatched():
    """The names `instantiation` forms occur in the entry point's dispatch (DPK_LDS_CASE / DPK_CONV_CASE / the MFMA branch)."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'deeprob-kit_amd', 'csrc',
                            'flows2d.hip')).read()
    body = src[src.index('int dpk_conv2d_forward('):src.index('int dpk_coupling2d_transform(')]
    for pre in ('true', 'false'):
        for tw in (6, 7, 8):
            assert 'DPK_LDS_CASE(%s, 4, %d)' % (pre, tw) in body
        for ks in (1, 3):
            assert 'conv2d_mfma_kernel<%d, %s>' % (ks, pre) in body
            for mask in ('true', 'false'):
                assert 'DPK_CONV_CASE(%d, %s, %s)' % (ks, pre, mask) in body
    # the constants restated in flows2d_cases.py, and the guard
    assert re.search(r'kLdsCC = %d;' % fc.K_LDS_CC, src) and re.search(r'kLdsPix = %d;' % fc.K_LDS_PIX, src)
    assert 'lds_bytes <= 64 * 1024' in body and 'ntile <= 24' in body and 'ntile <= 28' in body


def test_rows_cover_the_lds_geometry():
    lds = [c for c in fc.CASES if c.want['route'] == 'lds']
    assert {24, 25, 28, 29, 32} <= {c.want['ntile'] for c in lds}
    assert {0, 1, 2, 3} == {c.Cin % 4 for c in lds} and {8, 9, 10, 11, 12} <= {c.Cin for c in lds if (c.H, c.W) == (7, 9)}
    assert {16, 17, 33, 48} <= {c.Cout for c in lds}
    for flag in ('fold', 'res'):
        assert {True, False} == {getattr(c, flag) for c in lds}
    assert any(c.sliced and c.res for c in lds)
    ragged = {c.name: (c.want['G'], c.B % c.want['G']) for c in lds}
    assert ragged['lds_16x16_b9_g4'] == (4, 1) and ragged['lds_6x6_b30_g28'] == (28, 2)
    assert (6 * 6) % 32 != 0
    mf = [c for c in fc.CASES if c.want['route'] == 'mfma']
    assert {20, 189, 257} <= {c.B * c.H * c.W for c in mf} and any(c.Cin % 2 for c in mf)
    assert {17, 33} <= {c.Cout for c in mf} and {True, False} == {c.fold for c in mf}
    assert any(c.sliced and c.res and c.bias for c in mf)
    va = [c for c in fc.CASES if c.want['route'] == 'valu']
    assert {1, 2, 3, 5} <= {c.W for c in va} and any(c.H == 1 for c in va)
    wide = [c for c in va if c.ks == 3 and not c.mask and c.Cin >= 8 and c.Cout >= 16 and c.H * c.W > fc.K_LDS_PIX]
    assert {(34, 32), (33, 33)} <= {(c.H, c.W) for c in wide}
    assert any(c.mask and c.Cin == 12 for c in va) and {1, 3} == {c.ks for c in va if c.fold and c.mask}
    assert len({c.sliced and c.want['route'] for c in fc.CASES} - {False}) == 3      # a sliced row per route


def test_thin_rows_stay_off_the_lds_route():
    for name, shape in (('thin_2x512', (2, 512)), ('thin_1x700', (1, 700))):
        c = fc.BY_NAME[name]
        got = _route(c)
        assert (c.H, c.W) == shape and (c.Cin, c.Cout, c.B, c.ks, c.mask) == (8, 16, 2, 3, False)
        assert c.H * c.W <= fc.K_LDS_PIX and got['lds_bytes'] > 65536 and got['route'] == 'valu'
    # the smallest thin widths: 1x681 and 2x511 are the first above 64 KB
    assert fc.route(1, 8, 16, 1, 680, 3, False)['route'] == 'lds' and fc.route(1, 8, 16, 1, 681, 3, False)['route'] == 'valu'
    assert fc.route(1, 8, 16, 1, 681, 3, False)['lds_bytes'] == 65568
    assert fc.route(1, 8, 16, 2, 510, 3, False)['route'] == 'lds' and fc.route(1, 8, 16, 2, 511, 3, False)['route'] == 'valu'


def test_switch_rows_take_the_switched_route():
    for var, (value, want, names) in fc.SWITCH_ROWS.items():
        insts = set()
        for name in names:
            c = fc.BY_NAME[name]
            assert _route(c, {var: value})['route'] == want, (var, name)
            assert _route(c)['route'] != want or c.H * c.W > fc.K_LDS_PIX, (var, name)
            insts.add(fc.instantiation(c, {var: value}))
        rows = [fc.BY_NAME[n] for n in names]
        if var == 'DPK_CONV_MFMA3':
            assert insts == {'conv2d_mfma_kernel<3, true>', 'conv2d_mfma_kernel<3, false>'}
            assert any(c.Cin % 2 for c in rows) and any(c.Cout == 17 for c in rows)
        elif var == 'DPK_CONV_VALU':
            assert {c.ks for c in rows} == {1, 3}
        wide3 = [c for c in rows if c.ks == 3 and c.H * c.W <= fc.K_LDS_PIX]
        assert {True, False} == {c.fold for c in wide3}
        assert all(c.Cin >= 8 and c.Cout >= 16 and not c.mask for c in rows)
    # an unset or differently set switch changes nothing
    c = fc.BY_NAME['lds_28x28_nt25']
    assert _route(c, {'DPK_CONV_LDS': '1', 'DPK_CONV_VALU': '0', 'DPK_CONV_MFMA3': ''})['route'] == 'lds'


def test_inputs_are_seeded_and_shift_both_ways():
    for c in fc.CASES:
        a, b = fc.make_inputs(c), fc.make_inputs(c)
        assert torch.equal(a['x'], b['x']) and torch.equal(a['v'], b['v'])
        assert (a['bn'] is not None) == c.fold and (a['mask'] is not None) == c.mask and (a['res'] is not None) == c.res
        assert (a['bias'] is not None) == c.bias
        if c.fold:
            gamma, beta, mean, var, eps = a['bn']
            shift = beta.double() - mean.double() * gamma.double() / torch.sqrt(var.double() + eps)
            assert 3 * int((shift > 0).sum()) >= c.Cin and 3 * int((shift < 0).sum()) >= c.Cin
            # the ReLU matters in the interior, the padding at the border
            pre = torch.relu((a['x'].double() - mean.reshape(1, -1, 1, 1)) / torch.sqrt(var.reshape(1, -1, 1, 1) + eps)
                             * gamma.reshape(1, -1, 1, 1) + beta.reshape(1, -1, 1, 1))
            assert 0.2 < float((pre == 0).double().mean()) < 0.8


@pytest.mark.parametrize('ks,fold,mask,res', [(3, True, False, True), (1, True, False, False), (3, False, False, False),
                                              (3, False, True, True)])
def test_conv_ref_equals_the_module_chain_in_float64(ks, fold, mask, res):
    """conv_ref against F.conv2d on a WeightNormConv2d + BatchNorm2d.eval() + ReLU chain built from the package's own
    modules (their parameters, torch's own weight normalisation), all in float64 on the CPU: 1e-12."""
    from torch import nn
    from deeprob.torch.utils import WeightNormConv2d
    case = fc._c('chain', 3, 7, 10, 6, 5, ks, fold=fold, mask=mask, res=res, route='valu')
    inp = fc.make_inputs(case)
    conv = WeightNormConv2d(7, 10, ks, padding=ks // 2, bias=True).double()
    bn = nn.BatchNorm2d(7, eps=fc.BN_EPS).double().eval()
    with torch.no_grad():
        conv.conv.weight_v.copy_(inp['v'])
        conv.conv.weight_g.copy_(inp['g'])
        conv.conv.bias.copy_(inp['bias'])
        h = inp['x'].double()
        if fold:
            for dst, src in zip((bn.weight, bn.bias, bn.running_mean, bn.running_var), inp['bn'][:4]):
                dst.copy_(src)
            h = torch.relu(bn(h))
        if mask:
            h = h * inp['mask'].double()
        w = torch._weight_norm(conv.conv.weight_v, conv.conv.weight_g, 0)
        want = F.conv2d(h, w, conv.conv.bias, padding=ks // 2)
        if res:
            want = want + inp['res'].double()
    got = fc.reference(case, inp)
    assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-12
