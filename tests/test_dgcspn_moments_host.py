"""DgcSpn.posterior_moments without a device: the header bound onto libdeeprob_dgc.so and the library's exports, the argument
errors raised before anything reaches the device, and the restatement the GPU tests compare with
(tests/dgcspn_moments_ref.py) pinned against three things that share no code with it: float64 autograd through the oracle
(ref.exact_marginals), trapezoid quadrature of the oracle's forward, and the oracle's mpe."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import dgcspn_oracle as dorc
from tests import dgcspn_moments_ref as mref
from tests import dgcspn_topdown_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ['dpm_dgcspn_moments', 'dpm_dgcspn_moments_workspace_bytes', 'dpm_last_error']
AGREE = 1e-9                    # (the bar of tests/test_ratspn_moments_host.py)
HOST_CASES = ['dw4', 'odd5', 'mixed6', 'full3']


# ---- the header and the library --------------------------------------------------------------------------------------------
def test_dgcm_header_parses_and_declares_its_entry_points_once():
    from deeprob import hip
    from deeprob.hip import dgcm
    text = open(os.path.join(ROOT, 'include', 'deeprob_dgcm.h')).read()
    sigs, consts, structs = hip.parse_header(text, prefix='dpm', header='deeprob_dgcm.h')
    assert sigs == dgcm.SIGNATURES and not structs
    assert sorted(sigs) == ENTRY_POINTS
    assert consts['DPM_OK'] == 0 and consts['DPM_EINVAL'] == -1 and consts['DPM_EWORKSPACE'] == -2 and consts['DPM_ELAUNCH'] == -3
    assert consts['DPM_EINVAL'] == hip.DGC.constants['DPG_EINVAL'] and consts['DPM_ELAUNCH'] == hip.DGC.constants['DPG_ELAUNCH']
    assert 1 <= consts['DPM_MAX_GROUPS'] <= 4096
    declared = re.findall(r'\b(dpm_\w+)\s*\(', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    assert sorted(declared) == sorted(set(declared)) == sorted(sigs), 'every entry point is declared once'
    assert len(sigs['dpm_dgcspn_moments'][1]) == 21 and len(sigs['dpm_dgcspn_moments_workspace_bytes'][1]) == 3
    assert sigs['dpm_dgcspn_moments_workspace_bytes'][0] is ctypes.c_int64


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], check=True, capture_output=True, text=True).stdout
    return [l.split()[-1] for l in out.splitlines() if l.split()]


def test_the_registry_and_the_exports():
    """BINDINGS is the pinned seven; DGCM is bound onto the library of DGC, which exports exactly the dpm_ names beside
    exactly its three dpg_ names; no other library exports a dpm_ name."""
    from deeprob import hip
    assert [b.prefix for b in hip.BINDINGS] == ['dpk', 'dps', 'dpl', 'dpc', 'dpg', 'dpq', 'dpr']
    assert hip.EXTENSIONS == (hip.DGCM,) and hip.ALL_BINDINGS == hip.BINDINGS + hip.EXTENSIONS
    assert hip.DGCM.onto is hip.DGC and hip.DGCM.lib_path == hip.DGC.lib_path and hip.DGCM.prefix == 'dpm'
    exported = _exports(hip.DGC.lib_path)
    assert sorted(n for n in exported if n.startswith('dpm_')) == ENTRY_POINTS
    assert sorted(n for n in exported if n.startswith('dpg_')) == ['dpg_abi_version', 'dpg_dgcspn_topdown', 'dpg_last_error']
    for path in sorted({b.lib_path for b in hip.BINDINGS} - {hip.DGC.lib_path}):
        assert not [n for n in _exports(path) if n.startswith('dpm_')], path
    lib = hip.DGCM.load()
    assert lib is hip.DGC.load() and hip.DGCM.lib is lib


def test_missing_library_and_header_raise(monkeypatch):
    from deeprob.hip import HipError, dgc, dgcm
    monkeypatch.setattr(dgc, '_lib', None)
    monkeypatch.setattr(dgcm, '_lib', None)
    monkeypatch.setattr(dgc, 'LIB_PATH', os.path.join(ROOT, 'no', 'such', 'libdeeprob_dgc.so'))
    with pytest.raises(HipError) as e:
        dgcm.load_library()
    assert 'make -C deeprob-kit_amd/csrc' in str(e.value)
    monkeypatch.setattr(dgcm, 'HEADER_PATH', os.path.join(ROOT, 'no', 'such', 'deeprob_dgcm.h'))
    with pytest.raises(HipError, match='deeprob_dgcm.h'):
        dgcm._read_header()


def _table(case):
    from deeprob.hip import dgc
    geom = ref.case_geometry(case)
    return geom, (ctypes.c_int32 * (len(geom) * dgc.DPG_GEOM_INTS))(*[int(v) for r in geom for v in r])


def _raw(lib, case='dw4', B=0, geom=True, tables=False, ws_bytes=0, **over):
    """dpm_dgcspn_moments on null data pointers with the sizes of a case, some overridden: what the entry point says before
    it touches a pointer or the device."""
    kw = ref.CASES[case]
    C, H, W = kw['in_features']
    rows, garr = _table(case)
    size = dict(C=C, H=H, W=W, K=kw['n_batch'], L=len(rows), classes=kw.get('out_classes', 1))
    size.update(over)
    L = len(rows)
    act, logw = (ctypes.c_void_p * L)(), (ctypes.c_void_p * (L + 1))()
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    return lib.dpm_dgcspn_moments(B, size['C'], size['H'], size['W'], size['K'], size['L'], cast(garr) if geom else None,
                                  size['classes'], 0, None, None, cast(act) if tables else None, cast(logw) if tables else None,
                                  None, None, None, None, None, None, ws_bytes, None)


def test_bad_arguments_are_reported_by_the_raw_handle():
    from deeprob.hip import dgcm
    lib = dgcm.load_library()
    assert _raw(lib, tables=True) == dgcm.DPM_OK                     # (B = 0: nothing to do, nothing launched)
    assert _raw(lib) == dgcm.DPM_EINVAL and b'null table' in lib.dpm_last_error()
    assert _raw(lib, tables=True, geom=False) == dgcm.DPM_EINVAL and b'null table' in lib.dpm_last_error()
    assert _raw(lib, tables=True, B=-1) == dgcm.DPM_EINVAL and b'bad sizes' in lib.dpm_last_error()
    for over in (dict(C=0), dict(H=0), dict(K=0), dict(classes=0), dict(L=0), dict(L=13), dict(K=5), dict(W=7)):
        assert _raw(lib, tables=True, **over) == dgcm.DPM_EINVAL, over
        assert b'dpm_dgcspn_moments' in lib.dpm_last_error()
    # the library has one error text: dpg_last_error() reads what a dpm_ entry point wrote
    assert lib.dpg_last_error() == lib.dpm_last_error()
    # the workspace: sized by the geometry, too small is its own code, reported before any pointer is read
    for case in ref.CASES:
        rows, garr = _table(case)
        nf = max(r[0] * r[1] * r[2] for r in rows)
        ng = max(r[3] * r[4] * r[5] for r in rows)
        size = lambda b: lib.dpm_dgcspn_moments_workspace_bytes(b, len(rows), ctypes.cast(garr, ctypes.c_void_p))
        assert size(0) == 0 and size(1) == 4 * (nf + ng) and size(301) == 301 * 4 * (nf + ng)
        assert size(10 ** 6) == dgcm.DPM_MAX_GROUPS * 4 * (nf + ng)
        assert dgcm.workspace_bytes(301, rows) == size(301)
        assert _raw(lib, case, B=4, tables=True, ws_bytes=size(4) - 1) == dgcm.DPM_EWORKSPACE
        assert b'workspace' in lib.dpm_last_error()
        assert _raw(lib, case, B=4, tables=True, ws_bytes=size(4)) == dgcm.DPM_EINVAL and b'null pointer' in lib.dpm_last_error()
    rows, garr = _table('dw4')
    assert lib.dpm_dgcspn_moments_workspace_bytes(-1, len(rows), ctypes.cast(garr, ctypes.c_void_p)) == dgcm.DPM_EINVAL
    assert lib.dpm_dgcspn_moments_workspace_bytes(4, len(rows), None) == dgcm.DPM_EINVAL
    # the 28 x 28 example model: below 1 GiB at any batch
    rows = ref.geometry((1, 28, 28), 16, 32, True, 0)
    assert max(r[0] * r[1] * r[2] for r in rows) == 32 * 59 * 59
    assert 0 < dgcm.workspace_bytes(1 << 20, rows) < (1 << 30)


def test_argument_errors_need_no_device():
    """A CPU model or tensor raises HipError (no silent fallback); training-mode dropout is not built and says so."""
    from deeprob.hip import HipError
    from deeprob.spn.models import DgcSpn
    model = ref.make_model('dw4')
    x = torch.randn(3, 1, 4, 4)
    for method in (model.posterior_moments, model.expectation, model.variance):
        with pytest.raises(HipError):
            method(x)
    for kw in (dict(in_dropout=0.2), dict(sum_dropout=0.2)):
        drop = DgcSpn((1, 4, 4), n_batch=2, sum_channels=2, depthwise=True, **kw).train()
        for method in (drop.posterior_moments, drop.expectation, drop.variance):
            with pytest.raises(NotImplementedError, match='dropout'):
                method(x)
        with pytest.raises(HipError):
            drop.eval().expectation(x)
    from deeprob.hip import dgcm, Workspace
    geom = dgcm.product_geometry(model._product_layers())
    with pytest.raises(HipError, match='no CPU'):
        dgcm.dgcspn_moments((1, 4, 4), geom, 1, x, None, [], [], model.base_layer.loc, model.base_layer.scale, Workspace())


# ---- the restatement against the oracle ------------------------------------------------------------------------------------
def _variants(case):
    """(label, y, all_classes, class whose root the oracle is asked for or None for the mixture)"""
    classes = ref.CASES[case].get('out_classes', 1)
    if classes == 1:
        return [('single', None, False, 0)]
    return [('class%d' % c, torch.tensor([c]), False, c) for c in range(classes)] + [('mixture', None, True, None)]


def _restate64(model, case, x, y, all_classes):
    return mref.restate_float64(model, case, x, y, all_classes)


def _scope(case):
    _, h, w = ref.CASES[case]['in_features']
    scope = np.ones((h, w), bool)
    if case == 'odd5':
        scope[-1, :] = scope[:, -1] = False
    return scope


@pytest.mark.parametrize('case', HOST_CASES)
def test_leaf_flow_is_the_gradient_of_the_log_evidence(case):
    """leaf_flow against d log p / d z by float64 autograd through the oracle, for every class and for the mixture of the
    classes (the classes' gradients weighted by softmax(root outputs)); the flows of a pixel in scope sum to 1, those of a
    pixel out of scope are 0."""
    model = ref.make_model(case)
    sd64, plan = ref.state(model, torch.float64), ref.case_plan(case)
    row = ref.half_observed_row(model, case)
    out = dorc.dgcspn_forward(sd64, row.double(), plan)[0]
    post = torch.softmax(out, dim=0).numpy()
    scope = _scope(case)
    for label, y, all_classes, cls in _variants(case):
        flow = _restate64(model, case, row, y, all_classes)[2][0]
        if cls is not None:
            want = ref.exact_marginals(sd64, row, plan, cls=cls)
        else:
            want = sum(post[c] * ref.exact_marginals(sd64, row, plan, cls=c) for c in range(len(post)))
        err = float(np.abs(flow - want).max())
        print('%s %s: max |leaf_flow - autograd| %.3e' % (case, label, err))
        assert flow.shape == want.shape and err <= AGREE, (label, err)
        total = flow.sum(axis=0)
        assert np.abs(total[scope] - 1.0).max() <= AGREE and (total[~scope] == 0.0).all()
    if len(post) > 1:
        # (class 0 alone is another answer than the mixture: the root of the all-classes pass is what was checked)
        f0 = _restate64(model, case, row, None, False)[2]
        fa = _restate64(model, case, row, None, True)[2]
        assert np.abs(f0 - fa).max() > 1e-3


@pytest.mark.parametrize('case', HOST_CASES)
def test_moments_are_the_quadrature_of_the_oracle(case):
    """E[x | e] and Var[x | e] of one NaN entry per case and variant by trapezoid quadrature of t^k p(t, e) on the float64
    oracle over loc +- 12 scale of the entry's components, with a step of a third of the smallest scale (the trapezoid rule
    on a mixture of Gaussians converges geometrically: the error at this step is far below 1e-9)."""
    model = ref.make_model(case)
    sd64, plan = ref.state(model, torch.float64), ref.case_plan(case)
    row = ref.half_observed_row(model, case)
    scope = torch.from_numpy(_scope(case))
    hidden = (torch.isnan(row[0]) & scope[None]).nonzero()
    c, h, w = (int(v) for v in hidden[len(hidden) // 2])
    locs, scales = sd64['base_layer.loc'][:, c, h, w], sd64['base_layer.scale'][:, c, h, w]
    lo, hi = float((locs - 12.0 * scales).min()), float((locs + 12.0 * scales).max())
    n = int(np.ceil((hi - lo) / (float(scales.min()) / 3.0))) + 1
    t = torch.linspace(lo, hi, n, dtype=torch.float64)
    rows = row.double().repeat(n, 1, 1, 1)
    rows[:, c, h, w] = t
    out = dorc.dgcspn_forward(sd64, rows, plan)
    for label, y, all_classes, cls in _variants(case):
        mean, var, _ = _restate64(model, case, row, y, all_classes)
        ll = out[:, cls] if cls is not None else torch.logsumexp(out, dim=1)
        p = torch.exp(ll - ll.max())
        z = torch.trapezoid(p, t)
        e1 = float(torch.trapezoid(p * t, t) / z)
        e2 = float(torch.trapezoid(p * (t - e1) ** 2, t) / z)
        got1, got2 = mean[0, c, h, w], var[0, c, h, w]
        print('%s %s: mean %.3e var %.3e' % (case, label, abs(got1 - e1), abs(got2 - e2)))
        assert abs(got1 - e1) <= AGREE * (1.0 + abs(e1)) and abs(got2 - e2) <= AGREE * (1.0 + e2), (label, got1, e1, got2, e2)


@pytest.mark.parametrize('case', ['dw4', 'odd5', 'full3'])
def test_mean_is_the_mpe_of_the_oracle(case):
    """On a model with one root the reference's mpe is the posterior mean: dorc.dgcspn_mpe in float64, every NaN entry in
    scope; observed entries come back as given with variance 0; the pixels of odd5 that are in nobody's scope are NaN in
    both outputs."""
    model = ref.make_model(case)
    sd64, plan = ref.state(model, torch.float64), ref.case_plan(case)
    row = ref.half_observed_row(model, case)
    mean, var, _ = _restate64(model, case, row, None, False)
    want = dorc.dgcspn_mpe(sd64, row.double(), plan).numpy()
    hid = torch.isnan(row).numpy()
    reached = hid & _scope(case)[None, None]
    assert reached.any() and np.abs(mean - want)[reached].max() <= AGREE
    assert (var[reached] > 0).all()
    assert np.array_equal(mean[~hid], row.double().numpy()[~hid]) and (var[~hid] == 0.0).all()
    outside = hid & ~_scope(case)[None, None]
    assert outside.any() == (case == 'odd5')
    assert np.isnan(mean[outside]).all() and np.isnan(var[outside]).all()


def test_all_nan_row_sums_to_one_per_pixel():
    """Nothing observed: every activation is log 1, the flows of a pixel in scope sum to 1 -- exactly, up to the rounding of
    the float64 sums themselves: 8 ulp of 1 are allowed, 2 are measured -- and the moments are the prior's: finite, with
    positive variance."""
    for case in HOST_CASES:
        model = ref.make_model(case)
        x = torch.full((1,) + tuple(ref.CASES[case]['in_features']), float('nan'))
        for label, y, all_classes, _ in _variants(case):
            mean, var, flow = _restate64(model, case, x, y, all_classes)
            scope = _scope(case)
            total = flow[0].sum(axis=0)
            assert np.abs(total[scope] - 1.0).max() <= 8 * np.finfo(np.float64).eps and (total[~scope] == 0.0).all(), (case, label)
            assert np.isfinite(mean[0][:, scope]).all() and (var[0][:, scope] > 0).all()
            assert np.isnan(mean[0][:, ~scope]).all() and np.isnan(var[0][:, ~scope]).all()


def test_impossible_evidence_in_the_restatement():
    """Activations of -inf: NaN in the NaN entries, the observed entries as given with variance 0, NaN flows."""
    case = 'dw4'
    model = ref.make_model(case)
    sd64, plan = ref.state(model, torch.float64), ref.case_plan(case)
    row = ref.half_observed_row(model, case)
    acts = [torch.full_like(a, float('-inf')) for a in ref.host_activations(sd64, row.double(), plan)]
    mean, var, flow = mref.posterior_moments(ref.case_geometry(case), acts, ref.host_logws(sd64, plan), sd64['base_layer.loc'],
                                             sd64['base_layer.scale'], row)
    hid = torch.isnan(row).numpy()
    assert np.isnan(mean[hid]).all() and np.isnan(var[hid]).all() and np.isnan(flow).all()
    assert np.array_equal(mean[~hid], row.double().numpy()[~hid]) and (var[~hid] == 0.0).all()
