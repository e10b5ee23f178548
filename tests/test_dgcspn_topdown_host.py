"""DgcSpn.sample / sample_conditional without a device: the header and the exports of the fourth library, the argument
errors raised before anything reaches the device, and the restatement the GPU tests replay against
(tests/dgcspn_topdown_ref.py) against the exact posterior marginals, d log p / d z of the oracle's forward in float64."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import dgcspn_oracle as dorc
from tests import dgcspn_topdown_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the header and the library --------------------------------------------------------------------------------------------
def test_dgc_header_parses_and_declares_its_entry_points_once():
    from deeprob import hip
    from deeprob.hip import dgc
    text = open(os.path.join(ROOT, 'include', 'deeprob_dgc.h')).read()
    sigs, consts, structs = hip.parse_header(text, prefix='dpg', header='deeprob_dgc.h')
    assert sigs == dgc.SIGNATURES and not structs
    assert sorted(sigs) == ['dpg_abi_version', 'dpg_dgcspn_topdown', 'dpg_last_error']
    assert consts['DPG_OK'] == 0 and consts['DPG_MODE_PRIOR'] == 1 and consts['DPG_MODE_POSTERIOR'] == 2
    assert consts['DPG_GEOM_INTS'] == 13 == len(ref.case_geometry('dw4')[0])
    declared = re.findall(r'\b(dpg_\w+)\s*\(', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    assert sorted(declared) == sorted(set(declared)) == sorted(sigs), 'every entry point is declared once'
    assert len(sigs['dpg_dgcspn_topdown'][1]) == 19


def test_missing_dgc_library_names_the_make_command(monkeypatch):
    from deeprob.hip import HipError, dgc
    monkeypatch.setattr(dgc, '_lib', None)
    monkeypatch.setattr(dgc, 'LIB_PATH', os.path.join(ROOT, 'no', 'such', 'libdeeprob_dgc.so'))
    with pytest.raises(HipError) as e:
        dgc.load_library()
    assert 'make -C deeprob-kit_amd/csrc' in str(e.value)


def test_geometry_of_the_binding_is_the_oracle_schedule():
    from deeprob.hip import dgc
    for case in ref.CASES:
        model = ref.make_model(case)
        geom = dgc.product_geometry(model._product_layers())
        assert geom == ref.case_geometry(case), case
    # 28 x 28, the example model: 6 levels, the counter layout is one slot a sum position and two a leaf entry
    geom = ref.geometry((1, 28, 28), 16, 32, True, 0)
    base, slots = ref.slot_layout(geom, 1, 28, 28)
    assert len(geom) == 6 and base[:2] == [0, 1] and slots == base[-1] + 2 * 784
    assert base[-1] == 1 + sum(r[4] * r[5] for r in geom[:-1]) == 8358 and slots == 9926


# ---- methods and errors ------------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_device():
    """A CPU model raises HipError (no silent fallback, and no longer the reference's NotImplementedError); training-mode
    dropout is not built and says so."""
    from deeprob.hip import HipError
    from deeprob.spn.models import DgcSpn
    model = ref.make_model('dw4')
    assert callable(DgcSpn.sample_conditional)
    with pytest.raises(HipError) as info:
        model.sample(3)
    assert not isinstance(info.value, NotImplementedError)
    with pytest.raises(HipError):
        model.sample(3, seed=1)
    with pytest.raises(HipError):
        model.sample_conditional(torch.randn(3, 1, 4, 4))
    for kw in (dict(in_dropout=0.2), dict(sum_dropout=0.2)):
        drop = DgcSpn((1, 4, 4), n_batch=2, sum_channels=2, depthwise=True, **kw).train()
        with pytest.raises(NotImplementedError, match='dropout'):
            drop.sample(3)
        with pytest.raises(NotImplementedError, match='dropout'):
            drop.sample_conditional(torch.randn(3, 1, 4, 4))
        with pytest.raises(HipError):
            drop.eval().sample_conditional(torch.randn(3, 1, 4, 4))


# ---- the restatement against the exact posterior -----------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['dw4', 'odd5'])
def test_restatement_draws_the_exact_posterior(case):
    """2^16 rows with distinct counters through the restatement, on the oracle's float64 activations of one half-observed
    image: the frequency of every (component, pixel) within 5 standard errors of d log p / d z in float64, over the cells
    with an expected count of at least 50 (the seed is fixed, so the outcome is deterministic).  On the 5 x 5 model under a
    pooling level the last row and column are in nobody's scope: component -1, value unchanged."""
    kw = ref.CASES[case]
    C, H, W = kw['in_features']
    model = ref.make_model(case)
    plan, geom = ref.case_plan(case), ref.case_geometry(case)
    sd64 = ref.state(model, torch.float64)
    row = ref.half_observed_row(model, case)
    marg = ref.exact_marginals(sd64, row, plan)                              # [K, H, W]
    total = marg.sum(axis=0)
    in_scope = np.ones((H, W), bool)
    if case == 'odd5':
        in_scope[-1, :] = in_scope[:, -1] = False
    assert (marg >= -1e-12).all() and np.allclose(total[in_scope], 1.0, atol=1e-9) and (total[~in_scope] == 0.0).all()
    acts = ref.host_activations(sd64, row.double(), plan)
    n = ref.STAT_ROWS
    samples, root, comp, _ = ref.topdown_sample(geom, (C, H, W), acts, ref.host_logws(sd64, plan), sd64['base_layer.loc'],
                                                sd64['base_layer.scale'], row.expand(n, -1, -1, -1), None, ref.STAT_SEED)
    obs = ~torch.isnan(row[0])
    assert torch.equal(samples[:, obs], row[0][obs].expand(n, -1))
    scope = torch.from_numpy(in_scope)
    assert not torch.isnan(samples[:, :, scope]).any()
    assert (comp.view(n, H, W)[:, scope] >= 0).all() and (comp.view(n, H, W)[:, ~scope] == -1).all()
    hidden_out = torch.isnan(row[0]) & ~scope[None]
    assert torch.isnan(samples[:, hidden_out]).all()
    freq = ref.component_frequencies(comp, kw['n_batch'])
    ref.check_frequencies(freq, marg, n, case)
    # the drawn pixels' means against the posterior mean, which is what the reference's mpe returns
    mean = dorc.dgcspn_mpe(sd64, row.double(), plan)[0].numpy()
    hid = (torch.isnan(row[0]) & scope[None]).numpy()
    got = samples.double().mean(dim=0).numpy()
    spread = samples.double().std(dim=0).numpy()
    assert hid.any() and (np.abs(got - mean)[hid] <= 5.0 * spread[hid] / np.sqrt(n)).all()
    # the weights alone are another distribution: the same draws without the evidence miss the bar
    prior = ref.topdown_sample(geom, (C, H, W), None, ref.host_logws(sd64, plan), sd64['base_layer.loc'],
                               sd64['base_layer.scale'], None, None, ref.STAT_SEED, n_rows=n)[2]
    fp = ref.component_frequencies(prior, kw['n_batch'])
    se = np.sqrt(np.maximum(marg.reshape(fp.shape) * (1 - marg.reshape(fp.shape)), 1e-12) / n)
    assert (np.abs(fp - marg.reshape(fp.shape)) > 5.0 * se).any()


def test_all_nan_evidence_normalises_and_every_case_is_decomposable():
    """The all-NaN image has log-likelihood 0 and marginals that sum to 1 per pixel in scope, for every case; and the
    restatement (which asserts that no position is reached twice) runs every case's geometry without evidence."""
    for case, kw in ref.CASES.items():
        model = ref.make_model(case)
        plan, geom = ref.case_plan(case), ref.case_geometry(case)
        sd64 = ref.state(model, torch.float64)
        x = torch.full((1,) + tuple(kw['in_features']), float('nan'))
        assert abs(float(dorc.dgcspn_forward(sd64, x.double(), plan)[0, 0])) <= 1e-9
        total = ref.exact_marginals(sd64, x, plan).sum(axis=0)
        assert np.allclose(total[total > 0], 1.0, atol=1e-9) and ((total > 0).all() or case == 'odd5')
        out, root, comp, margin = ref.topdown_sample(geom, kw['in_features'], None, ref.host_logws(sd64, plan),
                                                     sd64['base_layer.loc'], sd64['base_layer.scale'], None, None, 5, n_rows=64)
        assert ((comp >= 0).numpy().reshape(64, -1) == (total > 0).reshape(1, -1)).all()
        assert torch.isnan(out).any() == (case == 'odd5') and (margin >= 0).all()
