"""The buffer contract of the C ABI (include/deeprob_hip.h, Conventions) on poisoned, guard-banded device memory.

(a) Replay: existing small parity cases are called inside ``contract(pattern)`` (tests/buffer_contract.py) for both
    patterns.  Their own oracle assertions run unchanged; on top come the guard check of every allocation made by the
    operators and the record of the entry points called.  The union of that record over the table must be every writer
    entry point of the header except the few in NOT_COVERED.
(b) Bitwise independence: one direct scenario per kernel family and route, run twice plainly and once under each
    pattern, each run on a newly constructed module (the first call builds its tables inside poisoned memory, the second
    takes the cached-table path).  Where the two plain runs agree bit for bit, the poisoned runs must agree with them bit
    for bit; every run is also held to the scenario's oracle at the tolerance of the existing tests.

Nothing here plants a defect or reads out of bounds; the planted defects live in test_buffer_contract_host.py."""
import contextlib
import importlib
import inspect
import itertools
import os
import time
import zlib

import numpy as np
import pytest
import torch

from tests import buffer_contract as bc
from tests.buffer_contract import contract
from tests.conftest import load_golden
from tests.util import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN_IDS = ['ff', '7f']

from tests.dgc_cases import SMALL as _SMALL_DGC
SMALL_DGC = set(_SMALL_DGC)      # the fixtures that ship their state: the small models
I2, I8, PAD = 'ratspn_g784_d2_r8_i2_s2', 'ratspn_g784_d2_r8_i8_s8', 'ratspn_g15_d2_r3_i3_s5_pad'

# (module, test function, selector).  The selector picks parametrisations of the EXISTING test: a key that is one of its
# parametrize arguments (or a parametrised fixture of its module) must equal the value, or be in the set; '#' picks by
# position among what is left.  Every entry must select at least one case (no invented parameters).
REPLAY = [
    # ---- RAT-SPN ------------------------------------------------------------------------------------------------
    ('test_ratspn_gpu', 'test_forward_vs_oracle_ragged_batches', dict(name=I2, B={1, 63, 129}, mapping={'small', 'ring', 'slice'})),
    ('test_ratspn_gpu', 'test_forward_vs_oracle_ragged_batches', dict(name=I8, B={1, 129}, mapping='small')),
    ('test_ratspn_gpu', 'test_forward_vs_oracle_ragged_batches', dict(name=PAD, B={1, 63}, mapping='small')),
    ('test_ratspn_gpu', 'test_layers_golden', {}),
    ('test_ratspn_gpu', 'test_backward_golden', {}),
    ('test_ratspn_gpu', 'test_folded_route_for_wide_models', {'#': {0, 1}}),
    ('test_ratspn_gpu', 'test_bernoulli_known_answer', {}),
    ('test_ratspn_gpu', 'test_bernoulli_input_gradient', {}),
    ('test_ratspn_gpu', 'test_gradients_with_marginalised_inputs', {}),
    ('test_ratspn_gpu', 'test_mpe_golden', {'#': {0, 1}}),
    ('test_ratspn_gpu', 'test_mpe_bernoulli_golden', {}),
    ('test_ratspn_gpu', 'test_sample_replays_against_the_oracle', dict(case={'gauss_d2_pad', 'bernoulli_d3'})),
    ('test_ratspn_gpu', 'test_training_forward_golden_gradients', {}),
    ('test_ratspn_gpu', 'test_training_forward_single_launch_matches_layer_chain', dict(B={1, 37}, evidence='marginalised')),
    ('test_ratspn_gpu', 'test_folded_level_autograd_matches_layer_chain', {'#': {0, 2, 3, 5, 11}}),
    ('test_ratspn_gpu', 'test_unit_scale_fused_shapes_vs_oracle', {'#': {0, 4}}),
    ('test_ratspn_gaussian_gpu', 'test_leaf_forward_vs_float64', dict(name={'pad2', 'wide16_d1'}, B={1, 33}, kind='nan')),
    ('test_ratspn_gaussian_gpu', 'test_leaf_backward_vs_float64', dict(name={'ad4', 'odd3'}, B=300, kind='nan', sign='mixed',
                                                                       x_grad=True)),
    ('test_dropout_gpu', 'test_ratspn_dropout_replayed_by_the_oracle', {}),
    ('test_dropout_gpu', 'test_dgcspn_dropout_replayed_by_the_oracle', {}),
    # ---- DGC-SPN ------------------------------------------------------------------------------------------------
    ('test_dgcspn_gpu', 'test_layers_golden', {}),
    ('test_dgcspn_gpu', 'test_forward_golden', dict(name=SMALL_DGC)),
    ('test_dgcspn_gpu', 'test_gradients_golden', dict(name=SMALL_DGC)),
    ('test_dgcspn_gpu', 'test_mpe_golden', dict(name=SMALL_DGC)),
    ('test_dgcspn_gpu', 'test_streaming_levels_against_oracle', {'#': {0, 1, 3}}),
    ('test_dgcspn_gpu', 'test_random_shapes_against_oracle', {}),
    ('test_dgcspn_gpu', 'test_wide_fused_level_against_oracle', {'#': {2, 5}}),
    ('test_dgcspn_gpu', 'test_fused_leaf_and_first_level_against_oracle', {'#': {0}}),
    ('test_dgcspn_gpu', 'test_fused_level_autograd_matches_layer_chain', {'#': {0, 1}}),
    ('test_dgcspn_gpu', 'test_sum_backward_extreme_weights_against_oracle', dict(cin=6)),
    ('test_dgcspn_backward_gpu', 'test_generic_sum_backward_blocks_and_dispatch', dict(cin={16, 12}, cout={32, 17})),
    ('test_dgcspn_backward_gpu', 'test_fused_level_autograd_against_fp64', {'#': {0}}),
    # ---- RealNVP-1D ---------------------------------------------------------------------------------------------
    ('test_flows_gpu', 'test_log_prob_golden', {}),
    ('test_flows_gpu', 'test_layers_and_inverse_golden', {}),
    ('test_flows_gpu', 'test_custom_masks_vs_oracle', {}),
    ('test_flows_gpu', 'test_ragged_batches_vs_oracle', dict(B={1, 63, 65})),
    ('test_flows_gpu', 'test_training_route_golden', {}),
    ('test_flows_gpu', 'test_sampling_direction_gradients_vs_oracle', {}),
    ('test_flows_gpu', 'test_sampling_entry_points', {}),
    ('test_flows_gpu', 'test_sample_replays_against_the_oracle', {'#': {0}}),
    ('test_flows_gpu', 'test_column_pair_kernels_shapes_vs_oracle', {'#': {0, 6}}),
    ('test_routines_gpu', 'test_train_flow_with_batch_norm', {}),
    ('test_flows_gpu', 'test_coupling_backward_multi_tile_vs_oracle', dict(case='A')),
    # ---- MAF ----------------------------------------------------------------------------------------------------
    ('test_maf_gpu', 'test_golden_eval', dict(name={'maf20_depth2', 'maf33_tanh', 'maf2_energy', 'maf192_bn', 'maf12_units200'})),
    ('test_maf_gpu', 'test_fused_density_vs_float64', {}),
    ('test_maf_gpu', 'test_deep_sampling_kernel_one_launch', {'#': {0, 1}}),
    ('test_maf_gpu', 'test_sampling_kernel_vs_float64_step_loop', dict(B={1, 63})),
    ('test_maf_gpu', 'test_training_goldens', {}),
    ('test_maf_gpu', 'test_masked_linear_forward_backward', {}),
    ('test_maf_gpu', 'test_fused_density_folded_batch_norm_and_accumulate', {}),
    ('test_maf_gpu', 'test_rsample_gradient_golden', {}),
    ('test_gemm_f32_gpu', 'test_integer_data_is_exact', dict(shape=(257, 129, 65))),
    # ---- flat (node-graph) SPN ------------------------------------------------------------------------------------
    ('test_flat_spn_gpu', 'test_golden', {}),
    ('test_flat_spn_gpu', 'test_random_circuits_against_oracle', dict(B={1, 63, 65, 1000})),
    ('test_flat_spn_queries_gpu', 'test_mpe_golden', {}),
    ('test_flat_spn_queries_gpu', 'test_mpe_random_circuits', dict(B={1, 63, 65, 1000})),
    ('test_flat_spn_queries_gpu', 'test_mpe_tensor_inplace_and_extra_columns', {}),
    ('test_flat_spn_queries_gpu', 'test_eval_backward_golden', {}),
    ('test_flat_spn_queries_gpu', 'test_eval_backward_random_circuits', dict(B={1, 63})),
    ('test_flat_spn_queries_gpu', 'test_em_one_iteration', {}),
    ('test_flat_spn_queries_gpu', 'test_sample_replay', dict(case={'mixed4', 'random7'})),
    # ---- RealNVP-2D ---------------------------------------------------------------------------------------------
    ('test_flows2d_gpu', 'test_against_oracle', {}),
    ('test_flows2d_gpu', 'test_log_prob_and_latents_golden', {'#': {0, 3}}),
    ('test_flows2d_gpu', 'test_squeeze_and_unsqueeze', {}),
    ('test_flows2d_gpu', 'test_sampling_runs_on_the_device', {}),
    ('test_flows2d_gpu', 'test_conv_channel_slices_and_errors', {}),
    ('test_flows2d_train_gpu', 'test_gradients_against_oracle_strict', {}),
    ('test_flows2d_train_gpu', 'test_training_step_golden', {'#': {0}}),
    ('test_flows2d_train_gpu', 'test_convolution_node_against_fp64', {}),
    ('test_flows2d_train_gpu', 'test_statistics_and_affine_nodes_against_fp64', {'#': {0, 2}}),
    # ---- optimiser, losses ----------------------------------------------------------------------------------------
    ('test_routines_gpu', 'test_fused_adam_follows_torch_adam', {}),
    ('test_routines_gpu', 'test_neg_mean_loss_op', dict(shape={(1, 1), (4097, 1)})),
    ('test_parallel_gpu', 'test_sharded_mean_ll_on_device_one_process', {}),
    # ---- entry points no operator reaches in one process: direct cases of this module against float64 -------------
    (None, 'direct_bn1d_sharded_entry_points_single_rank', {}),
    (None, 'direct_dgcspn_last_product_into_root', {}),
    (None, 'direct_spatial_gaussian_backward', {}),
]

# Writer entry points no replayed case reaches, each with its reason.  At most 10; no forward / backward / sample / MPE /
# EM entry point of a model family may stand here.
NOT_COVERED = {
    'dpk_profile_next_kernel': 'measurement hook: records two caller-made events around the next launch, writes no tensor',
    'dpk_profile_next_kernel_of': 'measurement hook, as dpk_profile_next_kernel',
}
MAX_NOT_COVERED = 10

def direct_bn1d_sharded_entry_points_single_rank():
    """The four entry points of the batch-sharded BatchNormLayer1d, which the operators reach only with more than one rank,
    called as ONE rank would call them (world = 1: the gathered table is the rank's own moments, the reduced sums its own
    sums) against a float64 statement of training-mode batch norm and its autograd.  Bars: 1e-5 relative on the forward
    quantities, 1e-4 of the tensor's largest magnitude on gradients -- the bars of the flow tests."""
    from deeprob import hip
    from tests.util import grad_err
    lib = hip.load_library()
    dev = torch.device('cuda', torch.cuda.current_device())
    st = hip.stream_ptr(dev)
    momentum, eps = 0.9, 1e-5
    for B, D in ((2, 1), (63, 33), (129, 70), (300, 1025)):
        g = torch.Generator().manual_seed(B * D)
        x = torch.randn(B, D, generator=g) * 1.5 + 0.3
        w, b = 0.3 * torch.randn(D, generator=g), torch.randn(D, generator=g)
        rv, rm = 0.5 + torch.rand(D, generator=g), torch.randn(D, generator=g)
        gu, gi = torch.randn(B, D, generator=g), torch.randn(B, generator=g)
        x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
        var, mean = torch.var_mean(x64, dim=0)
        xhat = (x64 - mean) / torch.sqrt(var + eps)
        u = xhat * torch.exp(w64) + b64
        ildj = (w64 - 0.5 * torch.log(var + eps)).sum()
        ((gu.double() * u).sum() + gi.double().sum() * ildj).backward()
        xc, wc, bias_c, rvc, rmc, guc, gic = (t.to(dev) for t in (x, w, b, rv, rm, gu, gi))

        mom = torch.empty(2 * D + 1, dtype=torch.float32, device=dev)
        hip.call(lib.dpk_bn1d_local_moments, hip.ptr(xc), B, D, hip.ptr(mom), st)
        assert float(mom[0]) == B
        assert rel_err(mom[1:1 + D].cpu().numpy(), mean.detach().numpy()) <= 1e-5
        assert rel_err(mom[1 + D:].cpu().numpy(), ((x64 - mean) ** 2).sum(0).detach().numpy()) <= 1e-5

        out = torch.empty_like(xc)
        ldj = torch.empty(1, dtype=torch.float32, device=dev)
        smean = torch.empty(D, dtype=torch.float32, device=dev)
        svar = torch.empty(D, dtype=torch.float32, device=dev)
        ws = hip.Workspace().get(2 * D * 4, dev)          # "Workspace >= 2*D floats", exactly
        hip.call(lib.dpk_bn1d_sync_forward, hip.ptr(xc), B, D, hip.ptr(wc), hip.ptr(bias_c), hip.ptr(mom), 1, hip.ptr(rvc),
                 hip.ptr(rmc), momentum, eps, hip.ptr(out), hip.ptr(ldj), hip.ptr(smean), hip.ptr(svar), hip.ptr(ws),
                 ws.numel(), st)
        assert rel_err(out.cpu().numpy(), u.detach().numpy()) <= 1e-5
        assert rel_err(ldj.cpu().numpy(), ildj.detach().numpy().reshape(1)) <= 1e-5
        assert rel_err(smean.cpu().numpy(), mean.detach().numpy()) <= 1e-5
        assert rel_err(svar.cpu().numpy(), var.detach().numpy()) <= 1e-5
        assert rel_err(rvc.cpu().numpy(), (rv.double() * momentum + var.detach() * (1 - momentum)).numpy()) <= 1e-5
        assert rel_err(rmc.cpu().numpy(), (rm.double() * momentum + mean.detach() * (1 - momentum)).numpy()) <= 1e-5

        sums = torch.empty(2 * D + 1, dtype=torch.float32, device=dev)
        hip.call(lib.dpk_bn1d_backward_sums, hip.ptr(xc), hip.ptr(guc), hip.ptr(gic), B, D, hip.ptr(smean), hip.ptr(svar),
                 eps, hip.ptr(sums), st)
        want = torch.cat([gu.double().sum(0), (gu.double() * xhat.detach()).sum(0), gi.double().sum().reshape(1)])
        assert grad_err(sums.cpu().numpy(), want.numpy()) <= 1e-5

        gx = torch.empty_like(xc)
        gw = torch.empty(D, dtype=torch.float32, device=dev)
        gb = torch.empty(D, dtype=torch.float32, device=dev)
        hip.call(lib.dpk_bn1d_sync_backward, hip.ptr(xc), hip.ptr(guc), B, B, D, hip.ptr(wc), hip.ptr(smean), hip.ptr(svar),
                 eps, hip.ptr(sums), hip.ptr(sums), hip.ptr(gx), hip.ptr(gw), hip.ptr(gb), st)
        assert grad_err(gx.cpu().numpy(), x64.grad.numpy()) <= 1e-4
        assert grad_err(gw.cpu().numpy(), w64.grad.numpy()) <= 1e-4
        assert grad_err(gb.cpu().numpy(), b64.grad.numpy()) <= 1e-4
        if bc._active is not None:                        # (the contract in force: every element of every output written)
            bc._active.expect_written(mom, out, ldj, smean, svar, sums, gx, gw, gb)


def direct_dgcspn_last_product_into_root():
    """dpk_spatial_prodroot_forward: the last depthwise product folded into the root of a model whose channel count is
    outside the three-stage kernel (16 > 8), so that DgcSpn.forward ends in it; against the oracle at the forward bar."""
    from deeprob.spn.models import DgcSpn
    from oracle import dgcspn_oracle as dorc
    from tests.util import randomise_dgc
    shape = (1, 8, 8)
    torch.manual_seed(13)
    model = DgcSpn(shape, out_classes=3, n_batch=16, sum_channels=16, depthwise=True)
    randomise_dgc(model, 71)
    model.eval()
    sd = _state(model)
    plan = dorc.schedule(shape, 16, 16, True, 0)
    model.cuda()
    for B in (1, 37):
        x = torch.randn(B, *shape, generator=torch.Generator().manual_seed(B))
        x[0, :, ::2] = float('nan')
        want = dorc.dgcspn_forward(sd, x, plan).detach().numpy()
        with torch.no_grad():
            got = model(x.cuda())
        assert rel_err(got.cpu().numpy(), want) <= 1e-5
        if bc._active is not None:
            bc._active.expect_written(got)
            assert 'dpk_spatial_prodroot_forward' in bc._active.called


def direct_spatial_gaussian_backward():
    """dpk_spatial_gaussian_backward, which no operator calls any more (SpatialGaussianFn.backward goes through the dropout
    variant at rate 0): called directly against float64 autograd of the layer (dgcspn.py:101-120), marginalised pixels
    included, at the gradient bar (1e-4 of the tensor's largest magnitude)."""
    from deeprob import hip
    from tests.util import grad_err
    lib = hip.load_library()
    dev = torch.device('cuda', torch.cuda.current_device())
    for B, K, C, H, W in ((1, 4, 1, 3, 3), (5, 8, 3, 6, 5), (33, 6, 2, 7, 9), (130, 16, 1, 12, 12)):
        gen = torch.Generator().manual_seed(B + K)
        x = torch.randn(B, C, H, W, generator=gen)
        x[torch.rand(x.shape, generator=gen) < 0.15] = float('nan')
        loc, scale = torch.randn(K, C, H, W, generator=gen), 0.5 + torch.rand(K, C, H, W, generator=gen)
        g = torch.randn(B, K, H, W, generator=gen)
        seen = ~torch.isnan(x)
        x64 = torch.where(seen, x, torch.zeros_like(x)).double().requires_grad_(True)
        loc64, scale64 = loc.double().requires_grad_(True), scale.double().requires_grad_(True)
        lp = torch.distributions.Normal(loc64, scale64).log_prob(x64[:, None])
        out = torch.where(seen[:, None], lp, torch.zeros_like(lp)).sum(2)
        (g.double() * out).sum().backward()
        xc, lc, sc, gc = x.to(dev), loc.to(dev), scale.to(dev), g.to(dev)
        gl, gs, gx = torch.empty_like(lc), torch.empty_like(sc), torch.empty_like(xc)
        hip.call(lib.dpk_spatial_gaussian_backward, hip.ptr(xc), hip.ptr(gc), hip.ptr(lc), hip.ptr(sc), B, K, C, H, W,
                 hip.ptr(gl), hip.ptr(gs), hip.ptr(gx), hip.stream_ptr(dev))
        assert grad_err(gl.cpu().numpy(), loc64.grad.numpy()) <= 1e-4
        assert grad_err(gs.cpu().numpy(), scale64.grad.numpy()) <= 1e-4
        assert grad_err(gx.cpu().numpy(), x64.grad.numpy()) <= 1e-4
        assert (gx.cpu()[~seen] == 0).all()                # "marginalised inputs get a zero gradient"
        if bc._active is not None:
            bc._active.expect_written(gl, gs, gx)


def _parametrisations(func):
    """Every parametrisation of an existing test as a dict, in collection order of its own parametrize marks."""
    axes = []
    for mark in getattr(func, 'pytestmark', []):
        if mark.name != 'parametrize':
            continue
        names = [n.strip() for n in mark.args[0].split(',')] if isinstance(mark.args[0], str) else list(mark.args[0])
        rows = []
        for v in mark.args[1]:
            if hasattr(v, 'values') and hasattr(v, 'marks'):      # pytest.param(...)
                v = v.values
            elif len(names) == 1:
                v = (v,)
            rows.append(dict(zip(names, v)))
        axes.append(rows)
    out = []
    for combo in itertools.product(*reversed(axes)):     # (the mark nearest the function varies fastest, as in pytest)
        kw = {}
        for part in combo:
            kw.update(part)
        out.append(kw)
    return out


def _fixture_def(mod, name):
    obj = getattr(mod, name, None)
    return obj if type(obj).__name__ == 'FixtureFunctionDefinition' else None


def _matches(value, want):
    return value in want if isinstance(want, (set, frozenset)) else value == want


def _select(mod, func, selector):
    cases = _parametrisations(func)
    argnames = set(cases[0]) if cases else set()
    selector = dict(selector)
    pick = selector.pop('#', None)
    for key in selector:
        assert key in argnames or _fixture_def(mod, key) is not None, (func.__name__, key)
    cases = [kw for kw in cases if all(_matches(kw[k], w) for k, w in selector.items() if k in argnames)]
    if pick is not None:
        assert max(pick) < len(cases), (func.__name__, pick, len(cases))
        cases = [kw for i, kw in enumerate(cases) if i in pick]
    for key, want in selector.items():                    # parametrised fixtures of the module (`mapping`)
        if key not in argnames:
            params = _fixture_def(mod, key)._fixture_function_marker.params
            values = [p for p in params if _matches(p, want)]
            assert values, (func.__name__, key, want)
            cases = [dict(kw, **{key: v}) for kw in cases for v in values]
    assert cases, 'the selector of {} picks no existing case: {}'.format(func.__name__, selector)
    return cases


def _short(v):
    s = repr(v) if not isinstance(v, (dict, tuple, list)) else '%04x' % (zlib.crc32(repr(v).encode()) & 0xFFFF)
    return s.replace("'", '')[:32]


def _replay_cases():
    cases = []
    for modname, funcname, selector in REPLAY:
        mod = importlib.import_module('tests.' + modname) if modname else None
        func = getattr(mod, funcname) if modname else globals()[funcname]
        for kw in _select(mod, func, selector):
            ident = '{}::{}[{}]'.format(modname or 'direct', funcname, '-'.join(_short(kw[k]) for k in sorted(kw)))
            cases.append(pytest.param((mod, func, kw), id=ident))
    return cases


class _Request:
    def __init__(self, param, stack):
        self.param = param
        self._stack = stack

    def addfinalizer(self, fn):
        self._stack.callback(fn)


def _fixture_value(mod, name, kw, env, stack):
    fdef = _fixture_def(mod, name)
    if fdef is not None:
        fn = fdef._get_wrapped_function()
        args = {}
        for p in inspect.signature(fn).parameters:
            args[p] = _Request(kw.get(name), stack) if p == 'request' else _fixture_value(mod, p, kw, env, stack)
        value = fn(**args)
        if inspect.isgenerator(value):
            gen, value = value, next(value)
            stack.callback(lambda: next(gen, None))
        return value
    if name == 'golden':
        return load_golden
    if name == 'request':
        return _Request(None, stack)
    return env[name]


def _call_case(case, env):
    """The existing test, as pytest would call it: the conftest's seeds, its module's fixtures, its own assertions."""
    mod, func, kw = case
    with contextlib.ExitStack() as stack:
        np.random.seed(42)
        torch.manual_seed(42)
        args = {}
        for p in inspect.signature(func).parameters:
            if p in kw and _fixture_def(mod, p) is None:
                args[p] = kw[p]
            else:
                args[p] = _fixture_value(mod, p, kw, env, stack)
        func(**args)


def _writers():
    if not _WRITERS:
        with open(os.path.join(ROOT, 'include', 'deeprob_hip.h')) as f:
            _WRITERS.extend(bc.writer_entry_points(f.read()))
    return _WRITERS


_WRITERS = []


_recorded = {}      # case id -> entry points called
_seconds = {}


def _replay(case, ident, pattern, env):
    t0 = time.time()
    with contract(pattern) as c:
        _call_case(case, env)
    torch.cuda.synchronize()
    _recorded.setdefault(ident, set()).update(c.called)
    _seconds[ident] = _seconds.get(ident, 0.0) + time.time() - t0
    print('replay {} 0x{:02X}: {} guarded allocations, {:.1f} s, entry points: {}'.format(
        ident, pattern, len(c.allocations), time.time() - t0, ' '.join(sorted(n for n in c.called if n in set(_writers())))))


_CASES = _replay_cases()


@pytest.mark.parametrize('pattern', bc.PATTERNS, ids=PATTERN_IDS)
@pytest.mark.parametrize('case', _CASES)
def test_replay(case, pattern, monkeypatch, tmp_path, request):
    _replay(case, request.node.callspec.id, pattern, dict(monkeypatch=monkeypatch, tmp_path=tmp_path))


def test_replay_covers_every_writer_entry_point(monkeypatch, tmp_path):
    """Union of the entry points recorded over the replay table == the header's writers minus NOT_COVERED."""
    env = dict(monkeypatch=monkeypatch, tmp_path=tmp_path)
    for p in _CASES:                      # (cases deselected from this run are replayed here, once)
        if not any(k.startswith(p.id + '-') or k == p.id for k in _recorded):
            _replay(p.values[0], p.id, bc.PATTERNS[0], env)
    writers = set(_writers())
    assert len(NOT_COVERED) <= MAX_NOT_COVERED and all(NOT_COVERED.values())
    assert set(NOT_COVERED) <= writers, set(NOT_COVERED) - writers
    covered = set().union(*_recorded.values()) & writers
    print('replay wall time per case (both patterns):')
    for k, s in sorted(_seconds.items(), key=lambda kv: -kv[1])[:15]:
        print('  {:6.1f} s  {}'.format(s, k))
    print('replay total {:.1f} s over {} cases'.format(sum(_seconds.values()), len(_seconds)))
    assert not covered & set(NOT_COVERED), 'listed as not covered but reached: {}'.format(sorted(covered & set(NOT_COVERED)))
    missing = writers - covered - set(NOT_COVERED)
    assert not missing, 'writer entry points no replayed case reaches: {}'.format(sorted(missing))


# ---- (b) bitwise independence ------------------------------------------------------------------------------------------
class _Plain:
    """What a scenario is handed outside the contract."""

    def frozen(self, *tensors):
        pass


@contextlib.contextmanager
def _mapping(which):
    """The RAT-SPN tile mappings, forced as the `mapping` fixture of test_ratspn_gpu.py forces them."""
    from deeprob.hip import load_library
    lib = load_library()
    prev = lib.dpk_ratspn_small_batch_max(0 if which == 'ring' else -1)
    prev_slice = lib.dpk_ratspn_slice_batch_min(0 if which == 'slice' else -1)
    try:
        yield
    finally:
        load_library().dpk_ratspn_small_batch_max(prev)
        load_library().dpk_ratspn_slice_batch_min(prev_slice)


def _state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _ratspn(c, kw, B, mapping='small', nan=False, layers=False):
    from deeprob.spn.models import GaussianRatSpn
    from oracle import ratspn_oracle as orc
    torch.manual_seed(5)
    model = GaussianRatSpn(random_state=42, **kw).eval()
    gen = torch.Generator().manual_seed(B)
    x = torch.randn(B, kw['in_features'], generator=gen) * 1.5
    if nan:
        x[torch.rand(x.shape, generator=gen) < 0.1] = float('nan')
        x[B // 2] = float('nan')
    want = orc.ratspn_forward(_state(model), x).numpy()
    model.cuda()
    xc = x.cuda()
    c.frozen(xc, *model.state_dict().values())
    outs = []
    with _mapping(mapping), torch.no_grad():
        for _ in range(2):                       # the second call: cached tables
            if layers:
                h = model.base_layer(xc)
                outs.append(h)
                for layer in model.layers:
                    h = layer(h)
                    outs.append(h)
                outs.append(model.root_layer(h))
            else:
                outs.append(model(xc))
            # (the marginalised-evidence hint that picks the next launch's kernel build is read by the host without
            # waiting: settled between the calls, as test_marginalised_inputs_on_both_kernel_builds settles it)
            torch.cuda.synchronize()

    def oracle(got):
        for o in ([got[len(got) // 2 - 1], got[-1]] if layers else got):
            assert rel_err(o.numpy(), want) <= 1e-5
    return outs, oracle


_R784 = dict(in_features=784, rg_depth=2, rg_repetitions=8)


def _coupling(c, depth, mask_kind, D=40, B=70):
    from deeprob.flows.layers.coupling import CouplingLayer1d
    from oracle import flows_oracle as forc
    gen = torch.Generator().manual_seed(D + depth)
    torch.manual_seed(1)
    layer = CouplingLayer1d(D, depth=depth, units=32, affine=True).eval()
    with torch.no_grad():
        if mask_kind == 'blocks':
            layer.mask.copy_((torch.arange(D) < D // 2).float())
            layer.inv_mask.copy_(1 - layer.mask)
        layer.scale_act.weight.fill_(0.7)
        for p in layer.network.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.3)
    lins = [(m.weight.detach().clone(), m.bias.detach().clone()) for m in layer.network if isinstance(m, torch.nn.Linear)]
    x = torch.randn(B, D, generator=gen)
    wu, wildj = forc.coupling_backward(x, layer.mask.clone(), layer.inv_mask.clone(), lins, torch.tensor([0.7]))
    layer.cuda()
    xc = x.cuda()
    c.frozen(xc, *layer.state_dict().values())
    outs = []
    with torch.no_grad():
        for _ in range(2):
            u, ildj = layer.apply_backward(xc)
            xr, ldj = layer.apply_forward(u)
            outs += [u, ildj, xr, ldj]

    def oracle(got):
        for i in (0, 4):
            assert rel_err(got[i].numpy(), wu.numpy()) <= 1e-5 and rel_err(got[i + 1].numpy(), wildj.numpy()) <= 1e-5
            assert torch.allclose(got[i + 2], x, atol=5e-6)
    return outs, oracle


def _maf(c, depth, D, units, act, seed, B=65):
    from tests import maf_cases as mc
    from tests.test_maf_gpu import _layer
    layer = _layer(D, units, depth=depth, act=act, seed=seed).eval()
    x = torch.randn(B, D, generator=torch.Generator().manual_seed(B)).cuda()
    c.frozen(x, *layer.state_dict().values())
    outs = []
    with torch.no_grad():
        for _ in range(2):
            u, ildj = layer.apply_backward(x)      # the fused density kernel (depth 1) / the chained route
            xs, ldj = layer.apply_forward(x)       # the sampling kernel (depth 1) / the deep sampling kernel
            outs += [u, ildj, xs, ldj]
    wm, a = mc.layer_params(layer)
    z = mc.conditioner64(wm, act, x.cpu().numpy())
    s = a * np.tanh(z[:, D:])
    want_u, want_ildj = (x.cpu().numpy() - z[:, :D]) * np.exp(-s), -s.sum(1)
    want_x, want_ldj = mc.sample_step_loop64(layer, act, x.cpu().numpy())

    def oracle(got):
        for i in (0, 4):
            assert rel_err(got[i].numpy(), want_u) <= 1e-4 and rel_err(got[i + 1].numpy().reshape(-1), want_ildj) <= 1e-4
            assert rel_err(got[i + 2].numpy(), want_x) <= 1e-4 and rel_err(got[i + 3].numpy().reshape(-1), want_ldj) <= 1e-4
    return outs, oracle


def _dgcspn(c, shape, classes, B, stream, monkeypatch):
    from deeprob.spn.models import DgcSpn
    from oracle import dgcspn_oracle as dorc
    from tests.util import randomise_dgc
    monkeypatch.setenv('DPK_DGC_STREAM_MIN_B', '0' if stream else '1000000000')
    torch.manual_seed(11)
    model = DgcSpn(shape, out_classes=classes, n_batch=8, sum_channels=8, depthwise=True)
    randomise_dgc(model, 70)
    model.eval()
    x = torch.randn(B, *shape, generator=torch.Generator().manual_seed(3))
    x[2, :, ::2] = float('nan')
    want = dorc.dgcspn_forward(_state(model), x, dorc.schedule(shape, 8, 8, True, 0)).detach().numpy()
    model.cuda()
    xc = x.cuda()
    c.frozen(xc, *model.state_dict().values())
    with torch.no_grad():
        outs = [model(xc), model(xc)]

    def oracle(got):
        for o in got:
            assert rel_err(o.numpy(), want) <= 1e-5
    return outs, oracle


def _flat_spn(c, workspace_route):
    from deeprob.spn.structure.io import digraph_to_spn
    from deeprob.spn.algorithms.inference import log_likelihood, mpe
    from oracle import flat_spn_oracle as forc
    from tests.flat_spn_cases import random_circuit, random_inputs
    d, family = random_circuit(7, 1)
    x = random_inputs(family, 63, 101)
    want, want_table = forc.log_likelihood(d, x, return_results=True)
    spn = digraph_to_spn(d)
    if workspace_route:
        spn.n_slots = 0
    xc = torch.from_numpy(x).cuda()
    c.frozen(xc)
    outs = []
    for _ in range(2):
        ll, table = log_likelihood(spn, xc, return_results=True)
        outs += [log_likelihood(spn, xc), ll, table, mpe(spn, xc.clone())]      # (mpe completes its argument in place)

    def oracle(got):
        for i in (0, 4):
            assert rel_err(got[i].numpy(), want) <= 1e-5 and rel_err(got[i + 2].numpy(), want_table) <= 1e-5
            done = got[i + 3].numpy()
            assert not np.isnan(done[:, :spn.n_features]).any()
            assert np.array_equal(done[~np.isnan(x)], x[~np.isnan(x)])
    return outs, oracle


def _flow2d(c):
    from oracle import flows2d_oracle as f2orc
    from tests.util import flow2d_model
    model = flow2d_model((3, 8, 8), dict(n_flows=1, n_blocks=1, channels=8), 5)
    x = torch.randn(5, 3, 8, 8, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        want = f2orc.log_prob(_state(model), x).numpy()
    model.cuda()
    xc = x.cuda()
    c.frozen(xc, *model.state_dict().values())
    with torch.no_grad():
        outs = [model(xc), model(xc)]

    def oracle(got):
        for o in got:
            assert rel_err(o.numpy(), want) <= 1e-5
    return outs, oracle


SCENARIOS = {
    'ratspn_fused_small': lambda c, mp: _ratspn(c, dict(_R784, rg_batch=2, rg_sum=2), 129, 'small'),
    'ratspn_fused_ring': lambda c, mp: _ratspn(c, dict(_R784, rg_batch=2, rg_sum=2), 129, 'ring'),
    'ratspn_fused_slice': lambda c, mp: _ratspn(c, dict(_R784, rg_batch=2, rg_sum=2), 129, 'slice'),
    'ratspn_fused_wide': lambda c, mp: _ratspn(c, dict(_R784, rg_batch=8, rg_sum=8), 129, 'small'),
    'ratspn_fused_nan_evidence': lambda c, mp: _ratspn(c, dict(_R784, rg_batch=2, rg_sum=2), 300, 'ring', nan=True),
    'ratspn_fused_valu': lambda c, mp: _ratspn(c, dict(in_features=15, rg_depth=2, rg_repetitions=3, rg_batch=3, rg_sum=5,
                                                       optimize_scale=True), 63, 'small', nan=True),
    'ratspn_layers_mfma_leaf': lambda c, mp: _ratspn(c, dict(_R784, rg_batch=4, rg_sum=2), 63, layers=True),
    'ratspn_layers_padded': lambda c, mp: _ratspn(c, dict(in_features=15, rg_depth=3, rg_repetitions=2, rg_batch=2, rg_sum=2),
                                                  1, layers=True),
    'ratspn_folded_i16': lambda c, mp: _ratspn(c, dict(in_features=100, rg_depth=2, rg_repetitions=8, rg_batch=16,
                                                              rg_sum=16, optimize_scale=True), 130, nan=True),
    'coupling1d_pairs': lambda c, mp: _coupling(c, 1, 'own'),
    'coupling1d_generic': lambda c, mp: _coupling(c, 1, 'blocks'),
    'coupling1d_mlp': lambda c, mp: _coupling(c, 2, 'own'),
    'maf_density_and_sampling': lambda c, mp: _maf(c, 1, 33, 40, 'tanh', 2),
    'maf_deep_sampling': lambda c, mp: _maf(c, 2, 10, 16, 'tanh', 4, B=33),
    'dgcspn_fused_levels': lambda c, mp: _dgcspn(c, (1, 20, 20), 3, 37, False, mp),
    'dgcspn_streaming_levels': lambda c, mp: _dgcspn(c, (1, 20, 20), 3, 37, True, mp),
    'flat_spn_on_chip': lambda c, mp: _flat_spn(c, False),
    'flat_spn_workspace': lambda c, mp: _flat_spn(c, True),
    'flows2d_conv_and_coupling': lambda c, mp: _flow2d(c),
}

_unstable = []      # scenarios whose two plain runs differed (held to their oracle only): recorded, and printed below


def _cpu(outs):
    return [torch.as_tensor(o).detach().cpu() for o in outs]


def _run_scenario(name, pattern, monkeypatch):
    np.random.seed(42)
    torch.manual_seed(42)
    if pattern is None:
        outs, oracle = SCENARIOS[name](_Plain(), monkeypatch)
    else:
        with contract(pattern) as c:
            outs, oracle = SCENARIOS[name](c, monkeypatch)
            assert c.called, 'the scenario reached no entry point'
            c.expect_written(*[o for o in outs if isinstance(o, torch.Tensor)])
    outs = _cpu(outs)
    oracle(outs)
    return [o.numpy().tobytes() for o in outs]


@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_results_do_not_depend_on_what_the_buffers_held(name, monkeypatch):
    plain = [_run_scenario(name, None, monkeypatch) for _ in range(2)]
    stable = plain[0] == plain[1]
    if not stable:
        _unstable.append(name)
    print('scenario {}: plain runs {}; oracle-only so far: {}'.format(
        name, 'bitwise equal' if stable else 'DIFFER (held to the oracle tolerance only)', _unstable))
    for pattern in bc.PATTERNS:
        got = _run_scenario(name, pattern, monkeypatch)      # (oracle, guards, frozen inputs, outputs written: inside)
        if stable:
            differ = [i for i, (a, b) in enumerate(zip(got, plain[0])) if a != b]
            assert not differ, 'outputs {} of {} differ bitwise from the plain runs under poison 0x{:02X}'.format(differ, name, pattern)
