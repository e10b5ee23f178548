"""Measurement: DgcSpn.posterior_moments (exact posterior mean and variance of the missing pixels, dpm_dgcspn_moments) next to
DgcSpn.mpe and one DgcSpn.sample_conditional draw on the same batch -- the benchmark's DGC-SPN configuration,
DgcSpn((1, 28, 28), n_batch=8, sum_channels=8, depthwise=True, n_pooling=0), 50 % NaN evidence, B = 1 024 and B = 8 192 -- and
the two parts of a call (the bottom-up pass it shares with sample_conditional, the top-down launch of the moments) on
their own.  With --example also the 16 / 32 channel model whose flow maps set the workspace (32 x 59 x 59), B = 1 024.
Warm-up, then the median of repeated timed windows on device-resident inputs, with the spread (min, max) of the windows;
one JSON line, also written to profiles/dgcspn_moments_bench_line.json.
usage: bench_dgcspn_moments.py [--quick] [--example]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'deeprob-kit_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch
from deeprob.hip import Workspace, dgcm
from deeprob.spn.models import DgcSpn

assert torch.cuda.is_available(), 'a measurement needs a HIP device: there is no fallback'
QUICK, EXAMPLE = '--quick' in sys.argv, '--example' in sys.argv
WINDOWS, CALLS = (3, 3) if QUICK else (9, 20)


def timed(fn, windows=WINDOWS, calls=CALLS):
    """(median, min, max) over `windows` windows of `calls` back-to-back calls, milliseconds per call"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) / calls * 1e3)
    return statistics.median(per), min(per), max(per)


def measure(line, tag, model, B, windows=WINDOWS, calls=CALLS):
    x = torch.randn(B, 1, 28, 28, device='cuda')
    x[torch.rand(B, 1, 28, 28, device='cuda') < 0.5] = float('nan')
    geom = dgcm.product_geometry(model._product_layers())
    with torch.no_grad():
        acts, logw = model._upward_for_sampling(x), model._topdown_logw()
    ws = Workspace()
    mean, var = model.posterior_moments(x)
    obs = ~torch.isnan(x)
    assert torch.isfinite(mean).all() and torch.equal(mean[obs], x[obs]) and (var[~obs] > 0).all() and (var[obs] == 0).all()
    est = model.mpe(x)
    line['max_abs_expectation_minus_mpe_%s_B%d' % (tag, B)] = float((mean - est).abs().max())
    line['workspace_bytes_%s_B%d' % (tag, B)] = dgcm.workspace_bytes(B, geom)

    def bottom_up():
        with torch.no_grad():
            return model._upward_for_sampling(x)

    runs = {
        'posterior_moments': lambda: model.posterior_moments(x),
        'expectation': lambda: model.expectation(x),
        'bottom_up': bottom_up,
        'topdown_moments': lambda: dgcm.dgcspn_moments(model.in_features, geom, 1, x, None, acts, logw, model.base_layer.loc,
                                                       model.base_layer.scale, ws),
        'mpe': lambda: model.mpe(x),
        'sample_conditional': lambda: model.sample_conditional(x, seed=1),
    }
    for name, fn in runs.items():
        med, lo, hi = timed(fn, windows, calls)
        line['ms_%s_%s_B%d' % (name, tag, B)] = med
        line['ms_%s_%s_B%d_min_max' % (name, tag, B)] = [lo, hi]
    pm = line['ms_posterior_moments_%s_B%d' % (tag, B)]
    line['posterior_moments_over_mpe_%s_B%d' % (tag, B)] = pm / line['ms_mpe_%s_B%d' % (tag, B)]
    line['posterior_moments_over_sample_conditional_%s_B%d' % (tag, B)] = pm / line['ms_sample_conditional_%s_B%d' % (tag, B)]
    line['topdown_over_bottom_up_%s_B%d' % (tag, B)] = (line['ms_topdown_moments_%s_B%d' % (tag, B)]
                                                        / line['ms_bottom_up_%s_B%d' % (tag, B)])
    line['posterior_moments_images_per_s_%s_B%d' % (tag, B)] = B / (pm * 1e-3)


def scores_per_image(model):
    """sum over the sum layers of Cout x Cin x positions, and the root's inputs: what the top-down pass evaluates (each in
    three passes, two of them with an expf)"""
    geom = dgcm.product_geometry(model._product_layers())
    return sum(geom[j][0] * geom[j - 1][3] * geom[j - 1][4] * geom[j - 1][5] for j in range(1, len(geom))), \
        geom[-1][3] * geom[-1][4] * geom[-1][5]


_w = torch.zeros(64, device='cuda')
for _ in range(600):      # (the runtime's one-off per-queue pool growth, a host stall around the 200th launch, out of the way)
    _w.add_(1.0)
torch.cuda.synchronize()
torch.manual_seed(0)
model = DgcSpn((1, 28, 28), n_batch=8, sum_channels=8, depthwise=True, n_pooling=0).cuda().eval()
line = {'workload': 'DgcSpn posterior moments, (1, 28, 28), 50 % NaN; c4: n_batch 8, sum_channels 8, depthwise, n_pooling 0 '
                    '(the benchmark\'s); example: n_batch 16, sum_channels 32',
        'windows': WINDOWS, 'calls_per_window': CALLS, 'max_groups': dgcm.DPM_MAX_GROUPS}
line['sum_scores_per_image_c4'], line['root_scores_per_image_c4'] = scores_per_image(model)
for B in (1024,) if QUICK else (1024, 8192):
    measure(line, 'c4', model, B)
if EXAMPLE:
    big = DgcSpn((1, 28, 28), n_batch=16, sum_channels=32, depthwise=True, n_pooling=0).cuda().eval()
    line['sum_scores_per_image_example'], line['root_scores_per_image_example'] = scores_per_image(big)
    line['windows_example'], line['calls_per_window_example'] = 5, 3
    measure(line, 'example', big, 1024, 5, 3)
text = json.dumps(line)
print(text)
if not QUICK:
    with open(os.path.join(ROOT, 'profiles', 'dgcspn_moments_bench_line.json'), 'w') as f:
        f.write(text + '\n')
