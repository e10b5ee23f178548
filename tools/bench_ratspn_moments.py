"""Measurement: RatSpn.posterior_moments (exact posterior mean and variance of the missing entries, dpr_ratspn_moments) next
to RatSpn.mpe and RatSpn.sample_conditional on the same batch -- 784 variables, depth 2, 8 repetitions, 16 / 16 nodes, 50 %
NaN evidence, B = 4096 and B = 65 536 -- and the two parts of a call (the bottom-up pass all three share, the top-down launch
of the moments) on their own.
Warm-up, then the median of repeated timed windows on device-resident inputs, with the spread (min, max) of the windows;
one JSON line, also written to profiles/ratspn_moments_bench_line.json.
usage: bench_ratspn_moments.py [--quick] [--trace]     (--trace: a few calls only, for a kernel trace in a run of its own)"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'deeprob-kit_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch
from deeprob.hip import rat
from deeprob.spn.models import GaussianRatSpn

assert torch.cuda.is_available(), 'a measurement needs a HIP device: there is no fallback'
QUICK, TRACE = '--quick' in sys.argv, '--trace' in sys.argv
WINDOWS, CALLS = (3, 3) if QUICK or TRACE else (9, 20)


def timed(fn):
    """(median, min, max) over WINDOWS windows of CALLS back-to-back calls, milliseconds per call"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) / CALLS * 1e3)
    return statistics.median(per), min(per), max(per)


_w = torch.zeros(64, device='cuda')
for _ in range(600):      # (the runtime's one-off per-queue pool growth, a host stall around the 200th launch, out of the way)
    _w.add_(1.0)
torch.cuda.synchronize()
torch.manual_seed(0)
model = GaussianRatSpn(784, rg_depth=2, rg_repetitions=8, rg_batch=16, rg_sum=16, random_state=42).cuda().eval()
dist, p0, p1 = model._leaf_params()
line = {'workload': 'RatSpn posterior moments, 784 vars, depth 2, 8 repetitions, 16/16 nodes, 50 % NaN',
        'windows': WINDOWS, 'calls_per_window': CALLS,
        # scores a row: the bottom-up pass forms each sum input once, the top-down pass forms the same ones again (the root's in three passes)
        'scores_per_row_bottom_up': 8 * 2 * 16 * 256 + 2048, 'scores_per_row_top_down': 8 * 2 * 16 * 256 + 3 * 2048}
for B in (4096, 65536):
    x = torch.randn(B, 784, device='cuda')
    x[torch.rand(B, 784, device='cuda') < 0.5] = float('nan')
    acts, logw, src = model._upward_for_mpe(x), model._topdown_logw(), model._topdown_src()
    mean, var = model.posterior_moments(x)
    obs = ~torch.isnan(x)
    assert torch.isfinite(mean).all() and torch.equal(mean[obs], x[obs]) and (var[~obs] > 0).all() and (var[obs] == 0).all()
    runs = {
        'posterior_moments': lambda: model.posterior_moments(x),
        'expectation': lambda: model.expectation(x),
        'sample_conditional': lambda: model.sample_conditional(x, seed=1),
        'mpe': lambda: model.mpe(x),
        'bottom_up': lambda: model._upward_for_mpe(x),
        'topdown_moments': lambda: rat.ratspn_moments(dist, model._fused_ctx, x, None, acts, logw, src, p0, p1),
    }
    for name, fn in runs.items():
        med, lo, hi = timed(fn)
        line['ms_%s_B%d' % (name, B)] = med
        line['ms_%s_B%d_min_max' % (name, B)] = [lo, hi]
    line['posterior_moments_over_sample_conditional_B%d' % B] = (line['ms_posterior_moments_B%d' % B]
                                                                 / line['ms_sample_conditional_B%d' % B])
    line['topdown_over_bottom_up_B%d' % B] = line['ms_topdown_moments_B%d' % B] / line['ms_bottom_up_B%d' % B]
    line['posterior_moments_rows_per_s_B%d' % B] = B / (line['ms_posterior_moments_B%d' % B] * 1e-3)
text = json.dumps(line)
print(text)
if not (QUICK or TRACE):
    with open(os.path.join(ROOT, 'profiles', 'ratspn_moments_bench_line.json'), 'w') as f:
        f.write(text + '\n')
