"""Measurement: DgcSpn.sample and DgcSpn.sample_conditional (dpg_dgcspn_topdown) for the bench's DGC-SPN configuration --
DgcSpn((1, 28, 28), n_batch=8, sum_channels=8, depthwise=True, n_pooling=0), 50 % NaN evidence, B = 1024 and B = 8192 --
end to end and in parts: the bottom-up pass, the top-down launch of each mode, and the model's forward on the same batch
for scale.  Warm-up, then the median of repeated timed windows on device-resident inputs, with the spread (min, max) of the
windows; one JSON line, also written to profiles/dgcspn_topdown_bench_line.json.
The mpe_completion rows -- the whole call and its mode-3 launch, beside the mode-2 launch at the same shape, DgcSpn.mpe
(autograd) and DgcSpn.expectation, all in the same run -- are a line of their own, written to
profiles/dgcspn_mpe_bench_line.json; --mpe measures and writes that line alone.
usage: bench_dgcspn_topdown.py [--quick] [--trace] [--mpe] [--commit=TEXT]   (--trace: a few calls only, for a kernel trace in a run of its own)"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'deeprob-kit_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch
from deeprob.hip import dgc
from deeprob.spn.models import DgcSpn

assert torch.cuda.is_available(), 'a measurement needs a HIP device: there is no fallback'
QUICK, TRACE, MPE_ONLY = '--quick' in sys.argv, '--trace' in sys.argv, '--mpe' in sys.argv
MPE_ROWS = ('mpe_completion', 'topdown_mpe', 'topdown_posterior', 'mpe_autograd', 'expectation')
SAMPLING_ROWS = ('sample', 'sample_conditional', 'forward', 'bottom_up', 'topdown_prior', 'topdown_posterior')
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
model = DgcSpn((1, 28, 28), n_batch=8, sum_channels=8, depthwise=True, n_pooling=0).cuda().eval()
geom = dgc.product_geometry(model._product_layers())
loc, scale = model.base_layer.loc, model.base_layer.scale
line = {'workload': 'DgcSpn((1,28,28), n_batch=8, sum_channels=8, depthwise=True, n_pooling=0) sampling, 50 % NaN',
        'windows': WINDOWS, 'calls_per_window': CALLS}
mpe_line = dict(line, workload=line['workload'].replace('sampling', 'completion'))
for arg in sys.argv[1:]:
    if arg.startswith('--commit='):        # what the numbers were measured on, recorded with them
        line['commit'] = mpe_line['commit'] = arg[len('--commit='):]
for B in (1024, 8192):
    x = torch.randn(B, 1, 28, 28, device='cuda')
    x[torch.rand(B, 1, 28, 28, device='cuda') < 0.5] = float('nan')
    with torch.no_grad():
        acts, logw = model._upward_for_sampling(x), model._topdown_logw()
    out = model.sample_conditional(x, seed=1)
    obs = ~torch.isnan(x)
    assert torch.isfinite(out).all() and torch.equal(out[obs], x[obs]) and torch.isfinite(model.sample(B, seed=1)).all()

    def forward():
        with torch.no_grad():
            return model(x)

    def bottom_up():
        with torch.no_grad():
            return model._upward_for_sampling(x)

    runs = {
        'sample': lambda: model.sample(B, seed=1),
        'sample_conditional': lambda: model.sample_conditional(x, seed=1),
        'forward': forward,
        'bottom_up': bottom_up,
        'topdown_prior': lambda: dgc.dgcspn_topdown(1, B, model.in_features, geom, 1, None, None, None, logw, loc, scale, 1),
        'topdown_posterior': lambda: dgc.dgcspn_topdown(2, B, model.in_features, geom, 1, x, None, acts, logw, loc, scale, 1),
        'mpe_completion': lambda: model.mpe_completion(x),
        'topdown_mpe': lambda: dgc.dgcspn_topdown(dgc.DPG_MODE_MPE, B, model.in_features, geom, 1, x, None, acts, logw, loc,
                                                  scale, 0),
        'mpe_autograd': lambda: model.mpe(x),
        'expectation': lambda: model.expectation(x),
    }
    filled = model.mpe_completion(x)
    assert torch.isfinite(filled).all() and torch.equal(filled[obs], x[obs])
    if MPE_ONLY:
        runs = {name: runs[name] for name in MPE_ROWS}
    for name, fn in runs.items():
        med, lo, hi = timed(fn)
        for into in ([mpe_line] if name in MPE_ROWS else []) + ([line] if name in SAMPLING_ROWS else []):
            into['ms_%s_B%d' % (name, B)] = med
            into['ms_%s_B%d_min_max' % (name, B)] = [lo, hi]
    mpe_line['mpe_completion_rows_per_s_B%d' % B] = B / (mpe_line['ms_mpe_completion_B%d' % B] * 1e-3)
    mpe_line['topdown_mpe_over_posterior_B%d' % B] = mpe_line['ms_topdown_mpe_B%d' % B] / mpe_line['ms_topdown_posterior_B%d' % B]
    if MPE_ONLY:
        continue
    line['sample_rows_per_s_B%d' % B] = B / (line['ms_sample_B%d' % B] * 1e-3)
    line['sample_conditional_rows_per_s_B%d' % B] = B / (line['ms_sample_conditional_B%d' % B] * 1e-3)
    line['sample_conditional_over_forward_B%d' % B] = line['ms_sample_conditional_B%d' % B] / line['ms_forward_B%d' % B]
for name, record in (('dgcspn_topdown_bench_line.json', line), ('dgcspn_mpe_bench_line.json', mpe_line)):
    if MPE_ONLY and record is line:
        continue
    text = json.dumps(record)
    print(text)
    if not (QUICK or TRACE):
        with open(os.path.join(ROOT, 'profiles', name), 'w') as f:
            f.write(text + '\n')
