"""Measurement: posterior queries on the reference-learned 72-node circuit over 16 binary variables at B = 2^20 with 30 %
NaN -- expectation(root, x), the four-order launch behind kurtosis (and kurtosis itself, with its float64 statistics),
posterior on one variable -- beside log_likelihood and mpe in the same run, and beside the only way to get at the posterior
flows without the fused launch: log_likelihood(return_results=True) followed by eval_backward on the same rows, which
writes two [n_nodes, B] float32 tables to device memory (and still lacks the gather over the leaves).
Warm-up, then the median of repeated timed windows on device-resident inputs, each window ended by a device synchronise;
one JSON line, printed and written to --out (default profiles/flat_spn_posterior_bench_line.json).
usage: bench_flat_spn_posterior.py [--quick] [--out PATH]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'deeprob-kit_amd'), ROOT]
import numpy as np
import torch
from deeprob.hip import spnq
from deeprob.spn.structure.io import load_spn_json
from deeprob.spn.algorithms.inference import log_likelihood, mpe, posterior
from deeprob.spn.algorithms.gradient import eval_backward
from deeprob.spn.algorithms.moments import expectation, kurtosis

QUICK = '--quick' in sys.argv
WINDOWS, CALLS = (3, 3) if QUICK else (7, 10)
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(
    ROOT, 'profiles', 'flat_spn_posterior_bench_line.json')


def timed(fn):
    """median over WINDOWS windows of CALLS back-to-back calls, seconds per call"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) / CALLS)
    return statistics.median(per)


spn = load_spn_json(os.path.join(ROOT, 'tests', 'golden', 'spn_binary16.json'))
rs = np.random.RandomState(0)
B = 1 << (14 if QUICK else 20)
x = (rs.rand(B, 16) < 0.5).astype(np.float32)
x[rs.rand(B, 16) < 0.3] = np.nan
xd = torch.from_numpy(x).cuda()
out = torch.empty_like(xd)


def mpe_into():
    out.copy_(xd)
    mpe(spn, out, inplace=True)


def composition():
    _, table = log_likelihood(spn, xd, return_results=True)
    return eval_backward(spn, table)


t_copy = timed(lambda: out.copy_(xd))
t_ll = timed(lambda: log_likelihood(spn, xd))
t_mpe = timed(mpe_into) - t_copy
t_exp = timed(lambda: expectation(spn, xd))
t_m4 = timed(lambda: spnq.flat_spn_posterior(spn, xd, spnq.DPQ_MODE_MOMENTS, n_orders=4))
t_kurt = timed(lambda: kurtosis(spn, xd))
t_post = timed(lambda: posterior(spn, xd, 0))
t_ws = timed(lambda: spnq.flat_spn_posterior(spn, xd, spnq.DPQ_MODE_MOMENTS, n_orders=1, force_workspace=True))
t_comp = timed(composition)
line = json.dumps({
    'workload': 'vanilla SPN posterior queries, 16 binary vars, 72 nodes, 30 % NaN', 'batch': B,
    'ms_log_likelihood': t_ll * 1e3, 'ms_mpe': t_mpe * 1e3, 'ms_expectation': t_exp * 1e3,
    'ms_moments_four_orders_launch': t_m4 * 1e3, 'ms_kurtosis': t_kurt * 1e3, 'ms_posterior_one_variable': t_post * 1e3,
    'ms_expectation_workspace_route': t_ws * 1e3, 'ms_log_likelihood_tables_then_eval_backward': t_comp * 1e3,
    'expectation_rows_per_s': B / t_exp, 'posterior_rows_per_s': B / t_post, 'mpe_rows_per_s': B / t_mpe,
    'log_likelihood_rows_per_s': B / t_ll, 'composition_rows_per_s': B / t_comp,
    'composition_time_over_expectation_time': t_comp / t_exp,
    'windows': WINDOWS, 'calls_per_window': CALLS})
print(line)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as f:
    f.write(line + '\n')
