"""Measurement: the node-graph SPN queries on the reference-learned 72-node circuit over 16 binary variables --
log_likelihood, mpe and sample at B = 2^20 with 30 % NaN, eval_backward at B = 2^17, seconds per EM iteration on a
100 000-row batch -- next to the numpy restatement (tests/flat_spn_query_ref.py) on the host for at most 100 000 rows.
Warm-up, then the median of repeated timed windows on device-resident inputs; one JSON line.
usage: bench_flat_spn_queries.py [--quick]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'deeprob-kit_amd'), ROOT]
import numpy as np
import torch
from deeprob.spn.structure.io import load_spn_json
from deeprob.spn.algorithms.inference import log_likelihood, mpe
from deeprob.spn.algorithms.sampling import sample
from deeprob.spn.algorithms.gradient import eval_backward
from deeprob.spn.learning import expectation_maximization
from tests import flat_spn_query_ref as qref

QUICK = '--quick' in sys.argv
WINDOWS, CALLS = (3, 3) if QUICK else (7, 10)


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


def host(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


path = os.path.join(ROOT, 'tests', 'golden', 'spn_binary16.json')
d = json.load(open(path))
spn = load_spn_json(path)
rs = np.random.RandomState(0)
B, BG, BE, NH = 1 << 20, 1 << 17, 100000, 100000
full = (rs.rand(B, 16) < 0.5).astype(np.float32)
x = full.copy()
x[rs.rand(B, 16) < 0.3] = np.nan
xd = torch.from_numpy(x).cuda()
out = torch.empty_like(xd)


def into(fn):
    out.copy_(xd)
    fn(spn, out, inplace=True)


t_copy = timed(lambda: out.copy_(xd))
t_ll = timed(lambda: log_likelihood(spn, xd))
t_mpe = timed(lambda: into(mpe)) - t_copy
t_smp = timed(lambda: into(lambda s, o, inplace: sample(s, o, inplace=inplace, seed=1))) - t_copy
table = log_likelihood(spn, xd[:BG], return_results=True)[1]
t_bwd = timed(lambda: eval_backward(spn, table))

# EM: every call draws one batch of BE rows out of 2 BE
data = torch.from_numpy(full[:2 * BE]).cuda()
iters = 5 if QUICK else 20
expectation_maximization(spn, data, num_iter=2, batch_perc=0.5, random_init=False, random_state=0, verbose=False)
torch.cuda.synchronize()
t0 = time.perf_counter()
expectation_maximization(spn, data, num_iter=iters, batch_perc=0.5, random_init=False, random_state=0, verbose=False)
torch.cuda.synchronize()
t_em = (time.perf_counter() - t0) / iters       # includes drawing the index rows on the host

st = qref.State(d)
xs = x[:NH]
lls = [None]
h_ll = host(lambda: lls.__setitem__(0, qref.forward(st, xs)))
h_mpe = host(lambda: qref.mpe(st, xs, lls[0]))
h_bwd = host(lambda: qref.backward(st, lls[0]))
h_em = host(lambda: qref.em_step(qref.State(d), full[:NH], 0.5))
print(json.dumps({
    'workload': 'vanilla SPN queries, 16 binary vars, 72 nodes, 30 % NaN', 'batch': B,
    'log_likelihood_rows_per_s': B / t_ll, 'mpe_rows_per_s': B / t_mpe, 'sample_rows_per_s': B / t_smp,
    'mpe_time_over_log_likelihood_time': t_mpe / t_ll, 'ms_log_likelihood': t_ll * 1e3, 'ms_mpe': t_mpe * 1e3,
    'ms_sample': t_smp * 1e3, 'eval_backward_batch': BG, 'eval_backward_rows_per_s': BG / t_bwd,
    'em_batch': BE, 's_per_em_iteration': t_em,
    'host_rows': NH, 'host_log_likelihood_rows_per_s': NH / h_ll, 'host_mpe_rows_per_s': NH / (h_ll + h_mpe),
    'host_eval_backward_rows_per_s': NH / h_bwd, 'host_s_per_em_iteration': h_em,
    'windows': WINDOWS, 'calls_per_window': CALLS}))
