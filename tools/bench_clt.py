"""BinaryCLT on the HIP path against the numpy restatement (tests/clt_ref.py) on the same host.

Workload: 60 000 x 784 binary rows of a 4-prototype mixture with 20 % noise, generated here from a seed.  Timed, each as
the median of ``--runs`` calls after one warm-up, with a host clock around work that ends in a device synchronise:

    fit            numpy rows in (upload, dpc_pack_bits, dpc_pair_counts, the read of the counts, the host arithmetic,
                   Prim, the CPTs);
    ll_complete    log_likelihood of the 60 000 training rows, resident on the device;
    ll_nan         log_likelihood of the same rows with 30 % of the entries NaN;
    mpe, sample    on the 30 % NaN rows;
    marginals      the posterior marginal of every NaN entry of those rows (checked against the float64 restatement,
                   tests/marginals_ref.py).

The restatement runs once: ``fit`` on all rows, the queries on the first ``--ref-rows`` rows (it holds a
[D, 2, rows] float32 message array); ``speedup`` compares seconds per row.  The device results are checked against it on
those rows.  The split of device time over the kernels comes from one ``rocprofv3 --kernel-trace --stats`` run of this
script with ``--profile-child``.  Writes one JSON line to ``--out`` (default profiles/clt_bench_line.json) and prints it.

    python tools/bench_clt.py [--rows 60000] [--cols 784] [--ref-rows 4096] [--no-profile] [--no-restatement]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, 'deeprob-kit_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

DATA_SEED, ROOT_VAR, ALPHA, SAMPLE_SEED = 1, 0, 0.1, 7
KERNELS = ('pack_bits', 'pack_query', 'pair_counts', 'query_kernel<0>', 'query_kernel<1>', 'query_kernel<2>',
           'clt_marginals_kernel')


def workload(rows, cols, n_clusters=4, noise=0.2):
    rs = np.random.RandomState(DATA_SEED)
    protos = rs.randint(0, 2, size=(n_clusters, cols))
    x = protos[rs.randint(0, n_clusters, size=rows)]
    flip = rs.rand(rows, cols) < noise
    x = np.where(flip, rs.randint(0, 2, size=(rows, cols)), x).astype(np.float32)
    x_nan = x.copy()
    x_nan[rs.rand(rows, cols) < 0.3] = np.nan
    return x, x_nan


def timed(fn, runs):
    import torch
    fn()                                    # warm-up: library load, allocator, first launches
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, times


def fit_model(x):
    from deeprob.spn.structure.cltree import BinaryCLT
    clt = BinaryCLT(list(range(x.shape[1])), root=ROOT_VAR)
    clt.fit(x, [[0, 1]] * x.shape[1], alpha=ALPHA)
    return clt


def steps(clt, xd, xd_nan):
    return {'ll_complete': lambda: clt.log_likelihood(xd), 'll_nan': lambda: clt.log_likelihood(xd_nan),
            'mpe': lambda: clt.mpe(xd_nan), 'sample': lambda: clt.sample(xd_nan, seed=SAMPLE_SEED),
            'marginals': lambda: clt.marginals(xd_nan)}


def kernel_split(rows, cols):
    """Device time per kernel of one fit and one call of every query, from a rocprofv3 run of this script (a fresh
    child process)."""
    if shutil.which('rocprofv3') is None:
        return {'error': 'rocprofv3 not found'}
    out = tempfile.mkdtemp(prefix='clt_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', out, '-o', 't', '--output-format', 'csv', '--',
               sys.executable, os.path.abspath(__file__), '--profile-child', '--rows', str(rows), '--cols', str(cols)]
        r = subprocess.run(cmd, cwd=out, capture_output=True, text=True, timeout=600)
        found = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
        if r.returncode != 0 or not found:
            return {'error': 'rocprofv3 run failed (rc {}): {}'.format(r.returncode, r.stderr[-300:])}
        split, total = {}, 0.0
        for row in csv.DictReader(open(found[0])):
            name, ns = row['Name'], float(row['TotalDurationNs'])
            key = next((k for k in KERNELS if k in name.replace(' ', '')), 'other (torch copies and fills)')
            split[key] = split.get(key, 0.0) + ns / 1e6
            total += ns / 1e6
        return {'device_ms_total': round(total, 3), 'device_ms': {k: round(v, 3) for k, v in sorted(split.items())}}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=60000)
    ap.add_argument('--cols', type=int, default=784)
    ap.add_argument('--ref-rows', type=int, default=4096)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clt_bench_line.json'))
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--no-restatement', action='store_true')
    ap.add_argument('--profile-child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_clt.py measures on a HIP device; none found')
    x, x_nan = workload(args.rows, args.cols)
    xd, xd_nan = torch.from_numpy(x).cuda(), torch.from_numpy(x_nan).cuda()
    if args.profile_child:
        clt = fit_model(x)
        for fn in steps(clt, xd, xd_nan).values():
            fn()
        torch.cuda.synchronize()
        return
    line = {'bench': 'clt', 'rows': args.rows, 'cols': args.cols, 'nan_share': 0.3, 'runs': args.runs,
            'method': 'host clock around calls that end in a device synchronise; median after one warm-up',
            'hip_seconds': {}, 'hip_seconds_all': {}}
    clt, times = timed(lambda: fit_model(x), args.runs)
    results = {}
    todo = [('fit', times)]
    for name, fn in steps(clt, xd, xd_nan).items():
        results[name], t = timed(fn, args.runs)
        todo.append((name, t))
    for name, t in todo:
        line['hip_seconds'][name] = round(statistics.median(t), 5)
        line['hip_seconds_all'][name] = [round(v, 5) for v in t]
    if not args.no_restatement:
        from tests import clt_ref as ref
        from tests import marginals_ref as mref
        n = min(args.ref_rows, args.rows)
        t0 = time.perf_counter()
        bfs, tree, params = ref.fit(x, ROOT_VAR, ALPHA)
        seconds = {'fit': time.perf_counter() - t0}
        want = {}
        for name, fn in (('ll_complete', lambda: ref.log_likelihood(bfs, tree, params, x[:n])),
                         ('ll_nan', lambda: ref.log_likelihood(bfs, tree, params, x_nan[:n])),
                         ('mpe', lambda: ref.mpe(bfs, tree, params, x_nan[:n])),
                         ('sample', lambda: ref.sample_replay(bfs, tree, params, x_nan[:n], SAMPLE_SEED)),
                         ('marginals', lambda: mref.tree_marginals(bfs, tree, params, x_nan[:n], np.float64))):
            t0 = time.perf_counter()
            want[name] = fn()
            seconds[name] = time.perf_counter() - t0
        line['restatement_rows'] = {'fit': args.rows, 'queries': n}
        line['restatement_seconds'] = {k: round(v, 3) for k, v in seconds.items()}
        line['speedup_per_row'] = {
            k: round(seconds[k] / (args.rows if k == 'fit' else n) / (line['hip_seconds'][k] / args.rows), 1) for k in seconds}

        def rel(got, ref_values):
            got = got.cpu().numpy().reshape(-1)[:n].astype(np.float64)
            return float(np.max(np.abs(got - ref_values) / np.maximum(1.0, np.abs(ref_values))))
        replay, near = want['sample']
        line['checks'] = {
            'same_tree': bool(np.array_equal(clt.tree, tree)),
            'params_max_abs_diff': float(np.max(np.abs(clt.params - params))),
            'll_complete_rel_err': rel(results['ll_complete'], want['ll_complete'].astype(np.float64)),
            'll_nan_rel_err': rel(results['ll_nan'], want['ll_nan'].astype(np.float64)),
            'mpe_rows_equal_share': float(np.mean((results['mpe'][:n].cpu().numpy() == want['mpe']).all(axis=1))),
            'sample_rows_equal_share_outside_window': float(np.mean(
                (results['sample'][:n].cpu().numpy() == replay).all(axis=1)[~near])),
            'sample_rows_inside_window_share': float(np.mean(near)),
            'marginals_max_abs_err': float(np.max(np.abs(results['marginals'][:n].cpu().numpy() - want['marginals'])))}
        line['multiple_of_ll_nan'] = {'marginals': round(line['hip_seconds']['marginals'] / line['hip_seconds']['ll_nan'], 2)}
    if not args.no_profile:
        line['kernel_split'] = kernel_split(args.rows, args.cols)
    text = json.dumps(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
