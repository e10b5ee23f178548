"""LearnSPN on continuous data on the HIP path against the numpy restatement (tests/learn_cont_ref.py) on the same host.

Workload: ``--rows`` x ``--cols`` float32 rows of a two-cluster mixture whose columns form blocks of 4 that share one
latent (tests/learn_cont_ref.py:two_blocks, widened), ``split_cols=rdc_cols`` (k = 20 random features per column),
k-means row splits, min_rows_slice = 512, MLE Gaussian leaves.  ``learn_spn`` end to end (upload, kernels, torch.sort,
host score algebra, the FlatSpn) is the median of ``--runs`` runs after one warm-up; the restatement runs once.  A second
figure times ``dpl_rdc_gram`` alone on the root task (all rows, all columns), the library's one dense product, on the VALU
and on the matrix core (``v_mfma_f64_16x16x4_f64``).
Writes profiles/learnspn_cont_bench_line.json and prints it.

    python tools/bench_learnspn_cont.py [--rows 20000] [--cols 16] [--runs 5] [--no-restatement]
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, 'deeprob-kit_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

SEED, DATA_SEED, MIN_ROWS, K = 42, 1, 512, 20


def workload(rows, cols):
    rs = np.random.RandomState(DATA_SEED)
    z = rs.randint(0, 2, size=rows)
    latent = rs.randn(rows, -(-cols // 4))
    x = np.stack([latent[:, c // 4] * (1.0 + 0.5 * (c % 4)) + 0.05 * rs.randn(rows) for c in range(cols)], axis=1)
    return (x + 12.0 * z[:, None]).astype(np.float32)


def run_hip(x):
    import torch
    from deeprob.spn.learning import learn_spn, learnspn_cont
    from deeprob.spn.learning.splitting.rdc import rdc_cols
    from deeprob.spn.structure.leaf import Gaussian
    cols = x.shape[1]
    domains = [(float(x[:, i].min()), float(x[:, i].max())) for i in range(cols)]
    t0 = time.perf_counter()
    flat = learn_spn(x, [Gaussian] * cols, domains, split_rows='kmeans', split_cols=rdc_cols, min_rows_slice=MIN_ROWS,
                     random_state=SEED, verbose=False)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, flat, learnspn_cont.last_info()


def time_gram(x, runs, mfma):
    """Milliseconds of dpl_rdc_gram (both launches, tables uploaded) on the root task on the matrix core or the VALU, by
    device events, median of ``runs``; and the float64 GFLOP/s of the upper triangle's products."""
    import torch
    from deeprob.hip import learn as L
    from deeprob.spn.learning.learnspn_cont import to_device_f
    from deeprob.spn.learning.splitting.rdc import draw_features
    n, m = x.shape
    dev = to_device_f(x)
    row_index = torch.arange(n, dtype=torch.int32, device=dev.device)
    ranks, _ = L.ecdf_ranks(dev, row_index, np.arange(m), np.zeros(m, np.int64), np.full(m, n))
    w, b = draw_features(np.random.RandomState(SEED), m, K, 1.0 / 6.0)
    times = []
    for i in range(runs + 1):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        L.rdc_gram(ranks, [(n, m, 0)], K, w, b, mfma=mfma)
        stop.record()
        stop.synchronize()
        if i:
            times.append(start.elapsed_time(stop))
    ms = statistics.median(times)
    flops = 2.0 * n * (m * K) * (m * K + 1) / 2.0         # the products of the upper triangle
    return round(ms, 3), round(flops / (ms * 1e-3) / 1e9, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=20000)
    ap.add_argument('--cols', type=int, default=16)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--no-restatement', action='store_true')
    args = ap.parse_args()
    x = workload(args.rows, args.cols)
    run_hip(x)                  # warm-up: library load, allocator, first launches
    times = []
    for _ in range(args.runs):
        t, flat, info = run_hip(x)
        times.append(t)
    from deeprob.hip import learn as L
    gram = {name: time_gram(x, args.runs, flag) for name, flag in (('valu', False), ('mfma', True))}
    line = {'bench': 'learnspn_cont', 'rows': args.rows, 'cols': args.cols, 'split_rows': 'kmeans', 'split_cols': 'rdc', 'k': K,
            'min_rows_slice': MIN_ROWS, 'hip_seconds_median': round(statistics.median(times), 4),
            'hip_seconds_all': [round(t, 4) for t in times], 'nodes': flat.n_nodes, 'generations': info['generations'],
            'kernels': info['kernels'], 'lloyd_launches': info['lloyd_launches'],
            'max_tasks_in_a_generation': max(info['tasks_per_generation']), 'root_gram_ms': {name: v[0] for name, v in gram.items()},
            'root_gram_f64_gflops': {name: v[1] for name, v in gram.items()},
            'gram_products_in_use': 'mfma' if L.GRAM_USE_MFMA else 'valu'}
    if not args.no_restatement:
        from tests import learn_cont_ref as ref
        from tests.test_learn_cont_gpu import circuits_differ
        t0 = time.perf_counter()
        want = ref.learn_spn(x, min_rows_slice=MIN_ROWS, random_state=SEED, k=K)
        line['restatement_seconds'] = round(time.perf_counter() - t0, 3)
        line['speedup_over_restatement'] = round(line['restatement_seconds'] / line['hip_seconds_median'], 2)
        line['same_graph_as_restatement'] = circuits_differ(flat, want) is None
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'learnspn_cont_bench_line.json'), 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
