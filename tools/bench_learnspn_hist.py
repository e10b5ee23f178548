"""LearnSPN with the histogram column splits on the HIP path against the numpy restatement of the same loop
(tests/learn_cont_ref.py with numpy's own ``np.histogram`` / ``np.histogram2d`` column splits) on the same host.

Workload: ``--rows`` x ``--cols`` float32 rows of tools/bench_learnspn_cont.py (two clusters, blocks of 4 columns that
share one latent), k-means row splits, min_rows_slice = 512, MLE Gaussian leaves, once with ``split_cols=gvs_cols`` (the
G-test on 'fd' bins) and once with ``split_cols=entropy_cols`` (``e`` between the entropies of the workload's columns).
``learn_spn`` end to end (upload, kernels, torch.sort, the host statistics, the FlatSpn) is the median of ``--runs`` runs
after one warm-up; the restatement runs once per split.
Writes profiles/learnspn_hist_bench_line.json and prints it.

    python tools/bench_learnspn_hist.py [--rows 20000] [--cols 16] [--runs 5] [--no-restatement]
"""
import argparse
import json
import os
import statistics
import sys
import time
from collections import deque

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, 'deeprob-kit_amd'), ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from bench_learnspn_cont import workload, SEED, MIN_ROWS  # noqa: E402

P, E, ALPHA = 5.0, 0.84, 0.1
EPS32 = np.finfo(np.float32).eps


def numpy_g(x1, x2):
    """gvs.py:185-197 in float64."""
    b1, b2 = np.histogram_bin_edges(x1, bins='fd'), np.histogram_bin_edges(x2, bins='fd')
    hist, _, _ = np.histogram2d(x1, x2, bins=[b1, b2])
    hist = hist + float(EPS32)
    m1, m2 = np.sum(hist, axis=1, keepdims=True), np.sum(hist, axis=0, keepdims=True)
    return 2.0 * np.sum(hist * np.log(hist / (m1 * m2 / len(x1)))), (len(b1) - 2) * (len(b2) - 2)


def numpy_gvs(x, rs):
    """gvs.py:29-50: the G-tests are made lazily, as the reference makes them."""
    nf = x.shape[1]
    start = rs.randint(0, nf)
    rest, seen, queue = set(range(nf)) - {start}, {start}, deque([start])
    while queue:
        f = queue.popleft()
        found = set()
        for o in rest:
            g, dof = numpy_g(x[:, f], x[:, o])
            if not g < 2.0 * dof * P:
                found.add(o)
                seen.add(o)
                queue.append(o)
        rest -= found
    part = np.zeros(nf, np.int64)
    part[list(seen)] = 1
    return part


def numpy_entropy(x, rs):
    """entropy.py:38-47."""
    part = np.zeros(x.shape[1], np.int64)
    for i in range(x.shape[1]):
        hist, _ = np.histogram(x[:, i], bins='scott')
        probs = (hist + ALPHA) / (len(x) + len(hist) * ALPHA)
        with np.errstate(divide='ignore', invalid='ignore'):
            if -np.sum(probs * np.log2(probs)) / np.log2(len(hist)) < E:
                part[i] = 1
    return part


def run_hip(x, name):
    import torch
    from deeprob.spn.learning import learn_spn, learnspn, splitting
    from deeprob.spn.structure.leaf import Gaussian
    cols = x.shape[1]
    domains = [(float(x[:, i].min()), float(x[:, i].max())) for i in range(cols)]
    kw = {'p': P} if name == 'gvs_cols' else {'e': E, 'alpha': ALPHA}
    t0 = time.perf_counter()
    flat = learn_spn(x, [Gaussian] * cols, domains, split_rows='kmeans', split_cols=getattr(splitting, name), split_cols_kwargs=kw,
                     min_rows_slice=MIN_ROWS, random_state=SEED, verbose=False)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, flat, learnspn.last_info()


def run_restatement(x, name):
    from tests import learn_cont_ref as ref
    split = numpy_gvs if name == 'gvs_cols' else numpy_entropy
    keep = ref.rdc_cols
    ref.rdc_cols = lambda data, rs, d, k, s, stats: split(np.asarray(data, np.float32), rs)     # (the loop's column split)
    try:
        t0 = time.perf_counter()
        root = ref.learn_spn(x, split_cols='rdc', min_rows_slice=MIN_ROWS, random_state=SEED)
        return time.perf_counter() - t0, root
    finally:
        ref.rdc_cols = keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=20000)
    ap.add_argument('--cols', type=int, default=16)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--no-restatement', action='store_true')
    args = ap.parse_args()
    x = workload(args.rows, args.cols)
    line = {'bench': 'learnspn_hist', 'rows': args.rows, 'cols': args.cols, 'split_rows': 'kmeans', 'min_rows_slice': MIN_ROWS,
            'p': P, 'e': E}
    for name in ('gvs_cols', 'entropy_cols'):
        run_hip(x, name)                  # warm-up: library load, allocator, first launches
        times = []
        for _ in range(args.runs):
            t, flat, info = run_hip(x, name)
            times.append(t)
        rec = {'hip_seconds_median': round(statistics.median(times), 4), 'hip_seconds_all': [round(t, 4) for t in times],
               'nodes': flat.n_nodes, 'generations': info['generations'], 'kernels': info['kernels'], 'reads': info['reads'],
               'uploads': info['uploads'], 'max_tasks_in_a_generation': max(info['tasks_per_generation'])}
        if not args.no_restatement:
            from tests.test_learn_cont_gpu import circuits_differ
            seconds, want = run_restatement(x, name)
            rec['restatement_seconds'] = round(seconds, 3)
            rec['speedup_over_restatement'] = round(seconds / rec['hip_seconds_median'], 2)
            rec['same_graph_as_restatement'] = circuits_differ(flat, want) is None
        line[name] = rec
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'learnspn_hist_bench_line.json'), 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
