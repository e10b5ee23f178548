"""LearnSPN on the HIP path against the numpy restatement (tests/learnspn_ref.py) on the same host.

Workload: 100 000 x 64 binary rows of the 4-prototype mixture with 20 % noise (tests/learnspn_ref.py:mixture), gvs column
splits, k-means row splits, min_rows_slice = 512.  ``learn_spn`` end to end (upload, kernels, host orchestration, the
FlatSpn) is the median of 5 runs after one warm-up; the restatement runs once.  The split of device time over the
kernels comes from one ``rocprofv3 --kernel-trace --stats`` run of this script with ``--profile-child`` (one learn_spn).
Writes profiles/learnspn_bench_line.json and prints it.

``--split-cols rdc`` runs the same workload with ``split_cols=rdc_cols`` (the exact maximal correlation) against
the restatement of tests/rdc_ref.py and writes profiles/learnspn_rdc_bench_line.json instead.

    python tools/bench_learnspn.py [--rows 100000] [--cols 64] [--split-cols gvs|rdc] [--no-profile] [--no-restatement]
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

SEED, DATA_SEED, MIN_ROWS = 42, 1, 512


def workload(rows, cols):
    from tests import learnspn_ref as ref
    x, _ = ref.mixture([2] * cols, rows, DATA_SEED)
    return x


def run_hip(x, split_cols='gvs'):
    import torch
    from deeprob.spn.learning import learn_spn, learnspn
    from deeprob.spn.learning.splitting.rdc import rdc_cols
    from deeprob.spn.structure.leaf import Bernoulli
    cols = x.shape[1]
    t0 = time.perf_counter()
    flat = learn_spn(x, [Bernoulli] * cols, [[0, 1]] * cols, split_rows='kmeans',
                     split_cols=rdc_cols if split_cols == 'rdc' else split_cols, min_rows_slice=MIN_ROWS,
                     random_state=SEED, verbose=False)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, flat, learnspn.last_info()


def kernel_split(rows, cols, split_cols='gvs'):
    """Device time per kernel of one learn_spn, from a rocprofv3 run of this script (a fresh child process)."""
    if shutil.which('rocprofv3') is None:
        return {'error': 'rocprofv3 not found'}
    out = tempfile.mkdtemp(prefix='learnspn_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', out, '-o', 't', '--output-format', 'csv', '--',
               sys.executable, os.path.abspath(__file__), '--profile-child', '--rows', str(rows), '--cols', str(cols),
               '--split-cols', split_cols]
        r = subprocess.run(cmd, cwd=out, capture_output=True, text=True, timeout=600)
        found = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
        if r.returncode != 0 or not found:
            return {'error': 'rocprofv3 run failed (rc {}): {}'.format(r.returncode, r.stderr[-300:])}
        split, total = {}, 0.0
        for row in csv.DictReader(open(found[0])):
            name, ns = row['Name'], float(row['TotalDurationNs'])
            key = next((k for k in ('column_counts', 'pair_g', 'pair_maxcorr', 'partition_rows', 'kmeans_init', 'kmeans_assign', 'kmeans_update',
                                    'kmeans_inertia') if k in name), 'other (torch copies and fills)')
            split[key] = split.get(key, 0.0) + ns / 1e6
            total += ns / 1e6
        return {'device_ms_total': round(total, 3), 'device_ms': {k: round(v, 3) for k, v in sorted(split.items())}}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=100000)
    ap.add_argument('--cols', type=int, default=64)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--split-cols', choices=('gvs', 'rdc'), default='gvs')
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--no-restatement', action='store_true')
    ap.add_argument('--profile-child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    x = workload(args.rows, args.cols)
    if args.profile_child:
        run_hip(x, args.split_cols)
        return
    from deeprob.spn.structure.io import spn_to_digraph
    from tests import learnspn_ref as ref
    run_hip(x, args.split_cols)                  # warm-up: library load, allocator, first launches
    times = []
    for _ in range(args.runs):
        t, flat, info = run_hip(x, args.split_cols)
        times.append(t)
    line = {'bench': 'learnspn', 'rows': args.rows, 'cols': args.cols, 'split_rows': 'kmeans', 'split_cols': args.split_cols,
            'min_rows_slice': MIN_ROWS, 'hip_seconds_median': round(statistics.median(times), 4),
            'hip_seconds_all': [round(t, 4) for t in times], 'nodes': flat.n_nodes,
            'generations': info['generations'], 'launches': info['launches'], 'lloyd_launches': info['lloyd_launches'],
            'max_tasks_in_a_generation': max(info['tasks_per_generation'])}
    if not args.no_restatement:
        t0 = time.perf_counter()
        if args.split_cols == 'rdc':
            from tests import rdc_ref
            want = rdc_ref.learn_spn(x, ['Bernoulli'] * args.cols, [2] * args.cols, split_rows='kmeans',
                                     min_rows_slice=MIN_ROWS, random_state=SEED)
        else:
            want = ref.learn_spn(x, ['Bernoulli'] * args.cols, [2] * args.cols, split_rows='kmeans', split_cols='gvs',
                                 min_rows_slice=MIN_ROWS, random_state=SEED)
        line['restatement_seconds'] = round(time.perf_counter() - t0, 3)
        line['speedup_over_restatement'] = round(line['restatement_seconds'] / line['hip_seconds_median'], 2)
        line['same_graph_as_restatement'] = ref.graphs_differ(spn_to_digraph(flat), ref.to_digraph(want)) is None
    if not args.no_profile:
        line['kernel_split'] = kernel_split(args.rows, args.cols, args.split_cols)
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    name = 'learnspn_rdc_bench_line.json' if args.split_cols == 'rdc' else 'learnspn_bench_line.json'
    with open(os.path.join(ROOT, 'profiles', name), 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
