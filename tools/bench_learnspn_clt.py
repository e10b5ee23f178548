"""LearnSPN with Chow-Liu tree leaves (``learn_leaf=learn_binary_clt``) on the HIP path, against two baselines.

Workload: the data of tools/bench_learnspn.py -- 100 000 x 64 binary rows of the 4-prototype mixture with 20 % noise
(tests/learnspn_ref.py:mixture) --, gvs column splits, min_rows_slice = 512 and RANDOM row splits, as in the goldens: a
random split leaves the mixture mixed, so the G-test keeps the columns together and the rows are halved down to leaf tasks
of many columns (with k-means the clusters come out pure, every column splits off and no leaf is multivariate).  The leaf
seed is an integer, so the splits are those of the MLE run.  ``learn_spn`` end to end (upload, kernels, host orchestration, the FlatSpn) is the
median of 5 runs after one warm-up, for

  * ``learn_leaf=learn_binary_clt``;
  * ``learn_leaf='mle'``, the same call without the feature: the difference is what the leaves add (the counting launch, its
    read, and on the host Prim's tree, the CPTs and the expansion of every leaf);
  * a host numpy restatement of the CLT run: the restatement of tests/learnspn_ref.py for the structure (its leaves are MLE
    leaves, whose cost is negligible) plus, for every Chow-Liu leaf of the HIP run, the gather of its rows from the host
    matrix, ``rows.T @ rows`` in int64 and the same host half (``BinaryCLT.fit_counts``, ``to_pc_nodes``); the counts are
    checked against the device's.

Writes profiles/learnspn_clt_bench_line.json and prints it.

    python tools/bench_learnspn_clt.py [--rows 100000] [--cols 64] [--runs 5] [--no-restatement]
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

SEED, LEAF_SEED, DATA_SEED, MIN_ROWS, ALPHA = 42, 7, 1, 512, 0.1


def run_hip(x, clt):
    import torch
    from deeprob.spn.learning import learn_spn, learnspn
    from deeprob.spn.learning.leaf import learn_binary_clt
    from deeprob.spn.structure.leaf import Bernoulli
    cols = x.shape[1]
    leaf = dict(learn_leaf=learn_binary_clt, learn_leaf_kwargs={'alpha': ALPHA, 'random_state': LEAF_SEED}) if clt else \
        dict(learn_leaf='mle', learn_leaf_kwargs={'alpha': ALPHA})
    t0 = time.perf_counter()
    flat = learn_spn(x, [Bernoulli] * cols, [[0, 1]] * cols, split_rows='random', split_cols='gvs', min_rows_slice=MIN_ROWS,
                     random_state=SEED, verbose=False, **leaf)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, flat, learnspn.last_info()


def median_of(x, clt, runs):
    run_hip(x, clt)                     # warm-up: library load, allocator, first launches
    times = []
    for _ in range(runs):
        t, flat, info = run_hip(x, clt)
        times.append(t)
    return times, flat, info


def restate_leaves(x, leaves):
    """The host restatement of the leaves: numpy counts of every leaf's rows, then the same host half.  Returns the
    seconds and whether trees and parameters equal the device run's."""
    from deeprob.spn.structure.cltree import BinaryCLT
    same = True
    t0 = time.perf_counter()
    for rec, rows in leaves:
        sub = x[rows][:, rec['scope']].astype(np.int64)
        leaf = BinaryCLT(rec['scope'], root=rec['root'])
        leaf.fit_counts(sub.T @ sub, len(rows), alpha=ALPHA)
        leaf.to_pc_nodes()
        same = same and np.array_equal(leaf.tree, rec['tree']) and np.array_equal(leaf.params, rec['params'])
    return time.perf_counter() - t0, bool(same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=100000)
    ap.add_argument('--cols', type=int, default=64)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--no-restatement', action='store_true')
    ap.add_argument('--parent-line', help="a JSON file with the timing of the 'mle' call measured on a checkout of the parent "
                                          "commit (same workload, same machine): stored under 'parent_commit_mle'")
    args = ap.parse_args()
    from deeprob.spn.algorithms.inference import log_likelihood
    from tests import learnspn_ref as ref
    x, _ = ref.mixture([2] * args.cols, args.rows, DATA_SEED)
    mle_times, mle_flat, mle_info = median_of(x, False, args.runs)
    clt_times, clt_flat, clt_info = median_of(x, True, args.runs)
    sample = x[:20000].astype(np.float32)
    line = {'bench': 'learnspn_clt', 'rows': args.rows, 'cols': args.cols, 'split_rows': 'random', 'split_cols': 'gvs',
            'min_rows_slice': MIN_ROWS,
            'clt_seconds_median': round(statistics.median(clt_times), 4), 'clt_seconds_all': [round(t, 4) for t in clt_times],
            'mle_seconds_median': round(statistics.median(mle_times), 4), 'mle_seconds_all': [round(t, 4) for t in mle_times],
            'clt_leaves': len(clt_info['clt_leaves']),
            'widest_clt_leaf': max([len(r['scope']) for r in clt_info['clt_leaves']] or [0]),
            'nodes_clt': clt_flat.n_nodes, 'nodes_mle': mle_flat.n_nodes, 'generations': clt_info['generations'],
            'launches_clt': clt_info['launches'], 'launches_mle': mle_info['launches'],
            'mean_ll_clt_first_20000_rows': round(float(np.mean(np.asarray(log_likelihood(clt_flat, sample), np.float64))), 4),
            'mean_ll_mle_first_20000_rows': round(float(np.mean(np.asarray(log_likelihood(mle_flat, sample), np.float64))), 4)}
    line['added_seconds'] = round(line['clt_seconds_median'] - line['mle_seconds_median'], 4)
    if not args.no_restatement:
        leaves = [(rec, rec['rows'].cpu().numpy()) for rec in clt_info['clt_leaves']]
        t0 = time.perf_counter()
        ref.learn_spn(x, ['Bernoulli'] * args.cols, [2] * args.cols, split_rows='random', split_cols='gvs',
                      min_rows_slice=MIN_ROWS, random_state=SEED)
        structure = time.perf_counter() - t0
        leaf_seconds, same = restate_leaves(x, leaves)
        line['restatement_structure_seconds'] = round(structure, 3)
        line['restatement_leaves_seconds'] = round(leaf_seconds, 4)
        line['restatement_seconds'] = round(structure + leaf_seconds, 3)
        line['speedup_over_restatement'] = round(line['restatement_seconds'] / line['clt_seconds_median'], 2)
        line['same_leaves_as_restatement'] = same
    if args.parent_line:
        with open(args.parent_line) as f:
            line['parent_commit_mle'] = json.load(f)
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'learnspn_clt_bench_line.json'), 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
