"""The XPC learners on the HIP path against the numpy restatement (tests/xpc_ref.py) on the same host.

Workload: 20 000 x 200 binary rows of a 6-prototype mixture with 20 % flips, generated here from a seed.  Three learners,
all with ``det = False``, ``min_part_inst = 200``, ``conj_len = 3``, ``arity = 4``, ``n_max_parts = 200``:

    xpc        learn_xpc(sd=False): Chow-Liu leaves that learn their own trees;
    xpc_sd     learn_xpc(sd=True): one dependency tree from the cumulative mutual information;
    expc       learn_expc(ensemble_dim=10, sd_level=1) under np.random.seed(11).

Each is timed as the median of ``--runs`` calls after one warm-up, numpy rows in, with a host clock around work that ends
in a device synchronise; the split of a call comes from ``deeprob.spn.learning.xpc.last_profile()`` of the same runs
(every lap ends in a synchronise): ``pack`` (upload, bit planes), ``partition`` (the partition trees: draws, one histogram
and one stable split per horizontal split, the read of the row ids), ``leaf_counts`` (one gather-pack, the co-occurrence
counts of all leaf partitions and their read-back) and ``host`` (mutual information, spanning trees, CPTs, leaves and the
flat circuit).

The restatement runs once per learner on the same rows and is timed in the two steps it has: ``partition`` and ``leaves``
(its counts are numpy products inside the leaf learning: they cannot be told apart from its host arithmetic).  The device
results are checked against it: the number of partitions, the conjunctions, and the log likelihood of the first
``--ref-rows`` rows.  Writes one JSON line to ``--out`` (default profiles/xpc_bench_line.json) and prints it.

    python tools/bench_xpc.py [--rows 20000] [--cols 200] [--members 10] [--no-restatement]
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

DATA_SEED, GLOBAL_SEED = 1, 11
HYPER = dict(det=False, min_part_inst=200, conj_len=3, arity=4, n_max_parts=200)
STEPS = ('pack', 'partition', 'leaf_counts', 'host')


def workload(rows, cols, n_clusters=6, noise=0.2):
    rs = np.random.RandomState(DATA_SEED)
    protos = rs.rand(n_clusters, cols) < 0.5
    return (protos[rs.randint(0, n_clusters, size=rows)] ^ (rs.rand(rows, cols) < noise)).astype(np.float32)


def timed(fn, runs):
    import torch
    from deeprob.spn.learning import xpc
    fn()                                    # warm-up: library load, allocator, first launches
    torch.cuda.synchronize()
    times, splits, out = [], [], None
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        splits.append(xpc.last_profile())
    return out, times, splits


def restated(kind, x, members):
    """``(model, seconds per step)`` of the restatement, its learners taken apart at their two steps."""
    from tests import xpc_ref as ref
    d = x.shape[1]
    rs, leaf_rs = np.random.RandomState(42), np.random.RandomState(42)
    sd = kind != 'xpc'
    ordering = np.arange(d).tolist()
    t0 = time.perf_counter()
    models = []
    if kind == 'expc':
        np.random.seed(GLOBAL_SEED)
    for _ in range(members if kind == 'expc' else 1):
        if kind == 'expc':
            np.random.shuffle(ordering)
        else:
            rs.shuffle(ordering)
        root, cl_parts, conj_l, n_parts = ref.partitioning(x, HYPER['min_part_inst'], HYPER['n_max_parts'], HYPER['conj_len'],
                                                           HYPER['arity'], sd, list(ordering), rs)
        models.append(dict(root=root, cl_parts=cl_parts, conj_vars_l=conj_l, n_parts=n_parts, trees_dict=None))
    t1 = time.perf_counter()
    for m in models:
        if sd:
            m['trees_dict'] = ref.trees_dict(x, [m['cl_parts']], m['conj_vars_l'], 0.01, rs)
        ref._build(x, m['root'], True, m['trees_dict'], False, 0.01, leaf_rs)
    t2 = time.perf_counter()
    return dict(members=models), {'partition': t1 - t0, 'leaves': t2 - t1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=20000)
    ap.add_argument('--cols', type=int, default=200)
    ap.add_argument('--members', type=int, default=10)
    ap.add_argument('--ref-rows', type=int, default=1024)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'xpc_bench_line.json'))
    ap.add_argument('--no-restatement', action='store_true')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_xpc.py measures on a HIP device; none found')
    from deeprob.spn.algorithms.inference import log_likelihood
    from deeprob.spn.learning import learn_expc, learn_xpc
    x = workload(args.rows, args.cols)

    def ensemble():
        np.random.seed(GLOBAL_SEED)
        return learn_expc(x, ensemble_dim=args.members, sd_level=1, **HYPER)
    learners = {'xpc': lambda: learn_xpc(x, sd=False, **HYPER), 'xpc_sd': lambda: learn_xpc(x, sd=True, **HYPER),
                'expc': ensemble}
    line = {'bench': 'xpc', 'rows': args.rows, 'cols': args.cols, 'members': args.members, 'runs': args.runs, 'hyper': HYPER,
            'method': 'host clock around calls that end in a device synchronise; median after one warm-up; the split is '
                      'last_profile() of the same calls, every lap closed by a synchronise',
            'hip_seconds': {}, 'hip_seconds_all': {}, 'hip_split_seconds': {}, 'model': {}}
    if not args.no_restatement:
        line.update(restatement_seconds={}, speedup={}, checks={})
    for name, fn in learners.items():
        (circuit, utils), times, splits = timed(fn, args.runs)
        utils = utils if isinstance(utils, list) else [utils]
        line['hip_seconds'][name] = round(statistics.median(times), 5)
        line['hip_seconds_all'][name] = [round(t, 5) for t in times]
        line['hip_split_seconds'][name] = {k: round(statistics.median(s.get(k, 0.0) for s in splits), 5) for k in STEPS}
        line['model'][name] = {'nodes': int(circuit.n_nodes), 'n_parts': [int(u['n_parts']) for u in utils],
                               'leaf_partitions': int(sum(len(u['cl_parts_l']) for u in utils)),
                               'leaf_rows': int(sum(p.n_rows for u in utils for p in u['cl_parts_l']))}
        if args.no_restatement:
            continue
        model, seconds = restated(name, x, args.members)
        line['restatement_seconds'][name] = {k: round(v, 3) for k, v in seconds.items()}
        split = line['hip_split_seconds'][name]
        line['speedup'][name] = {
            'partition': round(seconds['partition'] / max(split['partition'], 1e-9), 1),
            'leaves': round(seconds['leaves'] / max(split['leaf_counts'] + split['host'], 1e-9), 1),
            'whole': round(sum(seconds.values()) / line['hip_seconds'][name], 1)}
        n = min(args.ref_rows, args.rows)
        from tests import xpc_ref as ref
        got = log_likelihood(circuit, x[:n]).astype(np.float64).reshape(-1)
        want = ref.log_likelihood(model, x[:n])
        line['checks'][name] = {
            'same_n_parts': [int(u['n_parts']) for u in utils] == [m['n_parts'] for m in model['members']],
            'same_conjunctions': all([[int(v) for v in c] for c in u['conj_vars_l']] == m['conj_vars_l']
                                     for u, m in zip(utils, model['members'])),
            'll_rows': n,
            # (a leaf with several maximum spanning trees may take another of them than the restatement's Prim)
            'll_rel_err': float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))),
            'mean_ll_device': float(got.mean()), 'mean_ll_restatement': float(want.mean())}
    text = json.dumps(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
