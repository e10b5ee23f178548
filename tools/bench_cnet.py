"""BinaryCNet on the HIP path against the numpy restatement (tests/cnet_ref.py) on the same host.

Workload: 20 000 x 200 binary rows of a 6-prototype mixture with 20 % flips, generated here from a seed; ``fit`` with
``alpha = 0.01``, ``min_n_samples = 500``.  Timed, each as the median of ``--runs`` calls after one warm-up, with a host
clock around work that ends in a device synchronise:

    fit            numpy rows in: upload, the generations on the device (gather-pack, counts, scores, partition, the
                   records read back) and the leaves' host learning (mutual information, Prim, CPTs); the split comes
                   from ``BinaryCNet.fit_profile_`` of the same runs;
    ll_complete    log_likelihood of the training rows, resident on the device;
    ll_nan         log_likelihood of the same rows with 30 % of the entries NaN;
    sample_nan     BinaryCNet.sample of those rows with NaN: one exact posterior draw per row, one launch;
    mpe_nan        deeprob.hip.cnet.mpe of those rows (the tables uploaded per call, as the class's queries do);
    marginals_nan  BinaryCNet.marginals of those rows: the posterior marginal of every NaN entry, one launch.

The restatement runs once: ``fit`` on all rows, the queries on the first ``--ref-rows`` rows; ``speedup`` compares seconds
per row.  The device results are checked against it: the OR tree, and the likelihoods of the device model evaluated by
the restatement's query code.  Writes one JSON line to ``--out`` (default profiles/cnet_bench_line.json) and prints it.
The three filling queries go beside ``ll_nan`` -- the same rows, the same NaN share, the same walk plus one leaf pass -- into
a line of their own, ``--queries-out`` (default profiles/cnet_queries_bench_line.json), with their time as a multiple of
``ll_nan``'s and what was checked of their outputs (observed entries kept, every NaN filled with 0 / 1, the MPE no less
likely than the sample row by row, the marginals within [0, 1] and their distance from the float64 restatement,
tests/marginals_ref.py, on the first ``--marginals-ref-rows`` rows).

    python tools/bench_cnet.py [--rows 20000] [--cols 200] [--ref-rows 4096] [--no-restatement]
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

DATA_SEED, ROOT_SEED = 1, 7
HYPER = dict(alpha=0.01, min_n_samples=500, min_n_features=1, min_mean_entropy=0.01)


def workload(rows, cols, n_clusters=6, noise=0.2):
    rs = np.random.RandomState(DATA_SEED)
    protos = rs.rand(n_clusters, cols) < 0.5
    x = (protos[rs.randint(0, n_clusters, size=rows)] ^ (rs.rand(rows, cols) < noise)).astype(np.float32)
    x_nan = x.copy()
    x_nan[rs.rand(rows, cols) < 0.3] = np.nan
    return x, x_nan


def timed(fn, runs):
    import torch
    fn()                                    # warm-up: library load, allocator, first launches
    torch.cuda.synchronize()
    times, outs = [], []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs.append(fn())
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return outs, times


def fit_model(x):
    from deeprob.spn.structure.cnet import BinaryCNet
    return BinaryCNet(list(range(x.shape[1]))).fit(x, random_state=ROOT_SEED, **HYPER)


def as_ref_model(m):
    nodes = m._nodes()
    number = {id(n): k for k, n in enumerate(nodes)}
    return [dict(or_id=n.or_id, weights=list(n.weights), children=[number[id(c)] for c in n.children], scope=list(n.scope),
                 rows=())
            if n.clt is None else
            dict(or_id=-1, weights=None, children=None, scope=list(n.scope), rows=(), bfs=n.clt.bfs, tree=n.clt.tree,
                 params=n.clt.params) for n in nodes]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=20000)
    ap.add_argument('--cols', type=int, default=200)
    ap.add_argument('--ref-rows', type=int, default=4096)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cnet_bench_line.json'))
    ap.add_argument('--queries-out', default=os.path.join(ROOT, 'profiles', 'cnet_queries_bench_line.json'))
    ap.add_argument('--marginals-ref-rows', type=int, default=1024)
    ap.add_argument('--no-restatement', action='store_true')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_cnet.py measures on a HIP device; none found')
    x, x_nan = workload(args.rows, args.cols)
    xd, xd_nan = torch.from_numpy(x).cuda(), torch.from_numpy(x_nan).cuda()
    line = {'bench': 'cnet', 'rows': args.rows, 'cols': args.cols, 'nan_share': 0.3, 'runs': args.runs, 'hyper': HYPER,
            'method': 'host clock around calls that end in a device synchronise; median after one warm-up',
            'hip_seconds': {}, 'hip_seconds_all': {}}
    models, times = timed(lambda: fit_model(x), args.runs)
    model = models[-1]
    nodes = model._nodes()
    line['model'] = {'or_nodes': sum(n.clt is None for n in nodes), 'leaves': sum(n.clt is not None for n in nodes),
                     'generations': model.fit_profile_['generations'],
                     'largest_leaf': max(len(n.scope) for n in nodes if n.clt is not None)}
    line['fit_split_seconds'] = {k: round(statistics.median(m.fit_profile_[k] for m in models), 5)
                                 for k in ('generations_seconds', 'host_leaf_seconds')}
    todo, results = [('fit', times)], {}
    from deeprob.hip import cnet

    def mpe_nan():
        return cnet.mpe(model._on_device(xd_nan.device), xd_nan)
    for name, fn in (('ll_complete', lambda: model.log_likelihood(xd)), ('ll_nan', lambda: model.log_likelihood(xd_nan)),
                     ('sample_nan', lambda: model.sample(xd_nan, seed=DATA_SEED)), ('mpe_nan', mpe_nan),
                     ('marginals_nan', lambda: model.marginals(xd_nan))):
        outs, t = timed(fn, args.runs)
        results[name] = outs[-1]
        todo.append((name, t))
    queries = {'bench': 'cnet_queries', 'rows': args.rows, 'cols': args.cols, 'nan_share': 0.3, 'runs': args.runs,
               'hyper': HYPER, 'model': line['model'], 'method': line['method'], 'hip_seconds': {}, 'hip_seconds_all': {}}
    for name, t in todo:
        into = queries if name in ('sample_nan', 'mpe_nan', 'marginals_nan') else line
        into['hip_seconds'][name] = round(statistics.median(t), 5)
        into['hip_seconds_all'][name] = [round(v, 5) for v in t]
    queries['hip_seconds']['ll_nan'] = line['hip_seconds']['ll_nan']
    queries['multiple_of_ll_nan'] = {k: round(queries['hip_seconds'][k] / queries['hip_seconds']['ll_nan'], 2)
                                     for k in ('sample_nan', 'mpe_nan', 'marginals_nan')}
    observed = ~torch.isnan(xd_nan)
    drawn, best, soft = results.pop('sample_nan'), results.pop('mpe_nan'), results.pop('marginals_nan')
    queries['checks'] = {
        'observed_entries_kept': bool(torch.equal(drawn[observed], xd_nan[observed]) and torch.equal(best[observed], xd_nan[observed])),
        'every_nan_filled_with_0_or_1': bool(((drawn == 0) | (drawn == 1)).all() and ((best == 0) | (best == 1)).all()),
        'mpe_no_less_likely_than_the_sample': bool((model.log_likelihood(best) >= model.log_likelihood(drawn) - 1e-4).all()),
        'marginals_keep_observed_entries_and_lie_in_0_1': bool(torch.equal(soft[observed], xd_nan[observed])
                                                               and ((soft >= 0) & (soft <= 1)).all())}
    if not args.no_restatement:
        from tests import cnet_ref as ref
        n = min(args.ref_rows, args.rows)
        t0 = time.perf_counter()
        restated = ref.learn(x, random_state=np.random.RandomState(ROOT_SEED), **HYPER)
        seconds = {'fit': time.perf_counter() - t0}
        device_model = as_ref_model(model)
        want = {}
        for name, rows in (('ll_complete', x[:n]), ('ll_nan', x_nan[:n])):
            t0 = time.perf_counter()
            want[name] = ref.log_likelihood(device_model, rows)
            seconds[name] = time.perf_counter() - t0
        line['restatement_rows'] = {'fit': args.rows, 'queries': n}
        line['restatement_seconds'] = {k: round(v, 3) for k, v in seconds.items()}
        line['speedup_per_row'] = {
            k: round(seconds[k] / (args.rows if k == 'fit' else n) / (line['hip_seconds'][k] / args.rows), 1) for k in seconds}

        def rel(got, ref_values):
            got = got.cpu().numpy().reshape(-1)[:n].astype(np.float64)
            return float(np.max(np.abs(got - ref_values) / np.maximum(1.0, np.abs(ref_values))))
        from tests import marginals_ref as mref
        k = min(args.marginals_ref_rows, args.rows)
        queries['checks']['marginals_max_abs_err'] = float(np.max(np.abs(
            soft[:k].cpu().numpy() - mref.cnet_marginals(device_model, x_nan[:k], np.float64))))
        queries['checks']['marginals_rows_checked'] = k
        a, b = ref.structure(restated), ref.structure(device_model)
        line['checks'] = {
            'same_or_tree': bool(np.array_equal(a[0], b[0]) and a[2] == b[2]),
            'or_weights_max_abs_diff': float(np.nanmax(np.abs(a[1] - b[1]))) if np.array_equal(a[0], b[0]) else None,
            'leaves_with_the_same_edge_set': int(sum(p == q for p, q in zip(a[3], b[3]) if p is not None)),
            'll_complete_rel_err': rel(results['ll_complete'], want['ll_complete'].astype(np.float64)),
            'll_nan_rel_err': rel(results['ll_nan'], want['ll_nan'].astype(np.float64))}
    text = json.dumps(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)
    text = json.dumps(queries)
    os.makedirs(os.path.dirname(os.path.abspath(args.queries_out)), exist_ok=True)
    with open(args.queries_out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
