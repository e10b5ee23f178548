"""The posterior queries of BinaryCLTMixture (``marginals``, ``sample``, ``mpe``: one ``dpc_mixq_*`` launch per piece of the
batch) on the HIP path, beside the same marginals assembled from what the package had before them.

Workload: the 60 000 x 784 binary rows of tools/bench_clt.py with 30 % of the entries set to NaN from a seed, resident on
the device; the K random trees with random CPTs of tools/bench_clt_mixture.py, K = 2 and 8.  Timed per K, each as the median
of ``--runs`` windows of ``--inner`` consecutive calls after a warm-up window, with a host clock around work that ends in a
device synchronise:

    marginals        BinaryCLTMixture.marginals of all rows;
    sample           BinaryCLTMixture.sample(seed) of all rows;
    mpe              BinaryCLTMixture.mpe of all rows;
    assembled        the answer of ``marginals`` put together from K calls of BinaryCLT.marginals and one of
                     BinaryCLTMixture.responsibilities, mixed in torch in float64;
    log_likelihood   BinaryCLTMixture.log_likelihood of the same rows, for scale.

``checks`` holds the largest difference between ``marginals`` and ``assembled``.  Writes one JSON line to ``--out`` (default
profiles/clt_mixture_queries_bench_line.json) and prints it.

    python tools/bench_clt_mixture_queries.py [--rows 60000] [--cols 784] [--nan 0.3]
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, 'deeprob-kit_amd'), ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from bench_clt import workload  # noqa: E402
from bench_clt_mixture import random_mixture  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=60000)
    ap.add_argument('--cols', type=int, default=784)
    ap.add_argument('--nan', type=float, default=0.3)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--inner', type=int, default=5, help='consecutive calls per timed window')
    ap.add_argument('--components', type=int, nargs='+', default=[2, 8])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clt_mixture_queries_bench_line.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_clt_mixture_queries.py measures on a HIP device; none found')
    x, _ = workload(args.rows, args.cols)
    x = x.copy()
    x[np.random.RandomState(3).rand(*x.shape) < args.nan] = np.nan
    xd = torch.from_numpy(x).cuda()
    holes = torch.isnan(xd)
    line = {'bench': 'clt_mixture_queries', 'rows': args.rows, 'cols': args.cols, 'nan': args.nan, 'runs': args.runs,
            'inner': args.inner,
            'method': 'host clock around calls that end in a device synchronise; a window is `inner` consecutive calls on rows '
                      'resident on the device; median of the windows after a warm-up window',
            'components': {}}
    for k in args.components:
        m = random_mixture(args.cols, k, k)

        def assembled():
            resp = m.responsibilities(xd).double()
            acc = torch.zeros(xd.shape, dtype=torch.float64, device=xd.device)
            for j, c in enumerate(m.components):
                acc += resp[:, j:j + 1] * c.marginals(xd).double()
            return torch.where(holes, acc.float(), xd)

        bodies = {'marginals': lambda: m.marginals(xd), 'sample': lambda: m.sample(xd, seed=7), 'mpe': lambda: m.mpe(xd),
                  'assembled': assembled, 'log_likelihood': lambda: m.log_likelihood(xd)}

        def window(body):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.inner):
                body()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.inner

        out = {'hip_seconds': {}, 'hip_seconds_all': {}}
        for name, body in bodies.items():
            window(body)                            # warm-up
            t = [window(body) for _ in range(args.runs)]
            out['hip_seconds'][name] = round(statistics.median(t), 6)
            out['hip_seconds_all'][name] = [round(v, 6) for v in t]
        direct, pieces = m.marginals(xd), assembled()
        filled, best = m.sample(xd, seed=7), m.mpe(xd)
        out['checks'] = {'marginals_vs_assembled_max_abs_diff': float((direct - pieces)[holes].abs().max()),
                         'observed_entries_bit_equal': bool(all(torch.equal(t[~holes], xd[~holes]) for t in (direct, filled, best))),
                         'fills_are_binary': bool(((filled == 0) | (filled == 1)).all() and ((best == 0) | (best == 1)).all())}
        out['assembled_over_marginals'] = round(out['hip_seconds']['assembled'] / out['hip_seconds']['marginals'], 2)
        line['components'][str(k)] = out
    text = json.dumps(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
