"""BinaryCLTMixture on the HIP path against the numpy restatement (tests/clt_mixture_ref.py) on the same host.

Workload: 60 000 x 784 binary rows of a 4-prototype mixture with 20 % noise, generated here from a seed (the rows of
tools/bench_clt.py); K random trees with random CPTs, K = 2 and 8.  Timed per K, each as the median of ``--runs`` windows of many calls
after a warm-up window, with a host clock around work that ends in a device synchronise or a host read:

    em_iteration     one iteration of batch EM on a resident batch of 10 % of the rows (6 000): dpc_mix_log_likelihood and
                     dpc_mix_em_stats over the batch index, the read of the K (1 + 2 D) doubles, the float32 updates on the
                     host and the ONE upload of the new tables -- the body of BinaryCLTMixture.em's loop; a timed window
                     is ``--inner`` (100) consecutive iterations, each from the tables the one before left, and the
                     figure is the window over ``--inner``;
    em_device        the two launches of an iteration alone, ``--inner`` times per window;
    ll_complete      log_likelihood of the 60 000 rows, resident on the device, ``--inner`` / 5 calls per window.

The restatement runs once per K, float64 vectorised numpy: one EM iteration on the same batch, the log likelihood of the
first ``--ref-rows`` rows; ``speedup`` compares seconds per row.  The device results are checked against it.  Writes one JSON
line to ``--out`` (default profiles/clt_mixture_bench_line.json) and prints it.

    python tools/bench_clt_mixture.py [--rows 60000] [--cols 784] [--ref-rows 4096] [--no-restatement]
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

from bench_clt import workload  # noqa: E402

STEP = 0.5


def random_mixture(d, k, seed):
    from deeprob.spn.structure import BinaryCLTMixture
    from deeprob.spn.structure.cltree import BinaryCLT
    rs = np.random.RandomState(seed)
    scope, trees = list(range(d)), []
    for _ in range(k):
        order = rs.permutation(d)
        tree = np.full(d, -1, np.int32)
        for i in range(1, d):
            tree[order[i]] = order[rs.randint(0, i)]
        clt = BinaryCLT(scope, tree=tree, params=np.zeros((d, 2, 2), np.float32))
        clt.em_init(rs)
        trees.append(clt)
    return BinaryCLTMixture(scope, trees, rs.dirichlet(np.ones(k)).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=60000)
    ap.add_argument('--cols', type=int, default=784)
    ap.add_argument('--ref-rows', type=int, default=4096)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--inner', type=int, default=100, help='consecutive EM iterations per timed window')
    ap.add_argument('--components', type=int, nargs='+', default=[2, 8])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clt_mixture_bench_line.json'))
    ap.add_argument('--no-restatement', action='store_true')
    args = ap.parse_args()
    import torch
    from deeprob.hip import clt
    from deeprob.spn.structure.cltree import em_update
    if not torch.cuda.is_available():
        raise SystemExit('bench_clt_mixture.py measures on a HIP device; none found')
    x, _ = workload(args.rows, args.cols)
    xd = torch.from_numpy(x).cuda()
    codes = clt.pack_query(xd)
    batch = np.random.RandomState(2).choice(args.rows, args.rows // 10, replace=False).astype(np.int32)
    index = torch.from_numpy(batch).cuda()
    line = {'bench': 'clt_mixture', 'rows': args.rows, 'cols': args.cols, 'batch': len(batch), 'runs': args.runs, 'inner': args.inner,
            'method': 'host clock around calls that end in a device synchronise or a host read; a window is many consecutive calls; median of the windows after a warm-up window',
            'components': {}}
    for k in args.components:
        m = random_mixture(args.cols, k, k)
        start_w, start_p = m.weights.copy(), np.stack([c.params for c in m.components])
        mix = m._on_device(xd.device)

        def device_part():
            ll, _, resp = clt.mixture_codes_log_likelihood(mix, codes, index, complete=True)
            return ll, clt.mixture_em_stats(mix, codes, index, resp)

        def iteration(w, p):
            """The body of BinaryCLTMixture.em's loop from the weights ``w`` and tables ``p`` that the device holds."""
            _, stats = device_part()
            stats = stats.cpu().numpy()
            share = stats[:, 0].astype(np.float32) + np.finfo(np.float32).eps
            share /= share.sum()
            w = (np.float32(1.0 - STEP) * w + np.float32(STEP) * share).astype(np.float32)
            p = np.stack([em_update(p[j], c.tree, c.root, stats[j], STEP) for j, c in enumerate(m.components)])
            mix.update(p, np.log(w))
            return w, p

        def window(body, calls):
            """Seconds per call of ``calls`` consecutive ``body(state) -> state`` from the same start (the tables are put
            back outside the clock)."""
            mix.update(start_p, np.log(start_w))
            state = (start_w, start_p)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                state = body(state)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / calls

        bodies = {'em_iteration': (lambda st: iteration(*st), args.inner),
                  'em_device': (lambda st: device_part() and st, args.inner),
                  'll_complete': (lambda st: m.log_likelihood(xd) is None or st, max(1, args.inner // 5))}
        out = {}
        w, p = iteration(start_w, start_p)          # the iteration that is checked below
        mix.update(start_p, np.log(start_w))
        ll = m.log_likelihood(xd)
        times = {}
        for name, (body, calls) in bodies.items():
            window(body, calls)                     # warm-up
            times[name] = [window(body, calls) for _ in range(args.runs)]
        t_it, t_dev, t_ll = times['em_iteration'], times['em_device'], times['ll_complete']
        for name, t in (('em_iteration', t_it), ('em_device', t_dev), ('ll_complete', t_ll)):
            out.setdefault('hip_seconds', {})[name] = round(statistics.median(t), 6)
            out.setdefault('hip_seconds_all', {})[name] = [round(v, 6) for v in t]
        if not args.no_restatement:
            from tests import clt_mixture_ref as mref
            from tests import clt_ref
            n = min(args.ref_rows, args.rows)
            trees = [(clt_ref.bfs_order(c.tree), c.tree) for c in m.components]
            roots = [c.root for c in m.components]
            t0 = time.perf_counter()
            w64, p64, _ = mref.em_run(trees, roots, start_p, start_w, x, batch[None, :], STEP)
            seconds = {'em_iteration': time.perf_counter() - t0}
            t0 = time.perf_counter()
            with np.errstate(divide='ignore'):
                want_ll = mref.mix(mref.complete_lls(trees, start_p, x[:n]), np.log(start_w.astype(np.float64)))[0]
            seconds['ll_complete'] = time.perf_counter() - t0
            got_ll = ll.cpu().numpy().reshape(-1)[:n].astype(np.float64)
            out['restatement_rows'] = {'em_iteration': len(batch), 'll_complete': n}
            out['restatement_seconds'] = {key: round(v, 3) for key, v in seconds.items()}
            out['speedup_per_row'] = {
                'em_iteration': round(seconds['em_iteration'] / out['hip_seconds']['em_iteration'], 1),
                'll_complete': round(seconds['ll_complete'] / n / (out['hip_seconds']['ll_complete'] / args.rows), 1)}
            errs = mref.prob_err(w, p, w64, p64)
            out['checks'] = {'weights_max_abs_diff': errs[0], 'cpt_max_abs_diff': errs[1],
                             'll_complete_rel_err': float(np.max(np.abs(got_ll - want_ll) / np.maximum(1.0, np.abs(want_ll))))}
        line['components'][str(k)] = out
    text = json.dumps(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
