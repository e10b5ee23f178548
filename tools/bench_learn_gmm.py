"""The Gaussian-mixture row split on the HIP path (deeprob.spn.learning.splitting.gmm) against the numpy restatement
(tests/learn_gmm_ref.py) on the same host and, where scikit-learn is importable, ``GaussianMixture.fit_predict``.

Shapes: 100 000 x 64 binary rows (a two-prototype mixture with 20 % noise) and 20 000 x 32 Gaussian rows (two clusters that
differ in location and scale), ``n = 2``.  Per EM iteration over the three initialisations of the one task, after the Lloyd
initialisation: the E-step (``dpl_gmm_estep``, both launches, tables and parameters uploaded) and the moments pass
(``dpl_gmm_mstats``, on the VALU and on the matrix core) by device events, and the host M-step (Cholesky factors and
inversions) by the wall clock; medians of ``--runs`` after one warm-up.  The whole ``gmm()`` call (upload, Lloyd steps, EM,
label read) is the median of ``--runs`` calls after one warm-up; the restatement and scikit-learn run once.
Writes profiles/learn_gmm_bench_line.json and prints it.

    python tools/bench_learn_gmm.py [--runs 5] [--no-restatement] [--out profiles/learn_gmm_bench_line.json]
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

SEED = 7


def workloads():
    from deeprob.spn.structure.leaf import Bernoulli, Gaussian
    rs = np.random.RandomState(1)
    protos = rs.randint(0, 2, size=(2, 64))
    z = rs.randint(0, 2, size=100000)
    flip = rs.rand(100000, 64) < 0.2
    binary = np.where(flip, rs.randint(0, 2, size=(100000, 64)), protos[z]).astype(np.uint8)
    z = rs.rand(20000) < 0.4
    scale_a, scale_b = 0.5 + rs.rand(32), 0.5 + rs.rand(32)
    gauss = np.where(z[:, None], rs.randn(20000, 32) * scale_a, rs.randn(20000, 32) * scale_b + 1.5).astype(np.float32)
    return {'binary_100000x64': (binary, [Bernoulli] * 64, [[0, 1]] * 64, [2] * 64),
            'gaussian_20000x32': (gauss, [Gaussian] * 32, [(-100.0, 100.0)] * 32, None)}


def events(fn, runs):
    """Median milliseconds of ``fn()`` by device events, after one warm-up."""
    import torch
    times = []
    for i in range(runs + 1):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        if i:
            times.append(start.elapsed_time(stop))
    return round(statistics.median(times), 3)


def per_iteration(data, dists, doms, runs):
    import torch
    from deeprob.hip import learn as L
    from deeprob.spn.learning.splitting import cluster
    kind, dev, row_index, rs = cluster._setup(data, dists, doms, np.random.RandomState(SEED), 2, 'gmm')
    batch = kind.gmm_batch(row_index, [cluster._task(dev, rs, 2, L.GMM_N_INIT)], 2)
    km = L.KMeansBatch(batch.data, row_index, batch.tasks, batch.R, 2, batch.kmax)
    labels = km.run()[2]
    batch.resp.zero_()
    batch.resp.scatter_(2, labels.long().unsqueeze(-1), 1.0)
    pivot = batch.pivots(L.read(km.cent), km)
    pairs = sorted(pivot)
    F, n = batch.fs[0], batch.ns[0]
    par = {a: np.concatenate([np.zeros((2, 1)), pivot[a], np.zeros((2, F * F))], axis=1) for a in pairs}
    out, stat_off, _ = batch.launch([], pairs, par)
    host = L.read(out)

    def m_steps():
        return {a: L.gmm_m_step(host[stat_off[k]:stat_off[k] + 2 * batch.per(0)].reshape(2, -1), par[a][:, 1:1 + F], n)
                for k, a in enumerate(pairs)}
    host_ms = []
    for i in range(runs + 1):
        t0 = time.perf_counter()
        new = m_steps()
        if i:
            host_ms.append(1e3 * (time.perf_counter() - t0))
    par = new
    line = {'features': F, 'estep_ms': events(lambda: batch.launch(pairs, [], par), runs),
            'mstats_ms': {name: events(lambda: batch.launch([], pairs, par, mfma=flag), runs)
                          for name, flag in (('valu', False), ('mfma', True))},
            'host_m_step_ms': round(statistics.median(host_ms), 3)}
    flops = 3 * 2 * (2.0 * n * F * (F + 1) / 2.0)             # inits x components x the products of the lower triangle
    line['mstats_f64_gflops'] = {name: round(flops / (ms * 1e-3) / 1e9, 1) for name, ms in line['mstats_ms'].items()}
    torch.cuda.synchronize()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--no-restatement', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'learn_gmm_bench_line.json'))
    args = ap.parse_args()
    import torch
    from deeprob.hip import learn as L
    from deeprob.spn.learning.splitting import gmm
    line = {'bench': 'learn_gmm', 'n': 2, 'n_init': L.GMM_N_INIT, 'mstats_products_in_use': 'mfma' if L.GMM_USE_MFMA else 'valu',
            'shapes': {}}
    for name, (data, dists, doms, ks) in workloads().items():
        rec = per_iteration(data, dists, doms, args.runs)
        times = []
        for i in range(args.runs + 1):
            L.reset_counters()
            t0 = time.perf_counter()
            labels = gmm(data, dists, doms, np.random.RandomState(SEED), n=2)
            torch.cuda.synchronize()
            if i:
                times.append(time.perf_counter() - t0)
        rec.update(gmm_seconds_median=round(statistics.median(times), 4), gmm_seconds_all=[round(t, 4) for t in times],
                   em_passes=L.COUNTERS['gmm_reads'] - 3, sizes=np.bincount(labels).tolist())
        if not args.no_restatement:
            from tests import learn_gmm_ref as ref
            stats = {}
            t0 = time.perf_counter()
            want = ref.gmm(data, ks, np.random.RandomState(SEED), 2, stats)
            rec['restatement_seconds'] = round(time.perf_counter() - t0, 3)
            rec['restatement_iterations'] = stats['iterations']
            rec['speedup_over_restatement'] = round(rec['restatement_seconds'] / rec['gmm_seconds_median'], 2)
            rec['labels_agree_with_restatement'] = float(np.mean(labels == want))
            try:
                from sklearn.mixture import GaussianMixture
                t0 = time.perf_counter()
                sk = GaussianMixture(2, n_init=3, random_state=np.random.RandomState(SEED)).fit_predict(ref.features(data, ks))
                rec['sklearn_fit_predict_seconds'] = round(time.perf_counter() - t0, 3)
                agree = float(np.mean(sk == labels))
                rec['labels_agree_with_sklearn_up_to_order'] = max(agree, 1.0 - agree)
            except ImportError:
                pass
        line['shapes'][name] = rec
    text = json.dumps(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
