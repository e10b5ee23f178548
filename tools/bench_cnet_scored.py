"""learn_cnet_bd / learn_cnet_bic on the HIP path against the numpy restatement (tests/cnet_scored_ref.py) on the same host.

Workload: the data family of tools/bench_cnet.py -- ``--rows`` x ``--cols`` binary rows of a 6-prototype mixture with 20 %
flips, generated here from a seed -- learned with ``ess = 0.1`` (BDeu) and ``alpha = 0.01`` (BIC), ``--cands`` candidate
cuts per node.  Timed per learner as the median of ``--runs`` calls after one warm-up, with a host clock around work that
ends in a device synchronise; the phases come from ``fit_profile_`` of the same runs:

    seconds              numpy rows in: upload, the generations on the device and the host's trial trees;
    device_seconds       everything but the trial trees: gather-pack, counts, gains, conditioned counts, partition, the
                         reads of gains and blocks;
    host_tree_seconds    mutual information, Prim and scores of the trial trees, and the leaves' tables.

The restatement runs once per learner on the same rows, on the host where the bench runs; the device result is checked
against it (OR tree, worst relative difference of a candidate score).  Writes one JSON line to ``--out`` (default
profiles/cnet_scored_bench_line.json) and prints it.

    python tools/bench_cnet_scored.py [--rows 20000] [--cols 64] [--cands 5] [--no-restatement]
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

from bench_cnet import timed, workload  # noqa: E402

ROOT_SEED = 7
PARS = {'bd': 0.1, 'bic': 0.01}


def learn(kind, x, cands):
    from deeprob.spn.learning import learn_cnet_bd, learn_cnet_bic
    if kind == 'bd':
        return learn_cnet_bd(x, ess=PARS[kind], n_cand_cuts=cands, random_state=ROOT_SEED)
    return learn_cnet_bic(x, alpha=PARS[kind], n_cand_cuts=cands, random_state=ROOT_SEED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=20000)
    ap.add_argument('--cols', type=int, default=64)
    ap.add_argument('--cands', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cnet_scored_bench_line.json'))
    ap.add_argument('--no-restatement', action='store_true')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_cnet_scored.py measures on a HIP device; none found')
    x, _ = workload(args.rows, args.cols)
    line = {'bench': 'cnet_scored', 'rows': args.rows, 'cols': args.cols, 'n_cand_cuts': args.cands, 'runs': args.runs,
            'pars': PARS, 'method': 'host clock around calls that end in a device synchronise; median after one warm-up',
            'learners': {}}
    for kind in ('bd', 'bic'):
        models, times = timed(lambda: learn(kind, x, args.cands), args.runs)
        model = models[-1]
        nodes = model._nodes()
        info = model.fit_profile_
        entry = {'hip_seconds': round(statistics.median(times), 5), 'hip_seconds_all': [round(v, 5) for v in times],
                 'phase_seconds': {k: round(statistics.median(m.fit_profile_[k] for m in models), 5)
                                   for k in ('device_seconds', 'host_tree_seconds')},
                 'model': {'or_nodes': sum(n.clt is None for n in nodes), 'leaves': sum(n.clt is not None for n in nodes)},
                 'generations': info['generations'], 'tasks_per_generation': info['tasks_per_generation'],
                 'entries': info['entries'], 'launches': info['launches'], 'gathers': info['gathers']}
        if not args.no_restatement:
            from tests import cnet_scored_ref as ref
            t0 = time.perf_counter()
            restated = ref.learn(x, kind, PARS[kind], args.cands, random_state=np.random.RandomState(ROOT_SEED))
            entry['restatement_seconds'] = round(time.perf_counter() - t0, 3)
            same = [(-1 if n.clt is not None else n.or_id) for n in nodes] == [r['or_id'] for r in restated]
            entry['checks'] = {'same_or_tree': bool(same)}
            if same:
                got = [s for n in nodes for _, s in n.candidates_]
                want = [s for r in restated for _, s in r['candidates']]
                entry['checks']['candidate_scores_max_rel_diff'] = float(
                    np.max(np.abs(np.array(got) - np.array(want)) / np.abs(want))) if len(want) == len(got) and want else None
        line['learners'][kind] = entry
    text = json.dumps(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
