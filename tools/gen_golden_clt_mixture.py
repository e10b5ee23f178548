"""Golden batch-EM runs of the reference on a mixture of two BinaryCLTs, ``Sum([clt, clt])`` trained by
``expectation_maximization`` (deeprob/spn/learning/em.py, structure/cltree.py:117-155, structure/node.py:91-111).  The
output holds arrays only: tests/golden/clt_mixture_em.npz with

    data [600, 16] (packed bits): rows of two well-separated clusters; tree [2, 16], root [2]: two given trees (the
    structures the reference fits to the clusters); params [2, 16, 2, 2], weights [2]: given log CPTs and weights;
    <tag><iters>.weights / .params for tag in cold (random_init=False), rand (random_init=True) and iters in 1, 30: the
    reference's parameters after expectation_maximization(root, data, num_iter=iters, batch_perc=0.5, step_size=0.5,
    random_state=42); index_<tag> [30, 300]: the batch rows it drew; ll_start, ll_<tag>: the mean root log likelihood of
    the data before and after the 30 iterations; dref_<tag> [2]: the largest absolute difference of a probability
    (weights, CPTs) between the reference's float32 run and the float64 restatement of the same run
    (tests/clt_mixture_ref.py); step_*: one BinaryCLT.em_step of the first tree alone, its responsibilities step_stats
    [300] on the rows step_rows, step size 0.5, and the parameters step_params it leaves.

    cd tools && PYTHONPATH=<reference checkout>:.. python3 gen_golden_clt_mixture.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, '..', 'tests', 'golden')
sys.path.insert(0, os.path.join(HERE, '..'))

N_VARS, N_ROWS, NOISE = 16, 600, 0.15
NUM_ITER, BATCH_PERC, STEP, SEED = 30, 0.5, 0.5, 42
ROOTS = (0, 5)


class Recording(np.random.RandomState):
    """Keeps what `choice` returned: the batch rows of every EM iteration."""

    def __init__(self, seed):
        super().__init__(seed)
        self.rows = []

    def choice(self, *a, **k):
        r = super().choice(*a, **k)
        self.rows.append(np.asarray(r))
        return r


def two_clusters(rs):
    """Rows that copy one of two complementary prototypes, each entry replaced by a fair coin with probability NOISE."""
    proto = rs.randint(0, 2, size=N_VARS)
    label = (rs.rand(N_ROWS) < 0.4).astype(np.int64)
    x = np.where(label[:, None] == 1, 1 - proto, proto)
    flip = rs.rand(N_ROWS, N_VARS) < NOISE
    return np.where(flip, rs.randint(0, 2, size=x.shape), x).astype(np.float32), label


def model(trees, params, weights):
    from deeprob.spn.structure.cltree import BinaryCLT
    from deeprob.spn.structure.node import Sum, assign_ids
    scope = list(range(N_VARS))
    children = [BinaryCLT(scope, root=int(np.flatnonzero(t == -1)[0]), tree=t.copy(), params=p.copy())
                for t, p in zip(trees, params)]
    root = Sum(children=children, weights=weights.copy())
    assign_ids(root)
    return root


def main():
    from deeprob.spn.structure.cltree import BinaryCLT
    from deeprob.spn.learning.em import expectation_maximization
    from deeprob.spn.algorithms.inference import log_likelihood
    from tests import clt_mixture_ref as mref, clt_ref
    rs = np.random.RandomState(3)
    data, label = two_clusters(rs)
    scope = list(range(N_VARS))
    trees = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for c, root in enumerate(ROOTS):
            clt = BinaryCLT(scope, root=root)
            clt.fit(data[label == c], [[0, 1]] * N_VARS, alpha=0.1)
            trees.append(np.asarray(clt.tree, np.int32))
    # given CPTs and weights that are NOT the fit: EM has something to gain
    probs = 0.25 + 0.5 * rs.rand(2, N_VARS, 2)
    params = np.empty((2, N_VARS, 2, 2), np.float32)
    for c, root in enumerate(ROOTS):
        probs[c, root, 0] = probs[c, root, 1]
        params[c, :, :, 1] = probs[c]
        params[c, :, :, 0] = 1.0 - probs[c]
    params = np.log(params)
    weights = np.asarray([0.3, 0.7], np.float32)
    out = {'data': np.packbits(data.astype(bool)), 'n_rows': N_ROWS, 'n_vars': N_VARS, 'tree': np.stack(trees),
           'root': np.asarray(ROOTS, np.int32), 'params': params, 'weights': weights, 'step_size': STEP,
           'batch_perc': BATCH_PERC, 'seed': SEED}
    pairs = [(clt_ref.bfs_order(t), t) for t in trees]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out['ll_start'] = float(np.mean(log_likelihood(model(trees, params, weights), data)))
        for tag, init in (('cold', False), ('rand', True)):
            for iters in (1, NUM_ITER):
                root, rec = model(trees, params, weights), Recording(SEED)
                expectation_maximization(root, data, num_iter=iters, batch_perc=BATCH_PERC, step_size=STEP, random_init=init,
                                         random_state=rec, verbose=False)
                got_w = np.asarray(root.weights, np.float32)
                got_p = np.stack([np.asarray(c.params, np.float32) for c in root.children])
                out['%s%d.weights' % (tag, iters)], out['%s%d.params' % (tag, iters)] = got_w, got_p
                if iters == NUM_ITER:
                    index = np.stack(rec.rows).astype(np.int32)
                    out['index_' + tag] = index
                    out['ll_' + tag] = float(np.mean(log_likelihood(root, data)))
                    w64, p64, _ = mref.em_run(pairs, ROOTS, params, weights, data, index, STEP, np.float64,
                                              np.random.RandomState(SEED) if init else None)
                    out['dref_' + tag] = np.asarray(mref.prob_err(got_w, got_p, w64, p64))
                    print(tag, 'LL', out['ll_start'], '->', out['ll_' + tag], 'restated', mref.mean_ll(pairs, p64, w64, data),
                          'd_ref', out['dref_' + tag])
        # one em_step of the first tree alone
        rows = np.sort(rs.choice(N_ROWS, N_ROWS // 2, replace=False)).astype(np.int32)
        stats = rs.rand(len(rows)).astype(np.float32)
        clt = BinaryCLT(scope, root=ROOTS[0], tree=trees[0].copy(), params=params[0].copy())
        clt.em_step(stats, data[rows], STEP)
        out.update(step_rows=rows, step_stats=stats, step_params=np.asarray(clt.params, np.float32))
    path = os.path.join(OUT, 'clt_mixture_em.npz')
    np.savez_compressed(path, **out)
    print('bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
