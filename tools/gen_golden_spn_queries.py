"""Golden vectors for the node-graph SPN queries (mpe, eval_backward, EM): the reference runs on its own JSON exports
under tests/golden/ (tools/gen_golden_spn.py) and on the stored inputs.  Outputs hold data only:
tests/golden/spn_queries_<name>.npz, spn_em_<name>.npz and the reference's export after EM, spn_<name>_em.json.

    cd tools && PYTHONPATH=<reference checkout>:.. python3 gen_golden_spn_queries.py
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, '..', 'tests', 'golden')
sys.path.insert(0, os.path.join(HERE, '..'))

GROUPS = ('sum_w', 'bern_p', 'cat_p', 'gauss_mean', 'gauss_std')
NUM_ITER, BATCH_PERC, STEP, SEED = 30, 0.5, 0.5, 42
GRAD_ROWS = 256         # rows of the 1000-row inputs kept for the gradient tables (file size)


class Recording(np.random.RandomState):
    """Keeps what `choice` returned: the batch rows of every EM iteration."""

    def __init__(self, seed):
        super().__init__(seed)
        self.rows = []

    def choice(self, *a, **k):
        r = super().choice(*a, **k)
        self.rows.append(np.asarray(r))
        return r


def ref_params(root):
    from deeprob.spn.structure.node import bfs, Sum
    from deeprob.spn.structure.leaf import Bernoulli, Categorical, Gaussian
    g = {k: [] for k in GROUPS}
    for n in sorted(bfs(root), key=lambda n: n.id):
        if isinstance(n, Sum):
            g['sum_w'] += [float(w) for w in n.weights]
        elif isinstance(n, Bernoulli):
            g['bern_p'].append(float(n.p))
        elif isinstance(n, Categorical):
            g['cat_p'] += [float(q) for q in n.probabilities]
        elif isinstance(n, Gaussian):
            g['gauss_mean'].append(float(n.mean))
            g['gauss_std'].append(float(n.stddev))
    return {k: np.asarray(v, np.float64) for k, v in g.items()}


def grad_err(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-12)) if len(b) else 0.0


def load(name):
    from deeprob.spn.structure.io import load_spn_json
    return load_spn_json(os.path.join(OUT, 'spn_%s.json' % name))


def gen_queries(circuit, vectors, rows=None):
    from deeprob.spn.algorithms.inference import mpe, log_likelihood
    from deeprob.spn.algorithms.gradient import eval_backward
    g = np.load(os.path.join(OUT, 'spn_%s.npz' % vectors))
    x = g['x'] if rows is None else g['x'][:rows]
    root = load(circuit)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        filled = mpe(root, g['x'])
        _, lls = log_likelihood(root, x, return_results=True)
        grads = eval_backward(root, lls)
    assert np.array_equal(lls, g['per_node'][:, :len(x)])
    np.savez_compressed(os.path.join(OUT, 'spn_queries_%s.npz' % vectors), n_rows=len(x),
                        mpe=np.asarray(filled, np.float32), grads=np.asarray(grads, np.float32))
    print(vectors, 'mpe', filled.shape, 'grads', grads.shape)


def gen_em(name, data):
    from deeprob.spn.learning.em import expectation_maximization
    from deeprob.spn.algorithms.inference import log_likelihood
    from deeprob.spn.structure.io import save_spn_json
    from tests import flat_spn_query_ref as qref
    d = json.load(open(os.path.join(OUT, 'spn_%s.json' % name)))
    out = {'data': data.astype(np.float32)}
    data = out['data']
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        root = load(name)
        out['ll_start'] = float(np.mean(log_likelihood(root, data)))
        # em_init alone
        from deeprob.spn.utils.filter import filter_nodes_by_type
        from deeprob.spn.structure.node import Sum
        from deeprob.spn.structure.leaf import Leaf
        rs = np.random.RandomState(SEED)
        for n in filter_nodes_by_type(root, Sum):
            n.em_init(rs)
        for n in filter_nodes_by_type(root, Leaf):
            n.em_init(rs)
        for k, v in ref_params(root).items():
            out['init.' + k] = v
        for tag, init in (('cold', False), ('rand', True)):
            for iters in (1, NUM_ITER):
                root, rs = load(name), Recording(SEED)
                expectation_maximization(root, data, num_iter=iters, batch_perc=BATCH_PERC, step_size=STEP,
                                         random_init=init, random_state=rs, verbose=False)
                got = ref_params(root)
                for k, v in got.items():
                    out['%s%d.%s' % (tag, iters, k)] = v
                index = np.stack(rs.rows).astype(np.int32)
                if iters == NUM_ITER:
                    out['index_' + tag] = index
                    out['ll_%s' % tag] = float(np.mean(log_likelihood(root, data)))
                    f64 = qref.params_of(qref.em_run(d, data, index, STEP, np.float64,
                                                     np.random.RandomState(SEED) if init else None))
                    out['dref_' + tag] = np.array([grad_err(got[k], f64[k]) for k in GROUPS])
                    print(name, tag, 'LL', out['ll_start'], '->', out['ll_' + tag], 'd_ref', out['dref_' + tag])
                    if not init:
                        save_spn_json(root, os.path.join(OUT, 'spn_%s_em.json' % name))
    np.savez_compressed(os.path.join(OUT, 'spn_em_%s.npz' % name), **out)


if __name__ == '__main__':
    gen_queries('binary16', 'binary16', GRAD_ROWS)
    gen_queries('binary16', 'binary16_nan', GRAD_ROWS)
    gen_queries('mixed4', 'mixed4')
    gen_em('binary16', np.load(os.path.join(OUT, 'spn_binary16.npz'))['x'])
    # 2000 complete rows of the mixed circuit, drawn by the reference's own sampler
    from deeprob.spn.algorithms.sampling import sample
    np.random.seed(7)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        drawn = sample(load('mixed4'), np.full((2000, 4), np.nan, np.float32))
    gen_em('mixed4', drawn)
