"""Golden LearnSPN runs of the reference with Chow-Liu tree leaves (deeprob/spn/learning/learnspn.py with
``learn_leaf=learn_binary_clt``) on the ``binary16`` data of gen_golden_learnspn.py: gvs column splits, random row splits.
Outputs hold data only: tests/golden/learnspn_clt_<config>.npz with the training data, the reference's ``save_spn_json``
text of ``learn_spn`` with ``to_pc=False`` (``clt_json``: the BinaryCLT leaves with their roots, trees and CPTs) and with
``to_pc=True`` (``pc_json``), the per-row log-likelihoods of the data and of a 30 % NaN copy under the ``to_pc=False``
model, the seeds and the G-test margin; and, for every CLT leaf in the order the learner fits them (its queue order),
the id of its node in ``clt_json`` (``leaf_node``) and the numbers of its training rows (``leaf_rows`` from
``leaf_row_off``).  The rows are followed through the reference's slicing by an ndarray subclass that carries them.

Two configurations:
  a  a learner seed and a SEPARATE RandomState(leaf seed) for the roots of the leaves.  The reference's learn_spn
     overwrites ``learn_leaf_kwargs['random_state']`` with its own generator (learnspn.py:112), so the separate generator
     is handed over by a wrapper of our own around its ``learn_binary_clt``;
  b  ONE RandomState(seed) object for the splits and the leaves, which is what the reference does by itself.

A seed is kept only if
  * every G-test is clear of its threshold, min |g - threshold| / threshold >= 1e-3 (as in gen_golden_learnspn.py), and
  * for every CLT leaf, Prim's algorithm on the float64 mutual information of the exact integer counts of that leaf's rows
    gives the reference's tree (then a float32 or a float64 evaluation, and any correct spanning-tree algorithm, agree on
    it).

    cd tools && PYTHONPATH=<reference checkout> python3 gen_golden_learnspn_clt.py
"""
import json
import os
import warnings

import numpy as np

from gen_golden_learnspn import MAX_BYTES, MIN_MARGIN, Margin, mixture, text_of

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, '..', 'tests', 'golden')
KS, N_ROWS, DATA_SEED = [2] * 16, 2000, 1
ALPHA = 0.1
MIN_ROWS_SLICE = 256
LEAF_SEED_OFFSET = 500


def prim_tree_f64(ones, n, root, alpha=ALPHA):
    """The predecessors of Prim's maximum spanning tree, from ``root``, of the float64 mutual information of the
    co-occurrence counts ``ones`` of ``n`` rows (the smoothing of the reference's estimate_priors_joints)."""
    d = ones.shape[0]
    col = np.diag(ones).astype(np.float64)
    cells = np.empty((d, d, 2, 2))
    cells[:, :, 1, 1] = ones
    cells[:, :, 0, 1] = col[None, :] - ones
    cells[:, :, 1, 0] = col[:, None] - ones
    cells[:, :, 0, 0] = n - col[None, :] - col[:, None] + ones
    joints = (cells + alpha) / (n + 4 * alpha)
    p1 = (col + 2 * alpha) / (n + 4 * alpha)
    priors = np.stack([1.0 - p1, p1], axis=1)
    outer = priors[:, None, :, None] * priors[None, :, None, :]
    mi = np.sum(joints * (np.log(joints) - np.log(outer)), axis=(2, 3))
    tree = np.full(d, -1, np.int64)
    best, link, inside = mi[root].copy(), np.full(d, root), np.zeros(d, bool)
    inside[root] = True
    for _ in range(d - 1):
        v = int(np.argmax(np.where(inside, -np.inf, best)))
        tree[v], inside[v] = link[v], True
        better = ~inside & (mi[v] > best)
        best[better], link[better] = mi[v][better], v
    return tree


class Tagged(np.ndarray):
    """A data matrix that remembers which rows of the training set it holds (``rows``) through the reference's slicing
    (rows.py:40 ``data[mask, :]``, cols.py:45 and learnspn.py:156-164 ``data[:, mask]``)."""
    rows = None

    def __array_finalize__(self, obj):
        self.rows = None

    def __getitem__(self, key):
        out = super().__getitem__(key)
        if isinstance(out, Tagged) and out.ndim == 2 and self.rows is not None and isinstance(key, tuple) and len(key) == 2:
            rows = self.rows if isinstance(key[0], slice) and key[0] == slice(None) else self.rows[key[0]]
            if np.ndim(rows) == 1 and len(rows) == out.shape[0]:
                out.rows = rows
        return out


def generate(name):
    from deeprob.spn.structure.leaf import Bernoulli
    from deeprob.spn.structure.cltree import BinaryCLT
    from deeprob.spn.learning import leaf as ref_leaf
    from deeprob.spn.learning.learnspn import learn_spn
    from deeprob.spn.learning.splitting import gvs
    from deeprob.spn.algorithms.inference import log_likelihood
    x, _ = mixture(KS, N_ROWS, DATA_SEED)
    data = x.astype(np.float32)
    dists, domains = [Bernoulli] * len(KS), [[0, 1]] * len(KS)

    def run(seed, to_pc, seen=None):
        """One reference run; ``seen`` collects (leaf, its row numbers) of every CLT leaf in the order they are fitted."""
        leaf_state = np.random.RandomState(seed + LEAF_SEED_OFFSET)

        def leaf_fn(local, d, dom, scope, to_pc=False, alpha=0.1, random_state=None):
            if name == 'a':
                random_state = leaf_state          # (the learner's own generator is left to the splits)
            leaf = ref_leaf.learn_binary_clt(np.asarray(local), d, dom, scope, to_pc=to_pc, alpha=alpha,
                                             random_state=random_state)
            if seen is not None and len(scope) > 1:
                assert np.array_equal(data[local.rows][:, scope], np.asarray(local))
                seen.append((leaf, local.rows.copy()))
            return leaf

        state = seed if name == 'a' else np.random.RandomState(seed)
        tagged = data.view(Tagged)
        tagged.rows = np.arange(len(data))
        return learn_spn(tagged, dists, domains, learn_leaf=leaf_fn, split_rows='random', split_cols='gvs',
                         learn_leaf_kwargs={'to_pc': to_pc, 'alpha': ALPHA}, min_rows_slice=MIN_ROWS_SLICE,
                         random_state=state, verbose=False)

    for seed in range(42, 142):
        seen = []
        with Margin(gvs) as m, warnings.catch_warnings():
            warnings.simplefilter('ignore')
            root = run(seed, False, seen)
            pc_root = run(seed, True)
        if m.value < MIN_MARGIN:
            print(name, 'seed', seed, 'margin', m.value, 'rejected')
            continue
        leaves = [leaf for leaf, _ in seen]
        assert leaves and all(isinstance(leaf, BinaryCLT) for leaf in leaves)
        agree = True
        for leaf, row_ids in seen:
            rows = data[row_ids][:, leaf.scope].astype(np.int64)
            tree = prim_tree_f64(rows.T @ rows, len(rows), int(leaf.root))
            agree = agree and np.array_equal(tree, np.asarray(leaf.tree))
        if not agree:
            print(name, 'seed', seed, 'rejected: a leaf tree differs from the float64 Prim tree')
            continue
        rs = np.random.RandomState(1000 + seed)
        mask = rs.rand(*data.shape) < 0.3
        x_nan = data.copy()
        x_nan[mask] = np.nan
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ll = np.asarray(log_likelihood(root, data), np.float64).reshape(-1)
            ll_nan = np.asarray(log_likelihood(root, x_nan), np.float64).reshape(-1)
        clt_text, pc_text = text_of(root), text_of(pc_root)
        path = os.path.join(OUT, 'learnspn_clt_%s.npz' % name)
        np.savez_compressed(path, data=x, ks=np.asarray(KS, np.int32), clt_json=np.asarray(clt_text), pc_json=np.asarray(pc_text),
                            ll=ll, ll_nan=ll_nan, nan_mask=np.packbits(mask), seed=seed,
                            leaf_seed=seed + LEAF_SEED_OFFSET if name == 'a' else -1, data_seed=DATA_SEED, alpha=ALPHA,
                            margin=m.value, gtest_calls=m.calls, min_rows_slice=MIN_ROWS_SLICE, clt_leaves=len(leaves),
                            leaf_node=np.asarray([leaf.id for leaf in leaves], np.int32),
                            leaf_rows=np.concatenate([r for _, r in seen]).astype(np.int32),
                            leaf_row_off=np.cumsum([0] + [len(r) for _, r in seen]).astype(np.int64))
        size = os.path.getsize(path)
        print(name, 'seed', seed, 'margin %.3g over %d g-tests' % (m.value, m.calls), 'nodes',
              len(json.loads(clt_text)['nodes']), '->', len(json.loads(pc_text)['nodes']), 'clt leaves', len(leaves),
              'mean LL %.4f' % ll.mean(), 'bytes', size)
        assert size <= MAX_BYTES, 'raise min_rows_slice or shrink the data'
        return
    raise SystemExit('no seed passed for configuration ' + name)


if __name__ == '__main__':
    for config in ('a', 'b'):
        generate(config)
