"""What the two test files of ``learn_spn(learn_leaf=learn_binary_clt)`` share: the goldens of
tools/gen_golden_learnspn_clt.py, the call that replays a golden, and the expansion of a golden graph with BinaryCLT leaves
into the circuit this package builds.  A helper module, not a conftest."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CONFIGS = ['a', 'b']

_cache = {}


def golden(name):
    if name not in _cache:
        g = np.load(os.path.join(GOLDEN, 'learnspn_clt_%s.npz' % name))
        _cache[name] = {k: g[k] for k in g.files}
    return _cache[name]


def golden_leaves(name):
    """(node record of clt_json, the numbers of its training rows) of every CLT leaf, in the order the learner fits them."""
    g = golden(name)
    nodes = {int(r['id']): r for r in json.loads(str(g['clt_json']))['nodes']}
    off = g['leaf_row_off']
    return [(nodes[int(i)], g['leaf_rows'][off[k]:off[k + 1]]) for k, i in enumerate(g['leaf_node'])]


def call_kwargs(name, to_pc=False):
    """``(data, distributions, domains, keywords)`` of the ``learn_spn`` call that replays golden ``name``: (a) a learner
    seed and a separate RandomState for the leaves, (b) one RandomState object for both."""
    from deeprob.spn.structure.leaf import Bernoulli
    from deeprob.spn.learning.leaf import learn_binary_clt
    g = golden(name)
    n = g['data'].shape[1]
    if name == 'a':
        state, leaf_state = int(g['seed']), np.random.RandomState(int(g['leaf_seed']))
    else:
        state = leaf_state = np.random.RandomState(int(g['seed']))
    kw = dict(learn_leaf=learn_binary_clt, split_rows='random', split_cols='gvs', min_rows_slice=int(g['min_rows_slice']),
              learn_leaf_kwargs={'to_pc': to_pc, 'alpha': float(g['alpha']), 'random_state': leaf_state}, random_state=state,
              verbose=False)
    return g['data'].astype(np.float32), [Bernoulli] * n, [[0, 1]] * n, kw


def expand(digraph):
    """The FlatSpn of a reference graph whose BinaryCLT leaves are replaced by their ``to_pc_nodes()`` expansion: what
    ``learn_spn`` of this package returns for it.  No device."""
    from deeprob.spn.structure.cltree import BinaryCLT
    from deeprob.spn.learning.learnspn import new_node, to_flat
    built = {}
    for r in digraph['nodes']:
        if r['class'] == 'BinaryCLT':
            p = r['params']
            built[int(r['id'])] = BinaryCLT(r['scope'], tree=list(p['tree']), params=p['params']).to_pc_nodes()
        else:
            extra = {'weights': r['weights']} if r['class'] == 'Sum' else {}
            if r.get('params'):
                extra['params'] = r['params']
            built[int(r['id'])] = new_node(r['class'], r['scope'], **extra)
    for e in sorted(digraph['links' if 'links' in digraph else 'edges'], key=lambda e: (int(e['target']), int(e['idx']))):
        built[int(e['target'])]['children'].append(built[int(e['source'])])
    return to_flat(built[0])
