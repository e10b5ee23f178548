"""Golden XPC runs of the reference (deeprob/spn/learning/xpc.py) on small binary data sets.  Outputs hold data only:
tests/golden/xpc_<config>.npz with

    data (packed bits) / n_rows / n_vars / data_seed, fresh_bits (512 fresh rows of the same mixture),
    n_members and, per member m (prefix m<m>_): the reference's partition tree in pre-order -- masks (the row sets as bit
    masks), cols / col_off, flags (is_naive, is_conj), n_subs, disc / disc_off / has_disc (the sorted disc_assignments) --,
    conj_vars (the conjunctions, [K, conj_len]), n_parts, trees_dict as keys / tree / scope / off / given, and
    tree_unique: per tree the dictionary is chained from (bottom first), whether it is the only maximum spanning tree of
    the cumulative information (only_spanning_tree of gen_golden_cnet.py),
    ll_train, ll_fresh, ll_nan: the reference's log likelihoods of the training rows, the fresh rows and 256 fresh rows
    with 40 % NaN (tests/xpc_ref.queries).

The hyper-parameters are those of tests/xpc_ref.CONFIGS[<config>]; ensembles run under np.random.seed(xpc_ref.GLOBAL_SEED).

A fixture is written only if the restatement (tests/xpc_ref.py) makes every decision the reference made -- the partition
tree, the greedy ordering, conj_vars_l, n_parts, the scopes and roots of trees_dict -- and its float64 log likelihoods are
within 1e-5 of the reference's on all three row sets.  Where a tree has several maximum spanning trees, which one a routine
returns is a matter of its order of visits (scipy's Kruskal, the package's Prim and the restatement's differ) and the
likelihood of a row follows the tree.  So every Chow-Liu leaf that learns its own tree must have exactly one maximum spanning
tree of its float32 weights mi + 1, and a data seed with a tie is passed over; for the trees of trees_dict the tie is
recorded (tree_unique) and at least one structured-decomposable fixture must have only unique trees.  The data seed of a
configuration is chosen accordingly: `--search` tries the seeds from the configured one upwards and reports the first
that passes; tests/xpc_ref.CONFIGS then records it.

    cd tools && PYTHONPATH=<reference checkout> python3 gen_golden_xpc.py [--search] [config ...]
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.append(ROOT)          # (after the reference: `deeprob` is the reference's, `tests` is this project's)

from tests import cnet_ref, xpc_ref  # noqa: E402
from gen_golden_cnet import only_spanning_tree  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
MAX_BYTES = 150 * 1000
LL_BAR = 1e-5


class Refused(Exception):
    pass


def as_dicts(part):
    """A reference Partition tree as the dicts of tests/xpc_ref.py."""
    node = xpc_ref._part(part.row_ids, part.col_ids, part.uncond_vars, None, bool(part.is_naive), bool(part.is_conj))
    if part.disc_assignments is not None:
        node['disc'] = sorted(tuple(int(v) for v in a) for a in part.disc_assignments)
    node['subs'] = [as_dicts(sub) for sub in part.sub_partitions]
    return node


def close(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def generate(name, seed=None):
    from deeprob.spn.algorithms.inference import log_likelihood
    from deeprob.spn.learning import xpc as ref_xpc
    learner, (n, d, k, noise, data_seed), kw = xpc_ref.CONFIGS[name]
    data_seed = data_seed if seed is None else seed
    data, fresh = cnet_ref.mixture(n, d, k, noise, data_seed)
    nan_rows = xpc_ref.queries(fresh)
    greedy = []
    keep = ref_xpc.greedy_vars_ordering
    ref_xpc.greedy_vars_ordering = lambda *a, **b: greedy.append(keep(*a, **b)) or list(greedy[-1])
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if learner == 'xpc':
                circuit, utils = ref_xpc.learn_xpc(data, **kw)
                utils = [utils]
            else:
                np.random.seed(xpc_ref.GLOBAL_SEED)
                circuit, utils = ref_xpc.learn_expc(data, **kw)
            ll = [np.asarray(log_likelihood(circuit, rows)).reshape(-1).astype(np.float64) for rows in (data, fresh, nan_rows)]
    except (AssertionError, KeyError, AttributeError) as e:
        raise Refused('the reference fails: %r' % (e,))
    finally:
        ref_xpc.greedy_vars_ordering = keep
    model = xpc_ref.learn(learner, data, kw)
    if greedy and greedy[0] != xpc_ref.greedy_ordering(data, kw['conj_len']):
        raise Refused('the greedy ordering differs')

    out = dict(data=np.packbits(data.astype(bool)), n_rows=n, n_vars=d, data_seed=data_seed,
               fresh_bits=np.packbits(fresh.astype(bool)), n_members=len(utils), ll_train=ll[0], ll_fresh=ll[1], ll_nan=ll[2])
    alpha = kw.get('alpha', 0.01)
    sd2 = learner == 'expc' and kw['sd_level'] == 2
    for m, (u, mine) in enumerate(zip(utils, model['members'])):
        theirs = xpc_ref.tree_record(as_dicts(u['part_root']), n)
        if not xpc_ref.same_tree(theirs, xpc_ref.tree_record(mine['root'], n)):
            raise Refused('member %d: the partition tree differs' % m)
        conj = [[int(v) for v in c] for c in u['conj_vars_l']]
        if conj != mine['conj_vars_l'] or int(u['n_parts']) != mine['n_parts']:
            raise Refused('member %d: conj_vars_l or n_parts differ' % m)
        for a, b in zip(u['cl_parts_l'], mine['cl_parts']):
            if not np.array_equal(a.row_ids, b['rows']) or a.col_ids.tolist() != b['cols']:
                raise Refused('member %d: cl_parts_l differs' % m)
        ref_trees = None if u['trees_dict'] is None else {k: ([int(t) for t in v[0]], [int(s) for s in v[1]])
                                                          for k, v in u['trees_dict'].items()}
        unique = []
        if ref_trees is not None:
            got, want = xpc_ref.segments(mine['trees_dict']), xpc_ref.segments(ref_trees)
            if [s for s, _ in got] != [s for s, _ in want] or [t.index(-1) for _, t in got] != [t.index(-1) for _, t in want]:
                raise Refused('member %d: the scopes or roots of trees_dict differ' % m)
            parts_l = [x['cl_parts'] for x in model['members']] if sd2 else [mine['cl_parts']]
            info = xpc_ref.cumulative_information(data, parts_l, alpha)
            unique = [len(s) == 1 or only_spanning_tree(info[s][:, s], np.asarray(t)) for s, t in want]
        record = dict(theirs, conj_vars=np.array(conj, np.int32).reshape(-1, kw['conj_len']), n_parts=int(u['n_parts']),
                      tree_unique=np.array(unique, np.uint8), **xpc_ref.trees_record(ref_trees))
        out.update({'m%d_%s' % (m, key): value for key, value in record.items()})
    return out, model, ll, nan_rows, fresh, data


def verdict(name, seed=None):
    """The fixture of a configuration, or Refused with the reason."""
    out, model, ll, nan_rows, fresh, data = generate(name, seed)
    # a Chow-Liu leaf that learns its own tree: with several maximum spanning trees of its weights, which one a
    # spanning-tree routine returns is a matter of its order of visits, and the likelihoods follow the tree
    for m in model['members']:
        for node in xpc_ref.preorder(m['root']):
            leaf = node['leaf']
            if leaf is not None and leaf[0] == 'clt' and m['trees_dict'] is None and len(leaf[1]) > 1:
                mi = xpc_ref._mutual_information(data[node['rows']][:, leaf[1]], 0.01)
                if not only_spanning_tree(mi, np.asarray(leaf[3])):
                    raise Refused('a leaf has several maximum spanning trees')
    worst = max(close(xpc_ref.log_likelihood(model, rows), want) for rows, want in zip((data, fresh, nan_rows), ll))
    if not worst <= LL_BAR:
        raise Refused('the restatement is %g away from the reference (a leaf with several maximum spanning trees?)' % worst)
    return out, worst


def main(argv):
    search = '--search' in argv
    names = [a for a in argv if not a.startswith('--')] or list(xpc_ref.CONFIGS)
    for name in names:
        base = xpc_ref.CONFIGS[name][1][4]
        for seed in range(base, base + (200 if search else 1)):
            try:
                out, worst = verdict(name, seed)
            except Refused as e:
                print('%s seed %d: refused, %s' % (name, seed, e))
                continue
            path = os.path.join(OUT, 'xpc_%s.npz' % name)
            np.savez_compressed(path, **out)
            size = os.path.getsize(path)
            assert size <= MAX_BYTES, '%s is %d bytes' % (path, size)
            print('%s seed %d: written, %d bytes, %d members, restatement within %.2g of the reference' % (
                name, seed, size, int(out['n_members']), worst))
            break
        else:
            raise SystemExit('%s: no fixture written' % name)
    unique_sd = []
    for n in xpc_ref.CONFIGS:
        path = os.path.join(OUT, 'xpc_%s.npz' % n)
        if os.path.isfile(path):
            f = np.load(path)
            flags = [f[k] for k in f.files if k.endswith('_tree_unique')]
            if all(len(v) for v in flags) and all(v.all() for v in flags):
                unique_sd.append(n)
    assert unique_sd, 'no sd fixture has only unique spanning trees'
    print('sd fixtures with only unique spanning trees:', ' '.join(unique_sd))


if __name__ == '__main__':
    main(sys.argv[1:])
