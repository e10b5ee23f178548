"""Golden runs of the reference's scored cutset learners (deeprob/spn/learning/cnet_bayesian.py: learn_cnet_bd,
learn_cnet_bic) on the mixtures of tests/cnet_ref.py.  Outputs hold data only: tests/golden/cnet_<learner>_<config>.npz with

    data (packed bits) / n_rows / n_vars, learner (0 bd, 1 bic), par (ess or alpha), n_cand_cuts,
    the reference's OR tree in breadth-first order (left child before right): or_id (-1 at a leaf), weights, is_leaf,
    n_node_rows, node_depth, the leaves' scopes and undirected edge sets (as tools/gen_golden_cnet.py stores them) and
    leaf_unique (its only_spanning_tree rule on the mutual information the tree was taken from),
    node_score (the score of every node's single tree), cand_off / cand_vars / cand_scores (per node with more than one
    variable, every candidate that has two non-empty sides, by increasing variable id, with the score of cutting there),
    ll_train, fresh_bits and ll_fresh,
    the reference's helpers on the whole training matrix: helper_cands (select_cand_cuts, sorted), helper_or_scores,
    helper_clt_scores (ess = par for bd, 4 par for bic) and helper_deviation, the largest relative deviation of the
    float64 restatement (tests/cnet_scored_ref.py) from them (the pairwise scores off the diagonal),
    and the margins found: selection_margin, decision_margin, score_deviation, candidate_margin.

The reference draws the root of every trial tree from an unseeded generator; the scores depend on it by rounding only.
The scores are recomputed here per node of the reference's result with the reference's own functions.

The package scores in float64 from exact counts, the reference mixes float32 in, so a fixture is written only if, on the
reference's run,
  * every chosen candidate beats the runner-up by at least 1e-4 relative,
  * every split / no-split decision differs from the node's own score by at least 1e-4 relative,
  * both are at least 4 times score_deviation, the largest relative deviation between the reference's scores and the
    restatement's on that run,
  * the candidate set is unambiguous: the k-th and (k+1)-th gains differ by at least 1e-6 relative,
and the restatement makes every decision the reference made.

    cd tools && PYTHONPATH=<reference checkout> python3 gen_golden_cnet_scored.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.append(ROOT)          # (after the reference: `deeprob` is the reference's, `tests` is this project's)
if HERE not in sys.path:
    sys.path.append(HERE)

from tests import cnet_ref, cnet_scored_ref as scored  # noqa: E402
from gen_golden_cnet import only_spanning_tree  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
MAX_BYTES = 150 * 1000
SELECTION_MARGIN = DECISION_MARGIN = 1e-4
CANDIDATE_MARGIN = 1e-6
DEVIATION_FACTOR = 4.0


def rel(a, b):
    return abs(a - b) / abs(b)


def generate(name):
    import deeprob.spn.learning.cnet_bayesian as cb
    from deeprob.spn.structure.cltree import BinaryCLT
    from deeprob.utils.statistics import estimate_priors_joints, compute_mutual_information
    _, kind, par, n_cand = scored.CONFIGS[name]
    data, fresh = scored.data_of(name)
    n, d = data.shape
    warnings.simplefilter('ignore')
    model = cb.learn_cnet_bd(data, ess=par, n_cand_cuts=n_cand) if kind == 'bd' else \
        cb.learn_cnet_bic(data, alpha=par, n_cand_cuts=n_cand)
    ll_train, ll_fresh = model.log_likelihood(data), model.log_likelihood(fresh)

    def tree_score(part, depth):
        """The reference's score of the single tree of a partition at ``depth``."""
        width = part.shape[1]
        clt = BinaryCLT(scope=list(range(width)))
        if kind == 'bd':
            ess = par / 2.0 ** depth
            clt.fit(part, [[0, 1]] * width, alpha=0.01)
            return float(cb.eval_tree_score(clt.tree, cb.compute_clt_bd_scores(part, ess), cb.compute_or_bd_scores(part, ess)))
        clt.fit(part, [[0, 1]] * width, alpha=par)
        return float(np.sum(clt.log_likelihood(part)) - 0.5 * np.log(n) * (2 * width - 1))

    nodes, depth_of, at = [model], {id(model): 0}, 0
    while at < len(nodes):
        if nodes[at].clt is None:
            nodes += nodes[at].children
            for c in nodes[at].children:
                depth_of[id(c)] = depth_of[id(nodes[at])] + 1
        at += 1
    mine = scored.learn(data, kind, par, n_cand, roots=np.zeros(len(nodes), np.int64))
    assert len(mine) == len(nodes), '%s: the restatement has %d nodes, the reference %d' % (name, len(mine), len(nodes))

    or_id, weights, rows, depths, scopes, edges, unique, node_score = [], [], [], [], [], [], [], []
    cand_off, cand_vars, cand_scores = [0], [], []
    selection = decision = candidate = np.inf
    deviation = 0.0
    for node, restated in zip(nodes, mine):
        depth = depth_of[id(node)]
        part = data[node.row_indices][:, node.col_indices]
        scope = list(node.scope)
        assert scope == [int(c) for c in node.col_indices] == restated['scope']
        rows.append(len(node.row_indices))
        depths.append(depth)
        own = tree_score(part, depth)
        node_score.append(own)
        deviation = max(deviation, rel(restated['score'], own))
        found = {}
        if len(scope) > 1:
            ess = par / 2.0 ** depth
            k = min(n_cand, len(scope))
            smoothing = ess if kind == 'bd' else 4 * par
            idx = sorted(int(i) for i in np.atleast_1d(cb.select_cand_cuts(part, ess=smoothing, n_cand_cuts=k)))
            order, gains = scored.candidates(part, smoothing / 4, k)
            assert idx == sorted(order), '%s: candidate sets differ at a node of %d rows' % (name, len(part))
            ranked = np.sort(gains)[::-1]
            if len(ranked) > k:
                candidate = min(candidate, (ranked[k - 1] - ranked[k]) / abs(ranked[k - 1]))
            or_scores = cb.compute_or_bd_scores(part, ess) if kind == 'bd' else None
            for i in idx:
                right = part[:, i] == 1
                n_left, n_right = int((~right).sum()), int(right.sum())
                if n_left == 0 or n_right == 0:
                    continue
                rest = np.delete(np.arange(len(scope)), i)
                total = tree_score(part[~right][:, rest], depth + 1) + tree_score(part[right][:, rest], depth + 1)
                if kind == 'bd':
                    total += float(or_scores[i])
                else:
                    left_weight = (n_left + par) / (n_left + n_right + 2 * par)
                    total += n_left * np.log(left_weight) + n_right * np.log(1 - left_weight) - 0.5 * np.log(n)
                found[scope[i]] = float(total)
            theirs = dict(restated['candidates'])
            assert sorted(theirs) == sorted(found)
            deviation = max([deviation] + [rel(theirs[v], s) for v, s in found.items()])
        for v in sorted(found):
            cand_vars.append(v)
            cand_scores.append(found[v])
        cand_off.append(len(cand_vars))
        if found:
            ranked = sorted(found.values(), reverse=True)
            decision = min(decision, rel(ranked[0], own))
            if len(ranked) > 1 and ranked[0] > own:
                selection = min(selection, (ranked[0] - ranked[1]) / abs(ranked[0]))
        if node.clt is None:
            best = max(found, key=found.get)
            assert best == node.or_id == restated['or_id'] and found[best] > own
            or_id.append(int(node.or_id))
            weights.append([float(w) for w in node.weights])
            unique.append(False)
            scopes.append(None)
            edges.append(None)
            continue
        assert restated['or_id'] == -1 and (not found or not max(found.values()) > own)
        or_id.append(-1)
        weights.append([np.nan, np.nan])
        mi = compute_mutual_information(*estimate_priors_joints(part, alpha=0.01 if kind == 'bd' else par))
        unique.append(len(scope) == 1 or only_spanning_tree(mi, node.clt.tree))
        scopes.append(scope)
        edges.append(cnet_ref.edge_set(scope, node.clt.tree))

    smoothing = par if kind == 'bd' else 4 * par
    k = min(n_cand, d)
    helper_cands = np.sort(np.atleast_1d(cb.select_cand_cuts(data, ess=smoothing, n_cand_cuts=k))).astype(np.int32)
    helper_or = np.asarray(cb.compute_or_bd_scores(data, smoothing), np.float64)
    helper_clt = np.asarray(cb.compute_clt_bd_scores(data, smoothing), np.float64)
    pairs = ~np.eye(d, dtype=bool)          # (i, i) is no family of any tree: a sum of a few units that the reference's
    #                                         float32 terms of 1e4 leave with 1e-3 relative error
    helper_deviation = max(float(np.max(np.abs(scored.or_bd_scores(data, smoothing) - helper_or) / np.abs(helper_or))),
                           float(np.max((np.abs(scored.clt_bd_scores(data, smoothing) - helper_clt) / np.abs(helper_clt))[pairs])))
    assert helper_cands.tolist() == sorted(scored.candidates(data, smoothing / 4, k)[0])

    print(name, 'selection margin %.3g decision margin %.3g score deviation %.3g candidate margin %.3g helper deviation %.3g'
          % (selection, decision, deviation, candidate, helper_deviation))
    assert selection >= SELECTION_MARGIN, '%s: selection margin %g' % (name, selection)
    assert decision >= DECISION_MARGIN, '%s: decision margin %g' % (name, decision)
    assert min(selection, decision) >= DEVIATION_FACTOR * deviation, '%s: score deviation %g' % (name, deviation)
    assert candidate >= CANDIDATE_MARGIN, '%s: candidate margin %g' % (name, candidate)

    scope_off = np.concatenate([[0], np.cumsum([0 if s is None else len(s) for s in scopes])])
    edge_off = np.concatenate([[0], np.cumsum([0 if e is None else len(e) for e in edges])])
    flat_edges = np.array([p for e in edges if e for p in e], np.int32).reshape(-1, 2)
    path = os.path.join(OUT, 'cnet_%s.npz' % name)
    np.savez_compressed(
        path, data=np.packbits(data.astype(bool)), n_rows=n, n_vars=d, learner=0 if kind == 'bd' else 1, par=par,
        n_cand_cuts=n_cand, or_id=np.array(or_id, np.int32), weights=np.array(weights, np.float64),
        is_leaf=np.array(or_id, np.int32) < 0, n_node_rows=np.array(rows, np.int32), node_depth=np.array(depths, np.int32),
        leaf_unique=np.array(unique, bool), leaf_scopes=np.array([v for s in scopes if s for v in s], np.int32),
        leaf_scope_off=scope_off.astype(np.int32), leaf_edges=flat_edges, leaf_edge_off=edge_off.astype(np.int32),
        node_score=np.array(node_score, np.float64), cand_off=np.array(cand_off, np.int32),
        cand_vars=np.array(cand_vars, np.int32), cand_scores=np.array(cand_scores, np.float64),
        ll_train=np.asarray(ll_train, np.float32), fresh_bits=np.packbits(fresh.astype(bool)),
        ll_fresh=np.asarray(ll_fresh, np.float32), helper_cands=helper_cands, helper_or_scores=helper_or,
        helper_clt_scores=helper_clt, helper_deviation=helper_deviation, selection_margin=selection,
        decision_margin=decision, score_deviation=deviation, candidate_margin=candidate)
    size = os.path.getsize(path)
    n_or = int((np.array(or_id) >= 0).sum())
    print(name, 'OR nodes', n_or, 'leaves', len(or_id) - n_or, 'leaves with one spanning tree', sum(unique), 'bytes', size)
    assert size <= MAX_BYTES


if __name__ == '__main__':
    for config in (sys.argv[1:] or scored.CONFIGS):
        generate(config)
