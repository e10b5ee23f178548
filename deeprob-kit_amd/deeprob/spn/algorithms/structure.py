"""Structure transformations of a node-graph SPN (reference deeprob/spn/algorithms/structure.py) on a
:class:`deeprob.spn.structure.io.FlatSpn`.  Host code: the graph is small and is walked once."""
from collections import OrderedDict

import numpy as np

from deeprob.spn.structure.io import FlatSpn


def flat_to_nodes(flat: FlatSpn) -> list:
    """The circuit as one dict per node id (``class``, ``scope``, ``children`` as node objects, ``weights`` /
    ``params``): the form ``deeprob.spn.learning.learnspn`` builds and ``to_flat`` numbers."""
    nodes = []
    for i in range(flat.n_nodes):
        name = flat.classes[i]
        node = {'class': name, 'scope': list(flat._scope_as_given[i]), 'children': []}
        if name == 'Sum':
            c0, nc = int(flat.arg0[i]), int(flat.arg1[i])
            node['weights'] = [np.float32(w) for w in flat.child_weight[c0:c0 + nc]]
        elif name == 'Bernoulli':
            node['params'] = {'p': float(flat.raw0[i])}
        elif name == 'Categorical':
            c0, nc = int(flat.arg1[i]), int(flat.arg2[i])
            node['params'] = {'categories': [int(c) for c in flat.cat_value[c0:c0 + nc]],
                              'probabilities': [float(q) for q in flat.probabilities[c0:c0 + nc]]}
        elif name == 'Uniform':
            node['params'] = {'start': float(flat.raw0[i]), 'width': float(flat.raw1[i])}
        elif name == 'Gaussian':
            node['params'] = {'mean': float(flat.raw0[i]), 'stddev': float(flat.raw1[i])}
        nodes.append(node)
    for i in range(flat.n_nodes):
        nodes[i]['children'] = [nodes[c] for c in flat.children[i]]
    return nodes


def prune_nodes(root: dict) -> dict:
    """``prune`` on the dict form (reference structure.py:33-77): in reversed topological order a node with one child
    becomes that child, the children of a product's product children move up, the children of a sum's sum children
    move up with multiplied weights (a child reached twice gets the sum of its weights: DAG-safe).  Returns the new
    root; nodes are modified in place."""
    from deeprob.spn.learning.learnspn import topological_order
    nodes = topological_order(root)
    mapped = {id(n): n for n in nodes}
    for node in reversed(nodes):
        if node['class'] not in ('Sum', 'Product'):
            continue
        kids = [mapped[id(c)] for c in node['children']]
        if len(kids) == 1:
            mapped[id(node)] = kids[0]
        elif node['class'] == 'Product':
            children = []
            for child in kids:
                if child['class'] != 'Product':
                    children.append(child)
                else:
                    children.extend(mapped[id(c)] for c in child['children'])
            node['children'] = children
        else:
            weights = OrderedDict()            # child -> weight, in order of first appearance; float32 as the reference's
            keep = {}
            for i, child in enumerate(kids):
                w = np.float32(node['weights'][i])
                if child['class'] != 'Sum':
                    weights[id(child)] = np.float32(weights.get(id(child), np.float32(0.0)) + w)
                    keep[id(child)] = child
                    continue
                for j, sub in enumerate(mapped[id(c)] for c in child['children']):
                    weights[id(sub)] = np.float32(weights.get(id(sub), np.float32(0.0)) + w * np.float32(child['weights'][j]))
                    keep[id(sub)] = sub
            node['weights'] = list(weights.values())
            node['children'] = [keep[k] for k in weights]
    return mapped[id(root)]


def prune(root: FlatSpn, copy: bool = True) -> FlatSpn:
    """
    Prune (or simplify) the given SPN to a minimal and equivalent SPN (reference structure.py:16-77).

    :param root: The SPN.
    :param copy: Accepted for compatibility: a FlatSpn is never modified, the result is always a new one.
    :return: A minimal and equivalent SPN, numbered in ``assign_ids`` order.
    :raises ValueError: If the SPN is not smooth and decomposable or not a DAG.
    """
    from deeprob.spn.learning.learnspn import to_flat
    root.check()
    return to_flat(prune_nodes(flat_to_nodes(root)[root.root]))
