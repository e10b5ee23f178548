"""Loading a vanilla (node-graph) SPN from the reference's JSON format (deeprob/spn/structure/io.py:59-102,
133-220) into the flat arrays the HIP evaluator walks.

``load_spn_json`` returns a :class:`FlatSpn` -- node kinds, parameters and a child list per node over the file's node
ids -- instead of a tree of ``Node`` objects; ``deeprob.spn.algorithms`` (``log_likelihood``, ``mpe``, ``sample``,
``eval_backward``) and ``deeprob.spn.learning.em`` work on it on a HIP device, ``save_spn_json`` writes it back.
"""
import json
import math
import os
from typing import IO, Dict, List, Optional, Union

import numpy as np

KIND = {'Sum': 0, 'Product': 1, 'Bernoulli': 2, 'Categorical': 3, 'Uniform': 4, 'Gaussian': 5}


class FlatSpn:
    """A labelled SPN as arrays over node ids ``0..n_nodes-1`` (root = 0, as ``digraph_to_spn`` returns
    ``nodes[0]``, reference io.py:219): see ``include/deeprob_hip.h`` (dpk_flat_spn_forward) for the layout."""

    def __init__(self, nodes: Dict[int, dict], children: Dict[int, List[int]], root: int = 0):
        ids = sorted(nodes)
        if ids != list(range(len(ids))):
            raise ValueError("SPN is not correctly labeled: node ids must be 0..n-1")
        n = len(ids)
        self.n_nodes, self.root = n, root
        self.scopes = [sorted(int(v) for v in nodes[i]['scope']) for i in ids]
        self.classes = [nodes[i]['class'] for i in ids]
        self.children = [list(children.get(i, [])) for i in ids]
        self.order = np.asarray(self._evaluation_order(), dtype=np.int32)
        self.kind = np.zeros(n, np.int32)
        self.arg0, self.arg1, self.arg2 = (np.zeros(n, np.int32) for _ in range(3))
        self.par0, self.par1 = np.zeros(n, np.float64), np.zeros(n, np.float64)
        # the leaves' own parameters (par0 / par1 / cat_logp are derived from them, see refresh()):
        # raw0 = Bernoulli p | Uniform start | Gaussian mean, raw1 = Uniform width | Gaussian stddev
        self.raw0, self.raw1 = np.zeros(n, np.float64), np.zeros(n, np.float64)
        self._scope_as_given = [[int(v) for v in nodes[i]['scope']] for i in ids]
        child_index, child_weight, cat_value, cat_logp, cat_prob = [], [], [], [], []
        for i in ids:
            node, name, kids = nodes[i], nodes[i]['class'], self.children[i]
            if name not in KIND:
                raise ValueError("Unknown node of type {}".format(name))
            self.kind[i] = KIND[name]
            if name in ('Sum', 'Product'):
                if not kids:
                    raise ValueError("Inner node {} has no children".format(i))
                self.arg0[i], self.arg1[i] = len(child_index), len(kids)
                if name == 'Sum':
                    weights = np.asarray(node['weights'], dtype=np.float32)      # node.py:83-84
                    if len(weights) != len(kids):
                        raise ValueError("Each child of a sum node must be associated a weight")
                    if not np.isclose(np.sum(weights), 1.0):
                        raise ValueError("Weights don't sum up to 1")
                    child_weight += [float(w) for w in weights]
                else:
                    child_weight += [1.0] * len(kids)
                child_index += kids
                continue
            if kids:
                raise ValueError("Leaf node {} has children".format(i))
            if len(self.scopes[i]) != 1:
                raise ValueError("Leaf node {} must have a single variable in its scope".format(i))
            self.arg0[i] = self.scopes[i][0]
            prm = node.get('params', {})
            if name == 'Bernoulli':            # scipy.stats.bernoulli.logpmf: log p at 1, log1p(-p) at 0
                p = float(prm['p'])
                self.raw0[i] = p
                self.par0[i] = math.log(p) if p > 0.0 else -math.inf
                self.par1[i] = math.log1p(-p) if p < 1.0 else -math.inf
            elif name == 'Categorical':        # rv_discrete over float32 probabilities (leaf.py:236-239)
                cats = np.asarray(prm['categories'], dtype=np.int64)
                probs = np.asarray(prm['probabilities'], dtype=np.float32)
                if len(cats) != len(probs):
                    raise ValueError("Each category must be associated a probability")
                if not np.isclose(np.sum(probs), 1.0):
                    raise ValueError("Probabilities parameter must sum up to 1")
                self.arg1[i], self.arg2[i] = len(cat_value), len(cats)
                cat_value += [int(c) for c in cats]
                cat_prob += [float(v) for v in probs]
                with np.errstate(divide='ignore'):
                    cat_logp += [float(v) for v in np.log(probs.astype(np.float64))]
            elif name == 'Uniform':
                self.par0[i], self.par1[i] = float(prm['start']), float(prm['width'])
                self.raw0[i], self.raw1[i] = self.par0[i], self.par1[i]
            else:
                self.par0[i], self.par1[i] = float(prm['mean']), float(prm['stddev'])
                self.raw0[i], self.raw1[i] = self.par0[i], self.par1[i]
        self.child_index = np.asarray(child_index or [0], dtype=np.int32)
        self.child_weight = np.asarray(child_weight or [0.0], dtype=np.float32)
        self.cat_value = np.asarray(cat_value or [0], dtype=np.int32)
        self.cat_logp = np.asarray(cat_logp or [0.0], dtype=np.float32)
        #: Categorical probabilities, parallel to ``cat_value`` (float32 values as loaded, float64 after EM: leaf.py:239,278)
        self.probabilities = np.asarray(cat_prob or [1.0], dtype=np.float64)
        with np.errstate(divide='ignore'):
            self.child_logw = np.log(self.child_weight)                  # float32, as inference.py:125 takes it
        self.sum_index = np.full(n, -1, np.int32)
        sums = np.flatnonzero(self.kind == KIND['Sum'])
        self.sum_index[sums] = np.arange(len(sums), dtype=np.int32)
        self.n_sum = int(len(sums))
        self.max_children = int(self.arg1[sums].max()) if len(sums) else 0
        self.n_slots, self.node_slot = self._allocate_slots()
        self.child_slot = self.node_slot[self.child_index].astype(np.int32) if child_index else self.child_index
        self.n_features = 1 + max(max(s) for s in self.scopes)
        self._checked = False
        self._device = {}

    def _evaluation_order(self) -> List[int]:
        """Children before parents, every node reachable from the root once; a cycle is an error (reference:
        topological_order returning None, evaluation.py:79-81)."""
        order, state = [], [0] * self.n_nodes
        stack = [(self.root, 0)]
        while stack:
            node, k = stack.pop()
            if k == 0:
                if state[node] == 2:
                    continue
                state[node] = 1
            if k < len(self.children[node]):
                stack.append((node, k + 1))
                c = self.children[node][k]
                if state[c] == 1:
                    raise ValueError("SPN structure is not a directed acyclic graph (DAG)")
                if state[c] == 0:
                    stack.append((c, 0))
            else:
                state[node] = 2
                order.append(node)
        if len(order) != self.n_nodes:
            raise ValueError("SPN is not correctly labeled: {} nodes are not reachable from the root".format(
                self.n_nodes - len(order)))
        return order

    def _allocate_slots(self):
        """Rows of the evaluator's on-chip value table: a node keeps its row until its last parent (in evaluation
        order) has been computed, then the row returns to the free list."""
        position = {int(n): t for t, n in enumerate(self.order)}
        last_use = [position[i] for i in range(self.n_nodes)]        # a node nobody reads dies where it is born
        for parent in range(self.n_nodes):
            for c in self.children[parent]:
                last_use[c] = max(last_use[c], position[parent])
        last_use[self.root] = self.n_nodes                           # the root's row is read at the end
        expiring = {}
        for i, t in enumerate(last_use):
            expiring.setdefault(t, []).append(i)
        slot = np.zeros(self.n_nodes, np.int32)
        free, used = [], 0
        for t, node in enumerate(self.order):
            node = int(node)
            if free:
                slot[node] = free.pop()
            else:
                slot[node] = used
                used += 1
            # rows whose last reader is this node are free from the next node on (a node's own row is written
            # after its children's rows have been read)
            for dead in expiring.get(t, []):
                free.append(int(slot[dead]))
        return used, slot

    def check(self):
        """Smoothness and decomposability, as ``check_spn`` enforces before every evaluation (reference
        evaluation.py:67, utils/validity.py)."""
        if self._checked:
            return
        for i in range(self.n_nodes):
            kids, scope = self.children[i], self.scopes[i]
            if self.classes[i] == 'Sum':
                if any(self.scopes[c] != scope for c in kids):
                    raise ValueError("SPN is not smooth: children of sum node #{} have different scopes".format(i))
            elif self.classes[i] == 'Product':
                merged = sum((self.scopes[c] for c in kids), [])
                if len(merged) != len(set(merged)) or sorted(merged) != scope:
                    raise ValueError(
                        "SPN is not decomposable: children of product node #{} don't have disjoint scopes".format(i))
        self._checked = True

    def device_arrays(self, device):
        """The flat arrays as tensors on ``device`` (uploaded once per device)."""
        import torch
        key = str(device)
        if key not in self._device:
            names = ('order', 'kind', 'arg0', 'arg1', 'arg2', 'par0', 'par1', 'child_index', 'child_weight',
                     'cat_value', 'cat_logp', 'node_slot', 'child_slot', 'sum_index', 'child_logw', 'raw0', 'raw1')
            self._device[key] = {k: torch.from_numpy(getattr(self, k)).to(device) for k in names}
            self._device[key]['cat_prob'] = torch.from_numpy(self.probabilities).to(device)
        return self._device[key]

    #: the arrays that hold parameters (host attribute -> device array): what refresh() pushes and pull() reads back
    _PARAMS = {'child_weight': 'child_weight', 'child_logw': 'child_logw', 'par0': 'par0', 'par1': 'par1',
               'raw0': 'raw0', 'raw1': 'raw1', 'probabilities': 'cat_prob', 'cat_logp': 'cat_logp'}

    def circuit(self, device):
        """The ``dpk_flat_spn_circuit`` record of this circuit's arrays on ``device`` (``n_slots`` as it is set on the
        object at the time of the call: 0 forces the workspace routes)."""
        from deeprob.hip import FlatSpnCircuit
        a = self.device_arrays(device)
        rec = FlatSpnCircuit(n_nodes=self.n_nodes, root=self.root, n_sum=self.n_sum, n_vars=self.n_features,
                             n_child=len(self.child_index), n_cat=len(self.cat_value), n_slots=self.n_slots,
                             max_children=self.max_children)
        for field in ('order', 'kind', 'arg0', 'arg1', 'arg2', 'sum_index', 'child_index', 'child_slot', 'node_slot',
                      'cat_value', 'child_weight', 'child_logw', 'cat_logp', 'par0', 'par1', 'raw0', 'raw1', 'cat_prob'):
            setattr(rec, field, a[field].data_ptr())
        return rec

    def _leaf_view(self, raw, *families):
        out = np.full(self.n_nodes, np.nan)
        keep = np.isin(self.kind, [KIND[f] for f in families])
        out[keep] = raw[keep]
        return out

    # per-node copies of the leaves' parameters, NaN where a node is of another family; to change parameters write
    # ``raw0`` / ``raw1`` / ``probabilities`` / ``child_weight`` and call refresh()
    p = property(lambda self: self._leaf_view(self.raw0, 'Bernoulli'))
    mean = property(lambda self: self._leaf_view(self.raw0, 'Gaussian'))
    stddev = property(lambda self: self._leaf_view(self.raw1, 'Gaussian'))
    start = property(lambda self: self._leaf_view(self.raw0, 'Uniform'))
    width = property(lambda self: self._leaf_view(self.raw1, 'Uniform'))

    def refresh(self):
        """Recompute the derived arrays (``par0`` / ``par1`` / ``cat_logp`` / ``child_logw``) from the parameters
        (``child_weight``, ``raw0`` / ``raw1``, ``probabilities``) and push all of them to every device that holds a
        copy of the circuit (in place: the device addresses stay)."""
        import torch
        bern = self.kind == KIND['Bernoulli']
        with np.errstate(divide='ignore'):
            pb = self.raw0[bern]
            self.par0[bern] = np.where(pb > 0.0, np.log(np.where(pb > 0.0, pb, 1.0)), -np.inf)
            self.par1[bern] = np.where(pb < 1.0, np.log1p(-np.where(pb < 1.0, pb, 0.0)), -np.inf)
            cont = (self.kind == KIND['Uniform']) | (self.kind == KIND['Gaussian'])
            self.par0[cont], self.par1[cont] = self.raw0[cont], self.raw1[cont]
            self.cat_logp[:] = np.log(self.probabilities).astype(np.float32)
            self.child_logw[:] = np.log(self.child_weight)
        for arrays in self._device.values():
            for host, dev in self._PARAMS.items():
                arrays[dev].copy_(torch.from_numpy(getattr(self, host)))

    def pull(self, device):
        """Read the parameters back from ``device`` (where ``expectation_maximization`` updated them), then
        refresh() every copy."""
        a = self.device_arrays(device)
        self.child_weight[:] = a['child_weight'].cpu().numpy()
        self.raw0[:] = a['raw0'].cpu().numpy()
        self.raw1[:] = a['raw1'].cpu().numpy()
        self.probabilities[:] = a['cat_prob'].cpu().numpy()
        self.refresh()

    def bfs_order(self) -> List[int]:
        """Breadth-first order from the root, children in position order, each node once (node.py:175-189)."""
        seen, queue, out = {self.root}, [self.root], []
        while queue:
            node = queue.pop(0)
            out.append(node)
            for c in self.children[node]:
                if c not in seen:
                    seen.add(c)
                    queue.append(c)
        return out

    def em_init(self, random_state):
        """Random parameters for EM, drawn as the reference draws them (em.py:66-74): every sum node in breadth-first
        order (node.py:91-98), then every leaf in the same order (leaf.py:164-165, 267-279, 532-534).

        :raises NotImplementedError: If the circuit has a Uniform leaf (leaf.py:463-464); nothing is modified then.
        """
        if (self.kind == KIND['Uniform']).any():
            raise NotImplementedError("EM parameters initialization not yet implemented for Uniform distributions")
        order = self.bfs_order()
        for i in order:
            if self.kind[i] == KIND['Sum']:
                c0, nc = int(self.arg0[i]), int(self.arg1[i])
                self.child_weight[c0:c0 + nc] = random_state.dirichlet(np.ones(nc)).astype(np.float32)
        for i in order:
            k = self.kind[i]
            if k == KIND['Bernoulli']:
                self.raw0[i] = random_state.rand()
            elif k == KIND['Categorical']:
                c0, nc = int(self.arg1[i]), int(self.arg2[i])
                self.probabilities[c0:c0 + nc] = random_state.dirichlet(np.ones(nc))
            elif k == KIND['Gaussian']:
                self.raw0[i] = 1e-1 * random_state.randn()
                self.raw1[i] = 0.5 + 1e-1 * np.tanh(random_state.randn())
        self.refresh()


def load_spn_json(f: Union[IO, os.PathLike, str], leaves: Optional[list] = None) -> FlatSpn:
    """
    Load SPN from file by using the JSON format (reference io.py:73-102).

    :param f: A file-like object or a filepath of the input JSON file.
    :param leaves: Custom leaf classes are not evaluated by the HIP path.
    :return: The loaded SPN, flattened.
    :raises ValueError: If a node class is unknown or the structure is not a valid labelled DAG.
    """
    if leaves:
        raise NotImplementedError("custom leaf classes are outside the HIP evaluator (Bernoulli, Categorical, "
                                  "Uniform and Gaussian leaves are built in)")
    if isinstance(f, (os.PathLike, str)):
        with open(f, 'r', encoding='utf-8') as file:
            data = json.load(file)
    else:
        data = json.load(f)
    return digraph_to_spn(data)


def digraph_to_spn(data: dict) -> FlatSpn:
    """Node-link data (networkx ``node_link_data``: ``nodes`` with ``id / class / scope / weights / params``, and
    ``links`` -- ``edges`` in newer networkx -- child -> parent with the child's position ``idx``; reference
    io.py:150-175, :178-219) to a :class:`FlatSpn`."""
    nodes = {int(n['id']): n for n in data['nodes']}
    slots: Dict[int, Dict[int, int]] = {i: {} for i in nodes}
    for e in data['links'] if 'links' in data else data['edges']:
        child, parent, idx = int(e['source']), int(e['target']), int(e['idx'])
        if child not in nodes or parent not in nodes:
            raise ValueError("Edge ({}, {}) refers to a missing node".format(child, parent))
        slots[parent][idx] = child
    children = {}
    for i, s in slots.items():
        if sorted(s) != list(range(len(s))):
            raise ValueError("Children positions of node {} are not 0..{}".format(i, len(s) - 1))
        children[i] = [s[k] for k in range(len(s))]
    return FlatSpn(nodes, children)


def spn_to_digraph(root: FlatSpn) -> dict:
    """The circuit as node-link data (what networkx ``node_link_data`` gives for the reference's graph, reference
    io.py:133-177): floats rounded to 8 decimals (io.py:150, 160-166), edges child -> parent with the position."""
    nodes, links = [], []
    for i in range(root.n_nodes):
        name, scope = root.classes[i], list(root._scope_as_given[i])
        if name == 'Sum':
            c0, nc = int(root.arg0[i]), int(root.arg1[i])
            attr = {'class': name, 'scope': scope, 'weights': [round(float(w), 8) for w in root.child_weight[c0:c0 + nc]]}
        elif name == 'Product':
            attr = {'class': name, 'scope': scope}
        else:
            if name == 'Bernoulli':
                params = {'p': round(float(root.raw0[i]), 8)}
            elif name == 'Categorical':
                c0, nc = int(root.arg1[i]), int(root.arg2[i])
                params = {'categories': [int(c) for c in root.cat_value[c0:c0 + nc]],
                          'probabilities': np.around(root.probabilities[c0:c0 + nc].astype(np.float64), 8).tolist()}
            elif name == 'Uniform':
                params = {'start': round(float(root.raw0[i]), 8), 'width': round(float(root.raw1[i]), 8)}
            else:
                params = {'mean': round(float(root.raw0[i]), 8), 'stddev': round(float(root.raw1[i]), 8)}
            attr = {'class': name, 'scope': scope, 'params': params}
        attr['id'] = i
        nodes.append(attr)
    for i in range(root.n_nodes):
        for k, c in enumerate(root.children[i]):
            links.append({'idx': k, 'source': int(c), 'target': i})
    return {'directed': True, 'multigraph': False, 'graph': {}, 'nodes': nodes, 'links': links}


def save_spn_json(root: FlatSpn, f: Union[IO, os.PathLike, str]):
    """
    Save SPN to file by using the JSON format (reference io.py:59-70); the reference and ``load_spn_json`` read it.

    :param root: The SPN.
    :param f: A file-like object or a filepath of the output JSON file.
    """
    json_obj = json.dumps(spn_to_digraph(root))
    if isinstance(f, (os.PathLike, str)):
        with open(f, 'w', encoding='utf-8') as file:
            file.write(json_obj)
    else:
        f.write(json_obj)
