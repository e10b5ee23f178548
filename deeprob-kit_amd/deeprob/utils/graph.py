"""Trees over variables, as the reference's ``deeprob/utils/graph.py`` names them: ``TreeNode``,
``build_tree_structure``, ``compute_bfs_ordering`` and ``maximum_spanning_tree``.

A tree is a sequence of predecessors: ``tree[i]`` is the parent of ``i`` and the root has -1.

The package does not import scipy.  ``maximum_spanning_tree`` is Prim's algorithm in numpy over the dense matrix (the
reference runs scipy's Kruskal, graph.py:169-185): when the maximum spanning tree is unique -- no two of the weights that
decide it are equal -- both give the same edges and therefore the same ``tree``.  The ``bfs`` returned with it is THIS
project's order: breadth first from the root, the children of a node in increasing index.  scipy's
``breadth_first_order`` visits the neighbours of a node in the order its sparse matrix stores them, which is another
order; ``bfs`` only fixes the order in which float32 messages are added ("Chow-Liu trees"), no result
depends on it beyond rounding.
"""
from collections import deque
from typing import List, Optional, Tuple, Union

import numpy as np


class TreeNode:
    """A node of a rooted tree: an id, a parent and the children in the order they were attached."""

    def __init__(self, node_id: int, parent: 'TreeNode' = None):
        self.id = node_id
        self._parent = None
        self._children = []
        self.set_parent(parent)

    def get_id(self) -> int:
        return self.id

    def get_parent(self) -> 'TreeNode':
        """The parent, None at the root."""
        return self._parent

    def get_children(self) -> List['TreeNode']:
        return self._children

    def set_parent(self, parent: 'TreeNode'):
        """Attach this node under ``parent`` (once: a node that has a parent keeps it)."""
        if parent is None or self._parent is not None:
            return
        self._parent = parent
        parent._children.append(self)

    def is_leaf(self) -> bool:
        return not self._children

    def _breadth_first(self):
        queue = deque([self])
        while queue:
            node = queue.popleft()
            queue.extend(node._children)
            yield node

    def get_n_nodes(self) -> int:
        """The number of nodes of the tree rooted here."""
        return sum(1 for _ in self._breadth_first())

    def get_tree_scope(self) -> Tuple[list, list]:
        """``(tree, scope)`` of the tree rooted here: the ids breadth first, and the predecessors as positions in that
        list (-1 for this node)."""
        nodes = list(self._breadth_first())
        scope = [n.id for n in nodes]
        position = {n.id: p for p, n in enumerate(nodes)}
        tree = [-1 if n is self else position[n._parent.id] for n in nodes]
        return tree, scope


def build_tree_structure(tree: Union[List[int], np.ndarray], scope: Optional[List[int]] = None) -> TreeNode:
    """
    The ``TreeNode`` structure of a sequence of predecessors; returns its root.

    :param tree: The predecessors, -1 at the root.
    :param scope: Optional node ids, one per position.
    :raises ValueError: If there is not exactly one root, the scope has duplicates or another length.
    """
    tree = [int(t) for t in tree]
    if tree.count(-1) != 1:
        raise ValueError("Invalid tree structure")
    if scope is None:
        ids = list(range(len(tree)))
    else:
        ids = list(scope)
        if len(set(ids)) != len(ids):
            raise ValueError("The scope must not contain duplicates")
        if len(ids) != len(tree):
            raise ValueError("Invalid scope's number of variables")
    nodes = [TreeNode(i) for i in ids]
    for position, pred in enumerate(tree):      # in increasing position: the children of a node come out ascending
        if pred != -1:
            nodes[position].set_parent(nodes[pred])
    return nodes[tree.index(-1)]


def compute_bfs_ordering(tree: Union[List[int], np.ndarray]) -> Union[List[int], np.ndarray]:
    """The breadth-first order of a sequence of predecessors: from the root, children in increasing index.  A list
    for a list, an array of the same dtype for an array."""
    order = [n.get_id() for n in build_tree_structure(tree)._breadth_first()]
    return order if isinstance(tree, list) else np.array(order, dtype=tree.dtype)


def maximum_spanning_tree(root: int, adj_matrix: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """
    The maximum spanning tree of the complete graph with the symmetric weights ``adj_matrix``, rooted at ``root``.

    :return: ``(bfs, tree)`` int32: this project's breadth-first order (see the module docstring) and the
             predecessors, ``tree[root] = -1``.
    """
    w = np.asarray(adj_matrix)
    n = w.shape[0]
    if w.shape != (n, n) or not 0 <= int(root) < n:
        raise ValueError("expected a square matrix and a root inside it")
    tree = np.full(n, -1, np.int32)
    outside = np.ones(n, bool)
    outside[root] = False
    best = w[root].copy()                   # best[v]: the heaviest edge from v to the tree so far ...
    link = np.full(n, root, np.int32)       # ... and the tree node it ends at
    for _ in range(n - 1):
        v = int(np.flatnonzero(outside)[np.argmax(best[outside])])
        tree[v] = link[v]
        outside[v] = False
        better = outside & (w[v] > best)
        best[better] = w[v][better]
        link[better] = v
    return compute_bfs_ordering(tree), tree
