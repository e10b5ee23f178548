"""The leaf learners of the reference (deeprob/spn/learning/leaf.py:40-186) on the HIP path.

``learn_spn`` recognises ``learn_binary_clt`` BY IDENTITY, as it recognises ``splitting.rdc.rdc_cols``: pass the function
itself as ``learn_leaf`` and every multivariate leaf task becomes a Chow-Liu tree, its co-occurrence counts taken for all
leaf tasks of a generation in one launch (``dpl_pair_ones``; learnspn.py, DESIGN.md "Chow-Liu tree leaves in learn_spn").
The string ``'binary-clt'``, every other callable and every wrapper around the function keep raising
``NotImplementedError`` there.

Called on their own the functions below learn ONE leaf from ``data`` ``[N, len(scope)]`` (a numpy array or a device
tensor; the statistics are counted on the HIP device) and return this package's model types: a
:class:`deeprob.spn.structure.io.FlatSpn` -- one leaf node, or a Product over the leaves of a naive factorisation -- or a
fitted :class:`deeprob.spn.structure.cltree.BinaryCLT`.
"""
from typing import List, Optional, Union

import numpy as np
import torch

from deeprob.spn.structure.leaf import Bernoulli
from deeprob.spn.structure.cltree import BinaryCLT

SHAPE_MESSAGE = "Each data column should correspond to a random variable having a distribution and a domain"
BERNOULLI_MESSAGE = "Binary Chow-Liu trees are only available for Bernoulli data"


def _mle_nodes(data, distributions, domains, scope, alpha):
    """The node record of the MLE leaf of every column: one upload, one statistics launch, one read."""
    from deeprob.spn.learning import learnspn as LS
    from deeprob.spn.learning.splitting import rdc as R
    if len(scope) != len(distributions) or len(domains) != len(distributions) or len(data.shape) != 2 \
            or data.shape[1] != len(scope):
        raise ValueError(SHAPE_MESSAGE)
    if R.all_gaussian(distributions):
        from deeprob.spn.learning.learnspn_cont import GaussianColumns
        kind = GaussianColumns(distributions, domains)
    else:
        kind = LS.DiscreteColumns(distributions, domains)
    kind.check_columns(None)
    if kind.smoothed_leaves and alpha < 0.0:
        raise ValueError("The Laplace smoothing factor must be non-negative")
    dev = kind.upload(data)
    n, m = dev.n_rows, dev.n_cols
    row_index = torch.arange(n, dtype=torch.int32, device=dev.device)
    stats, _ = kind.column_stats(row_index, list(range(m)), [0] * m, [n] * m)
    nodes = []
    for i, s in enumerate(scope):
        node = kind.leaf(i, stats[i], n, alpha)
        node['scope'] = [s]
        nodes.append(node)
    return nodes


def learn_mle(data, distributions: list, domains: List[Union[list, tuple]], scope: List[int], alpha: float = 0.1,
              random_state=None):
    """
    Learn a leaf using Maximum Likelihood Estimate (MLE) (reference leaf.py:40-73).
    If the data is multivariate, a naive factorized model is learned.

    :param data: The data, where each column correspond to a random variable.
    :param distributions: The distributions of the random variables.
    :param domains: The domains of the random variables.
    :param scope: The scope of the leaf.
    :param alpha: Laplace smoothing factor.
    :param random_state: Accepted for the reference's signature (nothing is drawn).
    :return: A FlatSpn: the leaf, or the Product of a naive factorisation.
    :raises ValueError: If there are inconsistencies between the data, distributions and domains.
    """
    if len(scope) == 1:
        from deeprob.spn.learning.learnspn import to_flat
        return to_flat(_mle_nodes(data, distributions, domains, scope, alpha)[0])
    return learn_naive_factorization(data, distributions, domains, scope, learn_mle, alpha=alpha, random_state=random_state)


def learn_binary_clt(data, distributions: list, domains: List[Union[list, tuple]], scope: List[int], to_pc: bool = False,
                     alpha: float = 0.1, random_state=None):
    """
    Learn a leaf using a Binary Chow-Liu Tree (CLT) (reference leaf.py:112-155).
    If the data is univariate, a Maximum Likelihood Estimate (MLE) leaf is returned.

    Passed to ``learn_spn`` as ``learn_leaf`` (the function itself) it is not called: ``learn_spn`` counts all leaf
    tasks of a generation in one launch and builds the same leaves (see the module docstring).

    :param data: The data: a numpy array or a device tensor, every value 0 or 1.
    :param distributions: The distributions of the random variables, ``Bernoulli`` each.
    :param domains: The domains of the random variables, ``[0, 1]`` each.
    :param scope: The scope of the leaf.
    :param to_pc: Whether to convert the CLT into an equivalent circuit (a FlatSpn).
    :param alpha: Laplace smoothing factor.
    :param random_state: None, a seed or a Numpy RandomState: draws the root of the tree.
    :return: A fitted BinaryCLT, or a FlatSpn (``to_pc=True``, or one column).
    :raises ValueError: If there are inconsistencies between the data, distributions and domains.
    :raises ValueError: If the data doesn't follow a Bernoulli distribution.
    """
    if len(scope) != len(distributions) or len(domains) != len(distributions):
        raise ValueError(SHAPE_MESSAGE)
    if any(d is not Bernoulli for d in distributions):
        raise ValueError(BERNOULLI_MESSAGE)
    if len(scope) == 1:
        return learn_mle(data, distributions, domains, scope, alpha=alpha, random_state=random_state)
    leaf = BinaryCLT(scope)
    leaf.fit(data, [list(d) for d in domains], alpha=alpha, random_state=random_state)
    if to_pc:
        return leaf.to_pc()
    return leaf


def learn_naive_factorization(data, distributions: list, domains: List[Union[list, tuple]], scope: List[int],
                              learn_leaf_func, **learn_leaf_kwargs):
    """
    Learn a leaf as a naive factorized model (reference leaf.py:158-186): a Product over one leaf per column.

    :param learn_leaf_func: ``learn_mle`` or ``learn_binary_clt``, by identity (on one column both are the MLE leaf);
                            any other function raises NotImplementedError.
    :param learn_leaf_kwargs: ``alpha``, ``random_state`` and, for ``learn_binary_clt``, ``to_pc``.
    :return: A FlatSpn whose root is the Product.
    :raises ValueError: If there are inconsistencies between the data, distributions and domains.
    """
    from deeprob.spn.learning.learnspn import new_node, to_flat
    if learn_leaf_func is not learn_mle and learn_leaf_func is not learn_binary_clt:
        raise NotImplementedError("a custom learn_leaf function is not built on the HIP path (built: learn_mle, "
                                  "learn_binary_clt)")
    allowed = ('alpha', 'random_state') + (('to_pc',) if learn_leaf_func is learn_binary_clt else ())
    for k in learn_leaf_kwargs:
        if k not in allowed:
            raise TypeError("{} got an unexpected keyword argument '{}'".format(learn_leaf_func.__name__, k))
    if len(scope) != len(distributions) or len(domains) != len(distributions):
        raise ValueError(SHAPE_MESSAGE)
    if learn_leaf_func is learn_binary_clt and any(d is not Bernoulli for d in distributions):
        raise ValueError(BERNOULLI_MESSAGE)
    node = new_node('Product', scope)
    node['children'] = _mle_nodes(data, distributions, domains, scope, float(learn_leaf_kwargs.get('alpha', 0.1)))
    return to_flat(node)
