"""The learning wrappers of the reference (deeprob/spn/learning/wrappers.py) on the HIP path: they return a
:class:`deeprob.spn.structure.io.FlatSpn`."""
from typing import List, Optional, Union

import numpy as np

from deeprob.spn.structure.leaf import LeafType
from deeprob.spn.learning.learnspn import learn_spn, new_node, to_flat
from deeprob.spn.algorithms.structure import prune, prune_nodes, flat_to_nodes


def _host(data) -> np.ndarray:
    """The data on the host (domains and class values are found there); a CPU tensor is an error as everywhere."""
    if isinstance(data, np.ndarray):
        return data
    from deeprob.hip import HipError
    if not getattr(data, 'is_cuda', False):
        raise HipError("data lives on '{}': the deeprob HIP path only works on tensors on a HIP device (there is no CPU "
                       "fallback); pass a numpy array or a device tensor".format(getattr(data, 'device', type(data))))
    return data.cpu().numpy()


#: the arguments of the XPC learners that have no default: ``learn_estimator`` routes to them when all are given
XPC_KEYWORDS = {'xpc': ('det', 'sd', 'min_part_inst', 'conj_len', 'arity'),
                'ensemble-xpc': ('ensemble_dim', 'det', 'sd_level', 'min_part_inst', 'conj_len', 'arity')}


def learn_estimator(data, distributions: list, domains: Optional[List[Union[list, tuple]]] = None, method: str = 'learnspn',
                    **kwargs):
    """
    Learn a SPN density estimator given some training data, the features distributions and domains
    (reference wrappers.py:15-52): ``learn_spn`` followed by ``prune``, or ``learn_xpc`` / ``learn_expc``.

    :param method: 'learnspn', 'xpc' or 'ensemble-xpc'.  The XPC learners have required arguments without defaults
                   (``det``, ``sd`` -- ``sd_level`` and ``ensemble_dim`` for the ensemble --, ``min_part_inst``,
                   ``conj_len``, ``arity``): they are given as keywords.
    :raises ValueError: If the method used for structure learning is not known.
    :raises ValueError: If the method is 'xpc' or 'ensemble-xpc' but the variable domains are not binary.
    :raises NotImplementedError: For 'xpc' and 'ensemble-xpc' without their required keywords.
    """
    if method in XPC_KEYWORDS:
        if domains is None:
            domains = compute_data_domains(_host(data), distributions)
        if not all(d == [0, 1] for d in domains):
            raise ValueError("The domains must be binary for learning {}".format(
                'a XPC' if method == 'xpc' else 'an Ensemble-XPC'))
        missing = [k for k in XPC_KEYWORDS[method] if k not in kwargs]
        if missing:
            raise NotImplementedError("structure learning method '{}' has no defaults for {}: pass them as "
                                      "keywords".format(method, ', '.join(missing)))
        from deeprob.spn.learning.xpc import learn_expc, learn_xpc
        root, _ = (learn_xpc if method == 'xpc' else learn_expc)(data, **kwargs)
        return root
    if method != 'learnspn':
        raise ValueError("Unknown SPN learning method called {}".format(method))
    if domains is None:
        domains = compute_data_domains(_host(data), distributions)
    return prune(learn_spn(data, distributions, domains, **kwargs), copy=False)


def learn_classifier(data, distributions: list, domains: Optional[List[Union[list, tuple]]] = None, class_idx: int = -1,
                     verbose: bool = True, **kwargs):
    """
    Learn a SPN classifier (reference wrappers.py:55-99): one ``learn_spn`` per class value on the rows of that class,
    pruned, under a Sum weighted by the class frequencies.
    """
    host = _host(data)
    if domains is None:
        domains = compute_data_domains(host, distributions)
    n_samples = host.shape[0]
    classes = host[:, class_idx]
    weights, children = [], []
    for c in np.unique(classes):
        rows = classes == c
        local = host[rows] if isinstance(data, np.ndarray) else data[np.flatnonzero(rows)]
        branch = learn_spn(local, distributions, domains, verbose=verbose, **kwargs)
        weights.append(int(rows.sum()) / n_samples)
        children.append(prune_nodes(flat_to_nodes(branch)[branch.root]))
    root = new_node('Sum', children[0]['scope'], weights=weights)
    root['children'] = children
    return to_flat(root)


def compute_data_domains(data: np.ndarray, distributions: list) -> List[Union[list, tuple]]:
    """
    Compute the domains based on the training data and the features distributions (reference wrappers.py:102-124).

    :raises ValueError: If an unknown distribution type is found.
    """
    domains = []
    for i, d in enumerate(distributions):
        col = data[:, i]
        if d.LEAF_TYPE == LeafType.DISCRETE:
            domains.append(np.unique(col).tolist())
        elif d.LEAF_TYPE == LeafType.CONTINUOUS:
            domains.append((np.min(col).item(), np.max(col).item()))
        else:
            raise ValueError("Unknown distribution type {}".format(d.LEAF_TYPE))
    return domains
