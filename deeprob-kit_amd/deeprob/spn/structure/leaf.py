"""The leaf distribution classes of the reference (deeprob/spn/structure/leaf.py:14-20, 126, 210, 441, 506) as MARKERS:
what a caller passes in ``distributions`` to ``learn_spn`` / ``learn_estimator`` / ``learn_classifier``.  They carry
``LEAF_TYPE`` and the class name that ``FlatSpn`` and the JSON format use; they are tokens, not evaluators -- the HIP
evaluator works on the flat arrays of :class:`deeprob.spn.structure.io.FlatSpn`.
"""
from enum import Enum


class LeafType(Enum):
    """The type of the distribution leaf: discrete or continuous."""
    DISCRETE = 1
    CONTINUOUS = 2


class Leaf:
    LEAF_TYPE = None


class Bernoulli(Leaf):
    LEAF_TYPE = LeafType.DISCRETE


class Categorical(Leaf):
    LEAF_TYPE = LeafType.DISCRETE


class Uniform(Leaf):
    LEAF_TYPE = LeafType.CONTINUOUS


class Gaussian(Leaf):
    LEAF_TYPE = LeafType.CONTINUOUS
