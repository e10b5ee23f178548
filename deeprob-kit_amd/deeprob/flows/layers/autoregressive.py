"""Autoregressive (MADE) layer of the masked autoregressive flow behind the reference interface
(deeprob/flows/layers/autoregressive.py:13-181), evaluated by the HIP kernels of csrc/maf.hip through
deeprob/hip/ops_maf.py: a fused density kernel, a one-launch sampling kernel, and the chained masked-GEMM route
(training, rsample, and whatever lies outside the two kernels' envelopes)."""
from typing import Optional, Tuple, List

import numpy as np
import torch
from torch import nn

from deeprob.flows.utils import Bijector
from deeprob.torch.utils import ScaledTanh, MaskedLinear, get_activation_class
from deeprob.hip import Workspace


class AutoregressiveLayer(Bijector):
    def __init__(self, in_features: int, depth: int, units: int, activation: str, reverse: bool = False,
                 sequential: bool = True, random_state: Optional[np.random.RandomState] = None):
        """
        :param in_features: number of variables D.
        :param depth: hidden layers of the conditioner.
        :param units: units per hidden layer.
        :param activation: activation between the conditioner's layers ('relu', 'leaky-relu', 'softplus', 'tanh',
                           'sigmoid').
        :param reverse: reverse the input degrees (sequential degrees only).
        :param sequential: sequential degrees; otherwise random degrees drawn from `random_state`.
        :param random_state: a np.random.RandomState (required when sequential is False).
        :raises ValueError: if a parameter is out of domain.
        """
        if depth <= 0:
            raise ValueError("The depth value must be positive")
        if units <= 0:
            raise ValueError("The units value must be positive")
        if not sequential and not isinstance(random_state, np.random.RandomState):
            raise ValueError("A Numpy RandomState is required if sequential is False")
        activation_cls = get_activation_class(activation)

        super().__init__(in_features)
        self.layers = nn.ModuleList()
        self.scale_act = ScaledTanh()

        if sequential:
            degrees = self.build_degrees_sequential(depth, units, reverse)
        else:
            degrees = self.build_degrees_random(depth, units, random_state)
        masks = self.build_masks(degrees)

        # the input ordering: variables are produced in the order of increasing input degree
        self.ordering = degrees[0]
        self.inv_ordering = np.argsort(self.ordering)

        # conditioner: MaskedLinear -> activation -> ... -> MaskedLinear(units, 2D) with the output mask tiled twice
        stack, width = [], in_features
        for mask in masks[:-1]:
            stack.extend([MaskedLinear(width, units, mask), activation_cls()])
            width = units
        stack.append(MaskedLinear(width, self.in_features * 2, np.tile(masks[-1], reps=(2, 1))))
        self.network = nn.Sequential(*stack)
        self._ws = Workspace()
        self._ws_sample = Workspace()
        self._orders = None

    def apply_backward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """u = (x - t) exp(-s), ildj = -sum(s) with (t, s) = network(x), s = ScaledTanh(s) (reference :72-79)."""
        from deeprob.hip import ops_maf
        return ops_maf.autoregressive_backward(x, self)

    def apply_forward(self, u: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """x_i = u_i exp(s_i) + t_i, produced one variable at a time in the order of inv_ordering (reference :81-121)."""
        from deeprob.hip import ops_maf
        return ops_maf.autoregressive_forward(u, self)

    def build_degrees_sequential(self, depth: int, units: int, reverse: bool) -> List[np.ndarray]:
        """Input degrees 0..D-1 (or D-1..0 when reversed), hidden degrees arange(units) % (D - 1) (reference :123-142)."""
        degrees = []
        if reverse:
            degrees.append(np.arange(self.in_features - 1, -1, -1))
        else:
            degrees.append(np.arange(self.in_features))
        for _ in range(depth):
            degrees.append(np.arange(units) % (self.in_features - 1))
        return degrees

    def build_degrees_random(self, depth: int, units: int, random_state: np.random.RandomState) -> List[np.ndarray]:
        """A shuffled input ordering, then per hidden layer degrees drawn in [min previous degree, D - 1)
        (reference :144-162; the same draws from random_state, in the same order)."""
        degrees = []
        ordering = np.arange(self.in_features)
        random_state.shuffle(ordering)
        degrees.append(ordering)
        for _ in range(depth):
            min_prev_degree = np.min(degrees[-1])
            degrees.append(random_state.randint(min_prev_degree, self.in_features - 1, units))
        return degrees

    @staticmethod
    def build_masks(degrees: List[np.ndarray]) -> List[np.ndarray]:
        """mask[j, i] = d_prev[i] <= d_next[j] between hidden layers, d_last[j] < d_in[i] for the output layer
        (reference :164-181)."""
        masks = []
        for (d1, d2) in zip(degrees[:-1], degrees[1:]):
            masks.append(np.less_equal(np.expand_dims(d1, axis=0), np.expand_dims(d2, axis=1)))
        masks.append(np.less(np.expand_dims(degrees[-1], axis=0), np.expand_dims(degrees[0], axis=1)))
        return masks
