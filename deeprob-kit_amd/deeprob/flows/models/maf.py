"""Masked Autoregressive Flow behind the reference interface (deeprob/flows/models/maf.py:12-78)."""
from typing import Optional, Tuple

import torch

from deeprob.torch.base import DensityEstimator
from deeprob.utils.random import check_random_state, RandomState
from deeprob.flows.utils import BatchNormLayer1d
from deeprob.flows.layers.autoregressive import AutoregressiveLayer
from deeprob.flows.models.base import NormalizingFlow


class MAF(NormalizingFlow):
    def __init__(self, in_features: int, dequantize: bool = False, logit: Optional[float] = None,
                 in_base: Optional[DensityEstimator] = None, n_flows: int = 5, depth: int = 1, units: int = 128,
                 batch_norm: bool = True, activation: str = 'relu', sequential: bool = True,
                 random_state: Optional[RandomState] = None):
        """
        :param in_features: number of input features.
        :param dequantize: prepend the dequantisation transformation.
        :param logit: logit factor, None to disable the logit transformation.
        :param in_base: base density (None = standard Normal).
        :param n_flows: number of autoregressive layers.
        :param depth: hidden layers of every conditioner.
        :param units: units per hidden layer of every conditioner.
        :param batch_norm: a BatchNormLayer1d after every autoregressive layer.
        :param activation: activation of the conditioners' hidden layers.
        :param sequential: sequential degrees; otherwise random degrees.
        :param random_state: seed or np.random.RandomState of the random degrees (sequential=False only).
        :raises ValueError: if a parameter is out of domain.
        """
        if n_flows <= 0:
            raise ValueError("The number of autoregressive flow layers must be positive")
        if depth <= 0:
            raise ValueError("The number of hidden layers of conditioners must be positive")
        if units <= 0:
            raise ValueError("The number of hidden units per layer must be positive")

        super().__init__(in_features, dequantize=dequantize, logit=logit, in_base=in_base)
        self.n_flows = n_flows
        self.depth = depth
        self.units = units
        self.batch_norm = batch_norm
        self.activation = activation
        self.sequential = sequential

        if not self.sequential:
            random_state = check_random_state(random_state)

        # [AutoregressiveLayer, BatchNormLayer1d] x n_flows, the input ordering reversed from one layer to the next
        reverse = False
        for _ in range(self.n_flows):
            self.layers.append(AutoregressiveLayer(self.in_features, self.depth, self.units, self.activation,
                                                   reverse=reverse, sequential=self.sequential,
                                                   random_state=random_state))
            if self.batch_norm:
                self.layers.append(BatchNormLayer1d(self.in_features))
            reverse = not reverse

    def apply_backward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """data -> latent (reference: flows/models/base.py:182-193).  In eval mode without an autograd graph the batch
        norms are folded into the fused kernels of the autoregressive layers behind them (deeprob/hip/ops_maf.py)."""
        if self.training or not x.is_cuda or x.dim() != 2 or \
                (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))):
            return super().apply_backward(x)
        from deeprob.hip import ops_maf
        return ops_maf.flow_density(self, x)
