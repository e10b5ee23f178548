"""DGC-SPN model behind the reference interface (deeprob/spn/models/dgcspn.py)."""
from typing import Optional, Union, Tuple, List

import numpy as np
import torch
from torch import autograd

from deeprob.torch.base import ProbabilisticModel
from deeprob.torch.constraints import ScaleClipper
from deeprob.spn.layers.dgcspn import SpatialGaussianLayer, SpatialProductLayer, SpatialSumLayer, SpatialRootLayer


class DgcSpn(ProbabilisticModel):
    def __init__(
        self,
        in_features: Tuple[int, int, int],
        out_classes: int = 1,
        n_batch: int = 8,
        sum_channels: int = 8,
        depthwise: Union[bool, List[bool]] = False,
        n_pooling: int = 0,
        optimize_scale: bool = False,
        in_dropout: Optional[float] = None,
        sum_dropout: Optional[float] = None,
        quantiles_loc: Optional[np.ndarray] = None,
        uniform_loc: Optional[Tuple[float, float]] = None
    ):
        """
        Deep generalized convolutional SPN (constructor contract of the reference, dgcspn.py:16-131).

        :raises ValueError: if a parameter is out of domain.
        """
        if in_features[1] != in_features[2]:
            raise ValueError("The height and width of input size must be the same")
        if out_classes <= 0:
            raise ValueError("The number of output classes must be positive")
        if n_batch <= 0:
            raise ValueError("The number of base distribution batches must be positive")
        if sum_channels <= 0:
            raise ValueError("The number of output channels of spatial sum layers must be positive")
        if in_dropout is not None and not 0.0 < in_dropout < 1.0:
            raise ValueError("The dropout rate at base distribution must be in (0, 1)")
        if sum_dropout is not None and not 0.0 < sum_dropout < 1.0:
            raise ValueError("The dropout rate at spatial sum layers must be in (0, 1)")
        if quantiles_loc is not None and uniform_loc is not None:
            raise ValueError("At least one between quantiles_loc and uniform_loc must be None")
        if quantiles_loc is not None and len(quantiles_loc.shape) != 4:
            raise ValueError("The mean quantiles must be a 4D Numpy array")
        if uniform_loc is not None and (len(uniform_loc) != 2 or uniform_loc[0] >= uniform_loc[1]):
            raise ValueError("The uniform range must be a pair (A, B) with A < B")

        depth = int(np.ceil(np.log2(in_features[1])))
        if isinstance(depthwise, bool):
            depthwise = [depthwise] * (depth + 1)
        else:
            if len(depthwise) == 0 or len(depthwise) > depth + 1:
                raise ValueError("The length of depthwise argument must be in [1, ceil(log2(D)) + 1]")
            depthwise = list(depthwise) + [depthwise[-1]] * (depth + 1 - len(depthwise))
        if n_pooling < 0 or n_pooling > depth:
            raise ValueError("The number of initial pooling spatial product layers must be in [0, ceil(log2(D))]")

        super().__init__()
        self.in_features = in_features
        self.out_classes = out_classes
        self.n_batch = n_batch
        self.sum_channels = sum_channels
        self.depthwise = depthwise
        self.n_pooling = n_pooling
        self.optimize_scale = optimize_scale
        self.in_dropout = in_dropout
        self.sum_dropout = sum_dropout
        self.layers = torch.nn.ModuleList()

        self.base_layer = SpatialGaussianLayer(
            self.in_features, self.n_batch, optimize_scale=self.optimize_scale, dropout=self.in_dropout,
            quantiles_loc=quantiles_loc, uniform_loc=uniform_loc
        )
        shape = self.base_layer.out_features

        # level i: pooling product (valid, stride 2) for i < n_pooling, else dilated product with
        # 'full' padding ('final' at the last level); every product but the last feeds a sum layer
        for i in range(depth + 1):
            if i < self.n_pooling:
                padding, stride, dilation = 'valid', (2, 2), (1, 1)
            else:
                padding = 'final' if i == depth else 'full'
                stride = (1, 1)
                dilation = (2 ** (i - self.n_pooling),) * 2
            prod = SpatialProductLayer(shape, kernel_size=(2, 2), padding=padding, stride=stride,
                                       dilation=dilation, depthwise=self.depthwise[i])
            self.layers.append(prod)
            shape = prod.out_features
            if i != depth:
                ssum = SpatialSumLayer(shape, self.sum_channels, self.sum_dropout)
                self.layers.append(ssum)
                shape = ssum.out_features
        self.root_layer = SpatialRootLayer(shape, self.out_classes)
        if self.optimize_scale:
            self.scale_clipper = ScaleClipper()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """Log-likelihood ``[B, out_classes]`` of images ``x [B,C,H,W]``, NaN = marginalised
        (reference: dgcspn.py:134-151)."""
        if self._needs_graph(x):
            # training / gradients: the layer chain, with every depthwise product + sum pair of at most 8 channels as
            # one autograd node (no product map is written or kept; its backward recomputes it from the taps)
            from deeprob.hip import ops_spatial
            x = self.base_layer(x)
            i, n = 0, len(self.layers)
            while i < n:
                layer = self.layers[i]
                if (i + 1 < n and isinstance(layer, SpatialProductLayer) and isinstance(self.layers[i + 1], SpatialSumLayer)
                        and not (self.training and self.layers[i + 1].dropout is not None)):
                    y = ops_spatial.spatial_prodsum_autograd(x, layer, self.layers[i + 1].weight, self.layers[i + 1]._ws)
                    if y is not None:
                        x, i = y, i + 2
                        continue
                x = layer(x)
                i += 1
            return self.root_layer(x)
        # evaluation: every depthwise product is folded into the sum layer above it
        from deeprob.hip import ops_spatial
        # (the tables of every fused level rebuilt by one launch for the whole forward instead of one per level)
        ops_spatial.tables_prepare(self._fused_levels(), x)
        try:
            return self._forward_eval(x)
        finally:
            ops_spatial.tables_release()

    def _fused_levels(self):
        """The (product, sum) levels the evaluation loop below hands to spatial_prodsum / spatial_sumprodroot, in order."""
        levels, i, n = [], 0, len(self.layers)
        while i < n:
            layer = self.layers[i]
            nxt = self.layers[i + 1] if i + 1 < n else None
            if not (isinstance(layer, SpatialProductLayer) and isinstance(nxt, SpatialSumLayer)) or \
                    (self.training and nxt.dropout is not None):
                i += 1
                continue
            if i == n - 3 and isinstance(self.layers[i + 2], SpatialProductLayer):
                levels.append(('sumprodroot', layer, nxt, self.layers[i + 2], self.root_layer))
                break
            levels.append(('prodsum', layer, nxt))
            i += 2
        return levels

    def _forward_eval(self, x: torch.Tensor) -> torch.Tensor:
        from deeprob.hip import ops_spatial
        i, n = 0, len(self.layers)
        y = None
        if (n >= 4 and isinstance(self.base_layer, SpatialGaussianLayer) and isinstance(self.layers[0], SpatialProductLayer)
                and isinstance(self.layers[1], SpatialSumLayer) and not self.training):
            # the Gaussian leaf layer folded into the first (pooling) level: the leaf map is never written
            y = ops_spatial.spatial_leaf_prodsum(x, self.base_layer, self.layers[0], self.layers[1].weight, self.layers[1]._ws,
                                                 out_pixel_major=self._level_streams(2, x.shape[0]))
        if y is not None:
            x, i = y, 2
        else:
            x = self.base_layer(x)
        while i < n:
            layer = self.layers[i]
            if (i == n - 3 and isinstance(layer, SpatialProductLayer) and isinstance(self.layers[i + 1], SpatialSumLayer)
                    and isinstance(self.layers[i + 2], SpatialProductLayer)
                    and not (self.training and self.layers[i + 1].dropout is not None)):
                # last sum level + last product + root: the largest map stays on chip
                y = ops_spatial.spatial_sumprodroot(x, layer, self.layers[i + 1].weight, self.layers[i + 2],
                                                    self.root_layer.weight, self.root_layer._ws3)
                if y is not None:
                    return y
            if i + 1 < n and isinstance(layer, SpatialProductLayer) and isinstance(self.layers[i + 1], SpatialSumLayer):
                nxt = self.layers[i + 1]
                dropout = self.training and nxt.dropout is not None   # the sum layer raises: not on this path
                # (the map between two streaming levels stays pixel-major: csrc/dgcspn_stream.hip, round 6)
                y = None if dropout else ops_spatial.spatial_prodsum(x, layer, nxt.weight, nxt._ws,
                                                                     out_pixel_major=self._level_streams(i + 2, x.shape[0]))
                if y is not None:
                    x, i = y, i + 2
                    continue
            if i == n - 1 and isinstance(layer, SpatialProductLayer):
                # the last product feeds the root sum nodes directly
                y = ops_spatial.spatial_prodroot(x, layer, self.root_layer.weight, self.root_layer._ws2)
                if y is not None:
                    return y
            x = layer(x)
            i += 1
        return self.root_layer(x)

    def _level_streams(self, i: int, B: int) -> bool:
        """Whether the fused level that starts at layer ``i`` of the evaluation loop runs on the streaming route (the
        library's answer): its input may then arrive pixel-major."""
        from deeprob.hip import ops_spatial
        n = len(self.layers)
        if i + 1 >= n or self.training:
            return False
        layer, nxt = self.layers[i], self.layers[i + 1]
        if not (isinstance(layer, SpatialProductLayer) and isinstance(nxt, SpatialSumLayer)):
            return False
        if i == n - 3 and isinstance(self.layers[i + 2], SpatialProductLayer):
            return ops_spatial.level_streams(layer, B, nxt.weight.shape[0], self.layers[i + 2], self.root_layer.weight.shape[0])
        return ops_spatial.level_streams(layer, B, nxt.weight.shape[0])

    def _needs_graph(self, x: torch.Tensor) -> bool:
        if not torch.is_grad_enabled():
            return False
        return x.requires_grad or any(p.requires_grad for p in self.parameters())

    def mpe(self, x: torch.Tensor) -> torch.Tensor:
        """Gradient-based MPE completion of NaN pixels (reference: dgcspn.py:153-184)."""
        z = self.base_layer(x)
        if not z.requires_grad:
            z.requires_grad = True
        y = z
        for layer in self.layers:
            y = layer(y)
        y = self.root_layer(y)
        z_grad, = autograd.grad(y, z, grad_outputs=torch.ones_like(y), only_inputs=True)
        with torch.no_grad():
            estimates = torch.sum(torch.unsqueeze(z_grad, dim=2) * self.base_layer.loc, dim=1)
            return torch.where(torch.isnan(x), estimates, x)

    # ---- top-down pass: one launch (csrc/dgc/dgcspn_topdown.hip) -----------------------------------------------------------
    def _product_layers(self):
        return [layer for layer in self.layers if isinstance(layer, SpatialProductLayer)]

    def _topdown_logw(self):
        """log_softmax of every sum layer's weight (bottom to top) and of the root's, formed by the same torch call as the
        forward forms them (layers/dgcspn.py: SpatialSumLayer / SpatialRootLayer)."""
        out = [torch.log_softmax(layer.weight, dim=1) for layer in self.layers if isinstance(layer, SpatialSumLayer)]
        out.append(torch.log_softmax(self.root_layer.weight, dim=1))
        return out

    def _upward_for_sampling(self, x: torch.Tensor):
        """The leaf map and every sum layer's output, NCHW (no product map is kept): the fused product + sum level where it
        applies, else the two layers."""
        from deeprob.hip import ops_spatial
        h = self.base_layer(x)
        acts = [h]
        for i in range(0, len(self.layers) - 1, 2):
            prod, ssum = self.layers[i], self.layers[i + 1]
            y = ops_spatial.spatial_prodsum(h, prod, ssum.weight, ssum._ws, out_pixel_major=False)
            if y is None:
                y = ssum(prod(h))
            h = y
            acts.append(h)
        return acts

    def _check_topdown(self, what: str):
        from deeprob.hip import HipError
        if self.training and (self.in_dropout is not None or self.sum_dropout is not None):
            raise NotImplementedError('{}: training mode with in_dropout / sum_dropout set (call eval() first: the '
                                      'distribution is that of the model without dropout)'.format(what))
        device = self.root_layer.weight.device
        if device.type != 'cuda':
            raise HipError("{}: the model lives on '{}': the deeprob HIP path only samples on a HIP device (there is no "
                           "CPU fallback)".format(what, device))
        return device

    @torch.no_grad()
    def sample(self, n_samples: int, y: Optional[torch.Tensor] = None, seed: Optional[int] = None) -> torch.Tensor:
        """``[n_samples, C, H, W]`` ancestral samples, top-down in one launch (the reference raises here:
        dgcspn.py ``sample``).  ``y``: the class of every sample (drawn with ``torch.randint`` when missing, ignored by a
        model with one root; a label outside ``[0, out_classes)`` raises ``ValueError``).  The draws come from the library's
        counter-based hash (``seed``: fix them, e.g. to replay a batch).  A pixel outside every scope -- the last row and column of an odd map under a pooling level -- is NaN."""
        from deeprob.hip import dgc, ops
        device = self._check_topdown('sample')
        drawn = y is None
        if self.out_classes == 1:
            y = None
        elif y is None:
            y = torch.randint(self.out_classes, [n_samples], device=device)
        geom = dgc.product_geometry(self._product_layers())
        return dgc.dgcspn_topdown(dgc.DPG_MODE_PRIOR, n_samples, self.in_features, geom, self.out_classes, None, y, None,
                                  self._topdown_logw(), self.base_layer.loc, self.base_layer.scale,
                                  ops.draw_seed() if seed is None else int(seed), labels_trusted=drawn)

    @torch.no_grad()
    def sample_conditional(self, x: torch.Tensor, y: Optional[torch.Tensor] = None, seed: Optional[int] = None) -> torch.Tensor:
        """One exact draw from p(x_missing | x_observed, y) per row: the NaN entries of ``x [B,C,H,W]`` are drawn, the observed
        ones are returned as they are (the reference has no counterpart; ``mpe`` returns posterior means).  The bottom-up
        pass -- leaf map and every sum layer's output -- then one top-down launch that draws every sum node's input in
        proportion to weight * value of the input under the evidence.  Without labels the class of a row is drawn from
        softmax(root outputs) by ``torch.multinomial`` (rows whose evidence is impossible under every class take it
        uniformly; a given label outside ``[0, out_classes)`` raises ``ValueError``); ``seed`` fixes the kernel's counter-based
        draws: a row's draws depend on (seed, row index) and its evidence only.  A pixel outside every scope is returned as given."""
        from deeprob.hip import dgc, ops, ops_spatial
        device = self._check_topdown('sample_conditional')
        x = ops.require_device_f32(x, 'x')
        if x.dim() != 4 or tuple(x.shape[1:]) != tuple(self.in_features):
            raise ValueError("expected inputs [B, {}], got {}".format(tuple(self.in_features), tuple(x.shape)))
        acts = self._upward_for_sampling(x)
        drawn = y is None
        if self.out_classes == 1 or x.shape[0] == 0:
            y = None
        elif y is None:
            top = ops_spatial.spatial_prodroot(acts[-1], self.layers[-1], self.root_layer.weight, self.root_layer._ws2)
            if top is None:
                top = self.root_layer(self.layers[-1](acts[-1]))
            post = torch.softmax(top, dim=1)
            # (evidence impossible under every class: softmax gives NaN; such a row takes its class uniformly)
            post = torch.where(torch.isfinite(post).all(dim=1, keepdim=True), post, torch.full_like(post, 1.0 / self.out_classes))
            y = torch.multinomial(post, 1).squeeze(1)
        geom = dgc.product_geometry(self._product_layers())
        return dgc.dgcspn_topdown(dgc.DPG_MODE_POSTERIOR, x.shape[0], self.in_features, geom, self.out_classes, x, y, acts,
                                  self._topdown_logw(), self.base_layer.loc, self.base_layer.scale,
                                  ops.draw_seed() if seed is None else int(seed), labels_trusted=drawn)

    @torch.no_grad()
    def mpe_completion(self, x: torch.Tensor, y: Optional[torch.Tensor] = None, return_choice: bool = False):
        """The NaN entries of ``x [B,C,H,W]`` filled with the leaf modes of the induced tree that is chosen greedily from the
        sum-pass values; the observed entries are returned as they are.  The bottom-up pass of ``sample_conditional`` (the
        leaf map and every sum layer's output under the evidence), then one top-down launch (mode 3 of
        csrc/dgc/dgcspn_topdown.hip) that takes, at the root and at every reached sum node, the input with the largest
        weight * value under the evidence -- the lowest index among equal ones, the largest weight where no input is
        possible -- and at every reached pixel the ``loc`` of the chosen component.  This is the semantics of ``RatSpn.mpe``
        and of the reference's top-down MPE of RAT-SPNs; it is not a global MAP of p(x_missing | x_observed), which a
        max-product bottom-up pass would need.  The reference has no counterpart for DGC-SPNs.

        Against the other completions: ``mpe`` is the reference's gradient form and returns posterior means (for several
        classes, the classes' means added up); ``expectation`` returns the exact posterior mean, a blend of all components;
        ``sample_conditional`` returns one random draw.  This one is deterministic and sharp: every filled pixel is one
        component's location.

        Without labels a model with several classes descends from the class with the largest root output for the row (the
        first of equal ones; a row with a NaN root output, or with every root output ``-inf``, takes class 0); a model with
        one root ignores ``y``; a label outside ``[0, out_classes)`` raises ``ValueError``.  A pixel outside every scope is
        returned as given.  ``return_choice``: also the ``[B, 1 + H*W]`` int32 choices, the root's input index and then the
        component per pixel (-1 for a pixel out of scope)."""
        from deeprob import hip
        from deeprob.hip import dgc, ops, ops_spatial
        device = self._check_topdown('mpe_completion')
        x = ops.require_device_f32(x, 'x')
        if x.dim() != 4 or tuple(x.shape[1:]) != tuple(self.in_features):
            raise ValueError("expected inputs [B, {}], got {}".format(tuple(self.in_features), tuple(x.shape)))
        if self.out_classes == 1 or x.shape[0] == 0:
            y = None
        elif y is not None:
            # (a wrong label is reported before the bottom-up pass is spent on the batch)
            y = hip.require_labels('mpe_completion', y, x.shape[0], self.out_classes, device)
        acts = self._upward_for_sampling(x)
        if self.out_classes > 1 and x.shape[0] > 0 and y is None:
            top = ops_spatial.spatial_prodroot(acts[-1], self.layers[-1], self.root_layer.weight, self.root_layer._ws2)
            if top is None:
                top = self.root_layer(self.layers[-1](acts[-1]))
            # the first maximum; a NaN output equals nothing, so such a row finds none and takes class 0
            index = torch.arange(self.out_classes, device=top.device).expand_as(top)
            first = torch.where(top == top.max(dim=1, keepdim=True).values, index, self.out_classes).min(dim=1).values
            y = torch.where(first < self.out_classes, first, 0)
        geom = dgc.product_geometry(self._product_layers())
        return dgc.dgcspn_topdown(dgc.DPG_MODE_MPE, x.shape[0], self.in_features, geom, self.out_classes, x, y, acts,
                                  self._topdown_logw(), self.base_layer.loc, self.base_layer.scale, 0,
                                  want_choice=return_choice, labels_trusted=True)

    @torch.no_grad()
    def posterior_moments(self, x: torch.Tensor, y: Optional[torch.Tensor] = None,
                          want_var: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """Exact ``(E[x | e, y], Var[x | e, y])`` of every NaN entry of ``x [B,C,H,W]`` given the image's observed entries
        ``e`` (and the class ``y``, when given): the bottom-up pass of ``sample_conditional``, then one top-down launch that
        sends the posterior flow of every sum node to all of its inputs (csrc/dgc/dgcspn_moments.hip) and mixes the leaf
        components' moments by the flow they receive.  An observed entry comes back as it is, with variance 0.  Without
        labels a model with several classes answers for the mixture of its classes under the uniform class prior (class
        ``c`` weighted by ``softmax(root outputs)[c]``); a model with one root ignores ``y``; a label outside
        ``[0, out_classes)`` raises ``ValueError``.  A NaN entry of a pixel outside every scope stays NaN in both outputs,
        as ``sample_conditional`` returns such a pixel as given.  ``mpe`` is the reference's gradient form of the mean:
        autograd through every layer, and no variance."""
        from deeprob.hip import Workspace, dgcm, ops
        self._check_topdown('posterior_moments')
        x = ops.require_device_f32(x, 'x')
        if x.dim() != 4 or tuple(x.shape[1:]) != tuple(self.in_features):
            raise ValueError("expected inputs [B, {}], got {}".format(tuple(self.in_features), tuple(x.shape)))
        acts = self._upward_for_sampling(x)
        if self.out_classes == 1:
            y = None
        if getattr(self, '_moments_ws', None) is None:
            self._moments_ws = Workspace()                      # the flow maps of the launch's work-groups
        geom = dgcm.product_geometry(self._product_layers())
        mean, var, _ = dgcm.dgcspn_moments(self.in_features, geom, self.out_classes, x, y, acts, self._topdown_logw(),
                                           self.base_layer.loc, self.base_layer.scale, self._moments_ws,
                                           all_classes=y is None, want_var=want_var)
        return mean, var

    def expectation(self, x: torch.Tensor, y: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``E[x_missing | x_observed, y]`` in the NaN entries of ``x``, the observed entries as they are: mean imputation,
        the completion of least expected squared error.  See :meth:`posterior_moments`."""
        return self.posterior_moments(x, y, want_var=False)[0]

    def variance(self, x: torch.Tensor, y: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``Var[x_missing | x_observed, y]`` in the NaN entries of ``x``, 0 in the observed ones: the per-pixel uncertainty
        of the imputation.  See :meth:`posterior_moments`."""
        return self.posterior_moments(x, y)[1]

    def loss(self, x: torch.Tensor, y: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.out_classes == 1:
            from deeprob.hip import ops
            return ops.neg_mean(x)
        return torch.nn.functional.nll_loss(torch.log_softmax(x, dim=1), y)

    def apply_constraints(self):
        if self.optimize_scale:
            self.scale_clipper(self.base_layer)
