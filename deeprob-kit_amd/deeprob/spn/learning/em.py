"""Batch Expectation-Maximization for a vanilla SPN (reference: deeprob/spn/learning/em.py:18-113) on the HIP path:
one ``dpk_flat_spn_em_step`` per iteration, parameters updated on the device."""
import ctypes
from typing import Optional, Union

import numpy as np
import torch

from deeprob.hip import load_library, call, ptr, stream_ptr
from deeprob.spn.structure.io import FlatSpn, KIND
from deeprob.utils.random import RandomState, check_random_state


def draw_batches(random_state: np.random.RandomState, n_samples: int, batch_size: int, num_iter: int) -> np.ndarray:
    """The batch rows of every iteration ``[num_iter, batch_size]`` int32: the reference's draws (em.py:86), which do
    not depend on any result and are therefore taken up front."""
    if batch_size <= 0:
        return np.zeros((num_iter, 0), np.int32)
    return np.stack([random_state.choice(n_samples, size=batch_size, replace=False)
                     for _ in range(num_iter)]).astype(np.int32)


def expectation_maximization(
    root: FlatSpn,
    data: Union[np.ndarray, torch.Tensor],
    num_iter: int = 100,
    batch_perc: float = 0.1,
    step_size: float = 0.5,
    random_init: bool = True,
    random_state: Optional[RandomState] = None,
    verbose: bool = True
) -> FlatSpn:
    """
    Learn the parameters of a SPN by batch Expectation-Maximization (EM).
    See https://arxiv.org/abs/1604.07243 and https://arxiv.org/abs/2004.06231 for details.

    The batches are the reference's draws (``random_state.choice(n_samples, batch_size, replace=False)`` per
    iteration); all of them are drawn up front and the kernels gather the rows through the index.  With
    ``verbose=False`` the loop never waits for the device.  Two calls with the same arguments give bitwise identical
    parameters.  Unlike the reference (which lets NaN flow into the parameters), data containing NaN is an error.

    :param root: The SPN (as loaded by ``deeprob.spn.structure.io.load_spn_json``); updated in place.  A
                 ``deeprob.spn.structure.BinaryCLTMixture`` is handed to its own ``em`` with the same arguments.
    :param data: The data to use to learn the parameters ``[n_samples, >= n_features]`` (numpy, evaluated on the
                 current HIP device, or a tensor on a HIP device).
    :param num_iter: The number of iterations.
    :param batch_perc: The percentage of data to use for each step.
    :param step_size: The step size for batch EM.
    :param random_init: Whether to random initialize the weights of the SPN.
    :param random_state: The random state. It can be either None, a seed integer or a Numpy RandomState.
    :param verbose: Whether to show the batch mean log-likelihood of every iteration.
    :return: The spn with learned parameters.
    :raises ValueError: If a parameter is out of domain, or the data contains NaN.
    :raises NotImplementedError: If the SPN has a Uniform leaf (as the reference); nothing is modified then.
    """
    from deeprob.spn.structure.cltmix import BinaryCLTMixture
    if isinstance(root, BinaryCLTMixture):      # a mixture of Chow-Liu trees trains itself, with the CPTs of a tree tied
        return root.em(data, num_iter=num_iter, batch_perc=batch_perc, step_size=step_size, random_init=random_init,
                       random_state=random_state, verbose=verbose)
    if num_iter <= 0:
        raise ValueError("The number of iterations must be positive")
    if batch_perc <= 0.0 or batch_perc >= 1.0:
        raise ValueError("The batch percentage must be in (0, 1)")
    if step_size <= 0.0 or step_size >= 1.0:
        raise ValueError("The step size must be in (0, 1)")
    if not isinstance(root, FlatSpn):
        raise TypeError("expectation_maximization works on the FlatSpn returned by deeprob.spn.structure.io.load_spn_json")
    root.check()
    if (root.kind == KIND['Uniform']).any():
        raise NotImplementedError("EM step not yet implemented for Uniform distributions")
    lib = load_library()
    if isinstance(data, torch.Tensor):
        from deeprob.hip import require_device_f32
        xd = require_device_f32(data, 'data')
    else:
        xd = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).to(
            torch.device('cuda', torch.cuda.current_device()))
    if xd.dim() != 2 or xd.shape[1] < root.n_features:
        raise ValueError("expected data [n_samples, >= {}], got {}".format(root.n_features, tuple(xd.shape)))
    if bool(torch.isnan(xd[:, :root.n_features]).any()):
        raise ValueError("The data contains NaN: EM needs complete rows")
    n_samples, D = xd.shape
    batch_size = int(batch_perc * n_samples)
    random_state = check_random_state(random_state)
    if random_init:
        root.em_init(random_state)
    dev = xd.device
    index = torch.from_numpy(draw_batches(random_state, n_samples, batch_size, num_iter)).to(dev)
    root.refresh()                                   # the device copies hold what the host holds
    rec = root.circuit(dev)
    n = call(lib.dpk_flat_spn_em_step_workspace_bytes, batch_size, ctypes.addressof(rec))
    ws = torch.empty(max(int(n), 1), dtype=torch.uint8, device=dev)
    mean_ll = torch.zeros(num_iter, dtype=torch.float64, device=dev)
    bar = None
    if verbose:
        try:
            from tqdm import tqdm
            bar = tqdm(total=num_iter, leave=None, unit='batch',
                       bar_format='{desc}| {n_fmt}/{total_fmt} [{elapsed}<{remaining}, {rate_fmt}]')
        except ImportError:
            bar = None
    stream = stream_ptr(dev)
    for it in range(num_iter):
        call(lib.dpk_flat_spn_em_step, ptr(xd), n_samples, D, index.data_ptr() + 4 * it * batch_size, batch_size,
                                       ctypes.addressof(rec), float(step_size), mean_ll.data_ptr() + 8 * it, ptr(ws),
                                       ws.numel(), stream)
        if verbose:
            text = 'Batch Avg. LL: {:.4f}'.format(float(mean_ll[it]))
            if bar is not None:
                bar.set_description(text)
                bar.update(1)
            else:
                print('[{}/{}] {}'.format(it + 1, num_iter, text))
    if bar is not None:
        bar.close()
    root.pull(dev)
    #: batch mean log-likelihood of every iteration (before its update), kept on the device
    root.em_mean_ll = mean_ll
    return root
