"""ctypes binding of ``libdeeprob_clt.so`` (the C ABI declared in ``include/deeprob_clt.h``, prefix ``dpc_``): binary
Chow-Liu trees.  The prototypes and the ``DPC_*`` constants are read from the header with the parser of ``deeprob.hip``;
nothing of them is written down a second time.  There is no CPU fallback: a missing library raises.

The operators below take device tensors, allocate their outputs and scratch with ``torch.empty`` and return device
tensors; :class:`DeviceTree` holds the five tables of a tree, uploaded in one copy.
"""

import numpy as np
import torch

from deeprob import hip
from deeprob.hip import HipError

BINDING = hip.CLT
SIGNATURES, CONSTANTS = BINDING.signatures, BINDING.constants
globals().update(CONSTANTS)
load_library, call, _read_header = BINDING.load, BINDING.call, BINDING.read_header
hip.bound_module(__name__)         # LIB_PATH, HEADER_PATH, ABI_VERSION and _lib are views of BINDING

#: floats of scratch per query launch (128 MiB): a long batch is evaluated in pieces of WORK_FLOATS / (2 D) rows
WORK_FLOATS = 1 << 25


def query_rows(d: int) -> int:
    """Rows per query launch for ``d`` variables: a multiple of 64 (a wave of rows), at least 1024."""
    return max(1024, WORK_FLOATS // (2 * d) // 64 * 64)


def _rows(x: torch.Tensor, name: str) -> torch.Tensor:
    x = hip.require_device_f32(x, name)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("expected {} as [rows, variables], got {}".format(name, tuple(x.shape)))
    return x


def run_on_device(model, name: str, op, x, *args):
    """``op(model._on_device(device), x on the device, *args)`` under the input rules of ``BinaryCLT`` and ``BinaryCNet``
    (``model``: one of them, ``name``: what it calls itself in a message): numpy in, numpy out through the current device;
    a device tensor stays on its device; a CPU tensor or a missing library raises ``HipError``."""
    load_library()
    as_numpy = not isinstance(x, torch.Tensor)
    if as_numpy:
        if not torch.cuda.is_available():
            raise HipError("{} needs a HIP device (there is no CPU fallback)".format(name))
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.device('cuda', torch.cuda.current_device()))
    elif not x.is_cuda:
        raise HipError("x lives on '{}': the deeprob HIP path only works on tensors on a HIP device (there is no CPU "
                       "fallback) -- build the libraries with `make -C deeprob-kit_amd/csrc` and pass a numpy array or a "
                       "device tensor".format(x.device))
    if x.dim() != 2 or x.shape[1] != len(model.scope):
        raise ValueError("expected inputs [B, {}], got {}".format(len(model.scope), tuple(x.shape)))
    out = op(model._on_device(x.device), x, *args)
    return out.cpu().numpy() if as_numpy else out


def children_csr(bfs, parent):
    """``(child_off [D + 1], child_idx [D - 1])`` int32: the children of every node in decreasing position in ``bfs``
    (the header's list order)."""
    bfs, parent = np.asarray(bfs, np.int64), np.asarray(parent, np.int64)
    d = len(parent)
    lists = [[] for _ in range(d)]
    for j in bfs[:0:-1]:
        lists[parent[j]].append(int(j))
    off = np.zeros(d + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    idx = np.asarray([c for l in lists for c in l], np.int32)
    return off, idx


def check_tree(bfs, parent, params):
    """``(bfs, parent, params)`` as int64 / int64 / contiguous float32 arrays, checked on the host: the kernels trust these
    tables (they index device memory with them).  One root, first in ``bfs``, and every other node after its parent."""
    d = len(parent)
    if not 1 <= d <= DPC_MAX_D:
        raise HipError("a tree of {} variables is outside 1..{} (DPC_MAX_D)".format(d, DPC_MAX_D))
    params = np.ascontiguousarray(params, np.float32)
    bfs, parent = np.asarray(bfs, np.int64), np.asarray(parent, np.int64)
    position = np.full(d, -1, np.int64)
    if bfs.shape == (d,) and ((0 <= bfs) & (bfs < d)).all():
        position[bfs] = np.arange(d)
    rest = bfs[1:] if (position >= 0).all() else None
    if rest is None or parent.shape != (d,) or parent[bfs[0]] != -1 or not ((0 <= parent[rest]) & (parent[rest] < d)).all() \
            or not (position[parent[rest]] < position[rest]).all():
        raise ValueError("bfs and tree do not describe one rooted tree")
    if params.shape != (d, 2, 2):
        raise ValueError("Invalid conditional probability table (CPT) shape")
    return bfs, parent, params


class DeviceTree:
    """``bfs``, ``parent``, ``params`` and the children lists of one tree on ``device`` (one host-to-device copy)."""

    def __init__(self, bfs, parent, params, device):
        bfs, parent, params = check_tree(bfs, parent, params)
        d = len(parent)
        off, idx = children_csr(bfs, parent)
        ints = np.concatenate([np.asarray(bfs, np.int32), np.asarray(parent, np.int32), off, idx])
        buf = torch.from_numpy(np.concatenate([ints.view(np.uint8), params.reshape(-1).view(np.uint8)])).to(device)
        self.d, self.device, self._buf = d, buf.device, buf
        ints_d = buf[:4 * len(ints)].view(torch.int32)
        self.bfs, self.parent = ints_d[:d], ints_d[d:2 * d]
        self.child_off, self.child_idx = ints_d[2 * d:3 * d + 1], ints_d[3 * d + 1:]
        self.params = buf[4 * len(ints):].view(torch.float32)

    def pointers(self):
        return (self.bfs.data_ptr(), self.parent.data_ptr(), self.params.data_ptr(), self.child_off.data_ptr(),
                self.child_idx.data_ptr() if self.d > 1 else None)


def pack_bits(x: torch.Tensor) -> torch.Tensor:
    """``[D, W]`` int64 bit planes of the 0/1 rows ``x`` ``[N, D]`` (``dpc_pack_bits``)."""
    x = _rows(x, 'data')
    n, d = x.shape
    planes = torch.empty((d, (n + 63) // 64), dtype=torch.int64, device=x.device)
    call(load_library().dpc_pack_bits, x.data_ptr(), n, d, planes.data_ptr(), hip.stream_ptr(x.device))
    return planes


def pair_counts(planes: torch.Tensor) -> torch.Tensor:
    """``[D, D]`` int32 co-occurrence counts of the planes of :func:`pack_bits` (``dpc_pair_counts``)."""
    assert planes.dtype == torch.int64 and planes.dim() == 2 and planes.is_contiguous()
    d, w = planes.shape
    ones = torch.empty((d, d), dtype=torch.int32, device=planes.device)
    call(load_library().dpc_pair_counts, planes.data_ptr(), w, d, ones.data_ptr(), hip.stream_ptr(planes.device))
    return ones


def pack_query(x: torch.Tensor) -> torch.Tensor:
    """``[D, B]`` uint8 codes of the query rows ``x`` ``[B, D]`` (``dpc_pack_query``)."""
    x = _rows(x, 'x')
    b, d = x.shape
    codes = torch.empty((d, b), dtype=torch.uint8, device=x.device)
    call(load_library().dpc_pack_query, x.data_ptr(), b, d, codes.data_ptr(), hip.stream_ptr(x.device))
    return codes


def _query(tree: DeviceTree, x: torch.Tensor, what: str, seed: int = 0) -> torch.Tensor:
    lib = load_library()
    x = _rows(x, 'x')
    if x.shape[1] != tree.d:
        raise ValueError("expected inputs [B, {}], got {}".format(tree.d, tuple(x.shape)))
    if x.device != tree.device:
        raise HipError("x lives on '{}', the tree on '{}'".format(x.device, tree.device))
    b, d = x.shape
    st = hip.stream_ptr(x.device)
    out = torch.empty(b if what == 'll' else (b, d), dtype=torch.float32, device=x.device)
    step = query_rows(d)
    work = torch.empty(2 * d * min(b, step), dtype=torch.float32, device=x.device)
    for r0 in range(0, b, step):
        xs, os_ = x[r0:r0 + step], out[r0:r0 + step]
        n = xs.shape[0]
        codes = pack_query(xs)
        if what == 'll':
            call(lib.dpc_clt_log_likelihood, codes.data_ptr(), n, d, *tree.pointers(), work.data_ptr(), os_.data_ptr(), st)
        elif what == 'marginals':
            call(lib.dpc_mar_clt, xs.data_ptr(), codes.data_ptr(), n, d, *tree.pointers(), work.data_ptr(), os_.data_ptr(), st)
        elif what == 'mpe':
            call(lib.dpc_clt_mpe, xs.data_ptr(), codes.data_ptr(), n, d, *tree.pointers(), work.data_ptr(), os_.data_ptr(), st)
        else:
            call(lib.dpc_clt_sample, xs.data_ptr(), codes.data_ptr(), n, d, *tree.pointers(), seed, r0, work.data_ptr(),
                 os_.data_ptr(), st)
    return out


def log_likelihood(tree: DeviceTree, x: torch.Tensor) -> torch.Tensor:
    """``[B]`` float32 (``dpc_clt_log_likelihood``); NaN entries are marginalised."""
    return _query(tree, x, 'll')


def mpe(tree: DeviceTree, x: torch.Tensor) -> torch.Tensor:
    """``[B, D]`` float32: ``x`` with its NaN entries filled by the most probable completion (``dpc_clt_mpe``)."""
    return _query(tree, x, 'mpe')


def sample(tree: DeviceTree, x: torch.Tensor, seed: int) -> torch.Tensor:
    """``[B, D]`` float32: ``x`` with its NaN entries drawn given the observed ones (``dpc_clt_sample``)."""
    return _query(tree, x, 'sample', int(seed) & 0xFFFFFFFFFFFFFFFF)


def marginals(tree: DeviceTree, x: torch.Tensor) -> torch.Tensor:
    """``[B, D]`` float32: ``x`` with every NaN entry replaced by ``p(x_j = 1 | the row's observed entries)``, exact
    (``dpc_mar_clt``); NaN where the row's evidence has probability zero."""
    return _query(tree, x, 'marginals')
