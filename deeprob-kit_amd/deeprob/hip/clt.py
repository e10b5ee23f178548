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


def rows_on_device(x, name: str) -> torch.Tensor:
    """``x`` as a float32 tensor on a HIP device, under the input rules of the models (``name``: what the model calls itself
    in a message): numpy goes to the current device, a device tensor stays where it is, a CPU tensor or a missing library
    raises ``HipError``."""
    load_library()
    if isinstance(x, torch.Tensor):
        return hip.require_device_f32(x, 'data')
    if not torch.cuda.is_available():
        raise HipError("{} needs a HIP device (there is no CPU fallback)".format(name))
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.device('cuda', torch.cuda.current_device()))


def run_on_device(model, name: str, op, x, *args):
    """``op(model._on_device(device), x on the device, *args)`` under the input rules of ``BinaryCLT`` and ``BinaryCNet``
    (``model``: one of them, ``name``: what it calls itself in a message): numpy in, numpy out through the current device;
    a device tensor stays on its device; a CPU tensor or a missing library raises ``HipError``.  An ``op`` that returns a
    tuple of tensors gives a tuple."""
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
    if not as_numpy:
        return out
    return tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()


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


# ---- mixtures of trees (the last section of the header) --------------------------------------------------------------------
#: the ``dpc_abi_version()`` that has the ``dpc_mix_*`` entry points (``ABI_VERSION``, what the module needs to load, stays)
MIX_ABI_VERSION = 5


def _mix_library():
    lib = load_library()
    version = lib.dpc_abi_version()
    if version < MIX_ABI_VERSION:
        raise HipError("libdeeprob_clt.so at {} has ABI version {}, mixtures of trees need {} -- rebuild it with `make -C "
                       "deeprob-kit_amd/csrc` (or __graft_entry__.build())".format(BINDING.lib_path, version, MIX_ABI_VERSION))
    return lib


class DeviceMixture:
    """The tables of ``K`` trees over the same ``D`` positions, stacked as ``dpc_mix_log_likelihood`` takes them, and the
    float32 log weights ``logw`` ``[K]``, on ``device`` (one host-to-device copy).  ``trees``: ``(bfs, parent, params)``
    per component.  :meth:`update` replaces the parameters and the weights of the same structures in one copy."""

    def __init__(self, trees, logw, device):
        trees = [check_tree(*t) for t in trees]
        k = len(trees)
        if not 1 <= k <= DPC_MIX_MAX_K:
            raise HipError("a mixture of {} components is outside 1..{} (DPC_MIX_MAX_K)".format(k, DPC_MIX_MAX_K))
        d = len(trees[0][1])
        if any(len(t[1]) != d for t in trees):
            raise ValueError("the components of a mixture must have the same number of variables")
        logw = np.ascontiguousarray(logw, np.float32)
        if logw.shape != (k,):
            raise ValueError("expected {} log weights, got {}".format(k, logw.shape))
        csr = [children_csr(bfs, parent) for bfs, parent, _ in trees]
        ints = np.concatenate([np.concatenate([np.asarray(t[0], np.int32) for t in trees]),
                               np.concatenate([np.asarray(t[1], np.int32) for t in trees]),
                               np.concatenate([off for off, _ in csr]), np.concatenate([idx for _, idx in csr])])
        floats = np.concatenate([np.concatenate([t[2].reshape(-1) for t in trees]), logw])
        buf = torch.from_numpy(np.concatenate([ints.view(np.uint8), floats.view(np.uint8)])).to(device)
        self.k, self.d, self.device, self._buf = k, d, buf.device, buf
        ints_d = buf[:4 * len(ints)].view(torch.int32)
        self.bfs, self.parent = ints_d[:k * d], ints_d[k * d:2 * k * d]
        self.child_off, self.child_idx = ints_d[2 * k * d:2 * k * d + k * (d + 1)], ints_d[2 * k * d + k * (d + 1):]
        self._floats = buf[4 * len(ints):].view(torch.float32)
        self.params, self.logw = self._floats[:4 * k * d], self._floats[4 * k * d:]

    def update(self, params, logw):
        """New ``params`` ``[K, D, 2, 2]`` and ``logw`` ``[K]`` for the same trees: one copy."""
        floats = np.concatenate([np.ascontiguousarray(params, np.float32).reshape(-1), np.ascontiguousarray(logw, np.float32)])
        if floats.shape != (self._floats.numel(),):
            raise ValueError("expected params [{}, {}, 2, 2] and {} log weights".format(self.k, self.d, self.k))
        self._floats.copy_(torch.from_numpy(floats), non_blocking=False)

    def pointers(self):
        return (self.bfs.data_ptr(), self.parent.data_ptr(), self.params.data_ptr(), self.child_off.data_ptr(),
                self.child_idx.data_ptr() if self.d > 1 else None, self.logw.data_ptr())


def _mix_batch(mix: DeviceMixture, codes: torch.Tensor, rows):
    """``(b, nb, the pointer of rows or None)`` of a launch over ``codes`` ``[D, b]`` through the batch index ``rows``."""
    if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[0] != mix.d or not codes.is_contiguous():
        raise ValueError("expected codes as [{}, B] uint8 (pack_query), got {} {}".format(mix.d, tuple(codes.shape), codes.dtype))
    if codes.device != mix.device:
        raise HipError("the codes live on '{}', the mixture on '{}'".format(codes.device, mix.device))
    b = codes.shape[1]
    if rows is None:
        return b, b, None
    if rows.dtype != torch.int32 or rows.dim() != 1 or rows.device != codes.device or not rows.is_contiguous():
        raise ValueError("expected rows as a contiguous int32 vector on '{}'".format(codes.device))
    return b, rows.shape[0], rows.data_ptr()


def mixture_codes_log_likelihood(mix: DeviceMixture, codes: torch.Tensor, rows=None, work: torch.Tensor = None,
                                 complete: bool = False):
    """``(ll [nb], comp_ll [nb, K], resp [nb, K])`` float32 of the rows ``rows`` (int32 on the device; None: all, in order)
    of ``codes`` ``[D, b]`` from :func:`pack_query`: ONE ``dpc_mix_log_likelihood``.  ``work``: at least ``K * 2 * D * nb``
    float32 of scratch to reuse, allocated when None.  ``complete``: the caller knows that no row holds NaN (EM has checked
    it): no scratch is allocated or passed, and a row with NaN would get NaN."""
    lib = _mix_library()
    b, nb, rows_ptr = _mix_batch(mix, codes, rows)
    dev = codes.device
    work_ptr = None
    if not complete:
        need = mix.k * 2 * mix.d * nb
        if work is None:
            work = torch.empty(max(need, 1), dtype=torch.float32, device=dev)
        assert work.dtype == torch.float32 and work.device == dev and work.numel() >= need and work.is_contiguous()
        work_ptr = work.data_ptr()
    comp_ll = torch.empty((nb, mix.k), dtype=torch.float32, device=dev)
    ll = torch.empty(nb, dtype=torch.float32, device=dev)
    resp = torch.empty((nb, mix.k), dtype=torch.float32, device=dev)
    call(lib.dpc_mix_log_likelihood, codes.data_ptr(), b, mix.d, rows_ptr, nb, mix.k, *mix.pointers(), work_ptr,
         comp_ll.data_ptr(), ll.data_ptr(), resp.data_ptr(), hip.stream_ptr(dev))
    return ll, comp_ll, resp


def mixture_log_likelihood(mix: DeviceMixture, x: torch.Tensor, rows=None, want_resp: bool = False):
    """``ll`` ``[nb]`` float32, the log likelihood of the rows ``rows`` (None: all) of ``x`` ``[B, D]`` under the mixture,
    NaN entries marginalised; with ``want_resp`` ``(ll, comp_ll [nb, K], resp [nb, K])``.  With a row index it is one
    launch; without, a long batch is evaluated in pieces of ``WORK_FLOATS / (2 D K)`` rows."""
    x = _rows(x, 'x')
    if x.shape[1] != mix.d:
        raise ValueError("expected inputs [B, {}], got {}".format(mix.d, tuple(x.shape)))
    if x.device != mix.device:
        raise HipError("x lives on '{}', the mixture on '{}'".format(x.device, mix.device))
    if rows is not None:
        out = mixture_codes_log_likelihood(mix, pack_query(x), rows)
        return out if want_resp else out[0]
    b = x.shape[0]
    step = query_rows(mix.d * mix.k)
    work = torch.empty(mix.k * 2 * mix.d * min(b, step), dtype=torch.float32, device=x.device)
    pieces = [mixture_codes_log_likelihood(mix, pack_query(x[r0:r0 + step]), None, work) for r0 in range(0, b, step)]
    out = pieces[0] if len(pieces) == 1 else tuple(torch.cat(p) for p in zip(*pieces))
    return out if want_resp else out[0]


def mixture_em_stats(mix: DeviceMixture, codes: torch.Tensor, rows, resp: torch.Tensor) -> torch.Tensor:
    """``stats`` ``[K, 1 + 2 D]`` float64 (``dpc_mix_em_stats``): per component the sum of the responsibilities ``resp``
    ``[nb, K]`` over the batch ``rows`` of ``codes``, their sum where ``x_j = 1`` and where ``x_j = x_parent(j) = 1``, in
    the fixed order of the header."""
    lib = _mix_library()
    b, nb, rows_ptr = _mix_batch(mix, codes, rows)
    dev = codes.device
    if resp.dtype != torch.float32 or tuple(resp.shape) != (nb, mix.k) or resp.device != dev or not resp.is_contiguous():
        raise ValueError("expected resp as [{}, {}] float32 on '{}'".format(nb, mix.k, dev))
    width = 1 + 2 * mix.d
    n_chunks = (nb + DPC_MIX_CHUNK - 1) // DPC_MIX_CHUNK
    part = torch.empty((max(n_chunks, 1), mix.k, width), dtype=torch.float64, device=dev)
    stats = torch.empty((mix.k, width), dtype=torch.float64, device=dev)
    call(lib.dpc_mix_em_stats, codes.data_ptr(), b, mix.d, rows_ptr, nb, mix.k, resp.data_ptr(), mix.parent.data_ptr(),
         part.data_ptr(), stats.data_ptr(), hip.stream_ptr(dev))
    return stats


# ---- posterior queries of a mixture (the dpc_mixq_* section of the header) -------------------------------------------------
#: the ``dpc_abi_version()`` that has the ``dpc_mixq_*`` entry points
MIXQ_ABI_VERSION = 6


def _mixq_library():
    lib = load_library()
    version = lib.dpc_abi_version()
    if version < MIXQ_ABI_VERSION:
        raise HipError("libdeeprob_clt.so at {} has ABI version {}, the posterior queries of a mixture of trees need {} -- "
                       "rebuild it with `make -C deeprob-kit_amd/csrc` (or __graft_entry__.build())".format(
                           BINDING.lib_path, version, MIXQ_ABI_VERSION))
    return lib


def mixture_query_row_bytes(mix: DeviceMixture, what: str) -> int:
    """Bytes of scratch per row of ``dpc_mixq_marginals`` (``what == 'marginals'``) or of the two fills: the header's
    ``16 D + 8 K`` and ``8 D + 8 K``."""
    return (16 if what == 'marginals' else 8) * mix.d + 8 * mix.k


def _mixture_query(mix: DeviceMixture, x: torch.Tensor, what: str, seed: int = 0, row0: int = 0, want_component: bool = False):
    lib = _mixq_library()
    x = _rows(x, 'x')
    if x.shape[1] != mix.d:
        raise ValueError("expected inputs [B, {}], got {}".format(mix.d, tuple(x.shape)))
    if x.device != mix.device:
        raise HipError("x lives on '{}', the mixture on '{}'".format(x.device, mix.device))
    b, d = x.shape
    st = hip.stream_ptr(x.device)
    out = torch.empty((b, d), dtype=torch.float32, device=x.device)
    component = torch.empty(b, dtype=torch.int32, device=x.device) if want_component else None
    step = query_rows(d)        # the piece of `marginals`
    # (float64: the allocator then gives the 8-byte alignment the entry points ask for)
    work = torch.empty(mixture_query_row_bytes(mix, what) * min(b, step) // 8, dtype=torch.float64, device=x.device)
    for r0 in range(0, b, step):
        xs, os_ = x[r0:r0 + step], out[r0:r0 + step]
        n = xs.shape[0]
        codes = pack_query(xs)
        head = (xs.data_ptr(), codes.data_ptr(), n, d, mix.k) + mix.pointers()
        comp = component[r0:r0 + step].data_ptr() if want_component else None
        if what == 'marginals':
            call(lib.dpc_mixq_marginals, *head, work.data_ptr(), os_.data_ptr(), st)
        elif what == 'mpe':
            call(lib.dpc_mixq_mpe, *head, work.data_ptr(), os_.data_ptr(), comp, st)
        else:
            call(lib.dpc_mixq_sample, *head, seed, row0 + r0, work.data_ptr(), os_.data_ptr(), comp, st)
    return (out, component) if want_component else out


def mixture_marginals(mix: DeviceMixture, x: torch.Tensor) -> torch.Tensor:
    """``[B, D]`` float32: ``x`` with every NaN entry replaced by ``p(x_j = 1 | the row's observed entries)`` under the
    mixture, exact (``dpc_mixq_marginals``); NaN where the evidence is impossible under every component."""
    return _mixture_query(mix, x, 'marginals')


def mixture_sample(mix: DeviceMixture, x: torch.Tensor, seed: int, row0: int = 0, want_component: bool = False):
    """``[B, D]`` float32: ``x`` with its NaN entries drawn given the observed ones (``dpc_mixq_sample``): first the
    component from its posterior, then the entries from that tree.  ``row0``: the number of the first row in the generator's
    counters (a batch sampled in pieces gives the bytes of the whole).  With ``want_component`` also ``[B]`` int32, the
    drawn component (-1 where the evidence is impossible; such a row keeps its NaN)."""
    if row0 < 0:
        raise ValueError("row0 must not be negative")
    return _mixture_query(mix, x, 'sample', int(seed) & 0xFFFFFFFFFFFFFFFF, int(row0), want_component)


def mixture_mpe(mix: DeviceMixture, x: torch.Tensor, want_component: bool = False):
    """``[B, D]`` float32: ``x`` with its NaN entries filled by the completion of the pair (component, completion) that
    maximises ``w_k p_k(x)`` (``dpc_mixq_mpe``): the max-product MPE of the mixture's circuit, not the MAP of the mixture
    density.  With ``want_component`` also ``[B]`` int32, the winning component (-1 where the evidence is impossible)."""
    return _mixture_query(mix, x, 'mpe', want_component=want_component)
