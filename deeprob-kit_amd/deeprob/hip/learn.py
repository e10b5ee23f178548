"""ctypes binding of ``libdeeprob_learn.so`` (the C ABI declared in ``include/deeprob_learn.h``, prefix ``dpl_``): the
LearnSPN statistics kernels.  The prototypes and the ``DPL_*`` constants are read from the header with the parser of
``deeprob.hip``; nothing of them is written down a second time.  There is no CPU fallback: a missing library raises.

The operators below take the training set as :class:`DeviceData` and a generation's row-index array, allocate their
outputs with ``torch.empty`` and return them; the small integer tables of a launch go up in ONE host-to-device copy
(``upload``).  ``COUNTERS`` counts kernel launches, host reads and uploads for ``learn_spn``'s ``info``.
"""
import ctypes
import os

import numpy as np
import torch

from deeprob import hip
from deeprob.hip import HipError

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', '..', 'include', 'deeprob_learn.h'))
LIB_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', 'lib', 'libdeeprob_learn.so'))


def _read_header():
    if not os.path.isfile(HEADER_PATH):
        raise HipError("deeprob_learn.h not found at {} -- it is the declaration of the C ABI this binding is built "
                       "from".format(HEADER_PATH))
    with open(HEADER_PATH) as f:
        return hip.parse_header(f.read(), prefix='dpl', header='deeprob_learn.h')


SIGNATURES, CONSTANTS, _ = _read_header()
globals().update(CONSTANTS)

_lib = None


def load_library() -> ctypes.CDLL:
    """Load ``libdeeprob_learn.so`` (built in-tree by ``__graft_entry__.build()``) and bind every symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise HipError(
            "libdeeprob_learn.so not found at {} -- build it with `make -C deeprob-kit_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback".format(LIB_PATH))
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if the .so and the header disagree
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def call(fn, *args) -> int:
    rc = fn(*args)
    if rc < 0:
        msg = load_library().dpl_last_error()
        raise HipError("{} failed ({}): {}".format(fn.__name__, rc, msg.decode() if msg else ''))
    return rc


#: kernel launches outside the Lloyd loop, kernel launches inside it, device-to-host reads, host-to-device uploads
COUNTERS = {'kernels': 0, 'lloyd_kernels': 0, 'reads': 0, 'lloyd_reads': 0, 'uploads': 0}


def reset_counters():
    for k in COUNTERS:
        COUNTERS[k] = 0


def read(t: torch.Tensor, lloyd: bool = False) -> np.ndarray:
    """One device-to-host read (it waits for the stream)."""
    COUNTERS['lloyd_reads' if lloyd else 'reads'] += 1
    return t.cpu().numpy()


def upload(device, **arrays):
    """Integer host tables of one launch, packed into one int64-aligned buffer and copied in ONE transfer: a dict of
    device views (int32 or int64, as the host arrays are)."""
    COUNTERS['uploads'] += 1
    parts, spans, o = [], {}, 0
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        if a.dtype not in (np.int32, np.int64, np.uint8):
            raise TypeError('{}: {}'.format(name, a.dtype))
        raw = a.view(np.uint8).reshape(-1)
        pad = (-len(raw)) % 8
        parts.append(raw)
        if pad:
            parts.append(np.zeros(pad, np.uint8))
        spans[name] = (o, len(raw), a.dtype, a.shape)
        o += len(raw) + pad
    host = np.concatenate(parts) if parts else np.zeros(8, np.uint8)
    dev = torch.from_numpy(host).to(device)
    out = {}
    for name, (o, n, dtype, shape) in spans.items():
        view = dev[o:o + n]
        out[name] = view.view({np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64,
                               np.dtype(np.uint8): torch.uint8}[np.dtype(dtype)]).reshape(shape)
    out['_buffer'] = dev
    return out


class DeviceData:
    """The training set on the device: uint8 domain positions, column major (see the header)."""

    def __init__(self, x_cm: torch.Tensor, n_rows: int, n_cols: int):
        if not x_cm.is_cuda:
            raise HipError("data lives on '{}': the deeprob HIP path only works on a HIP device (there is no CPU "
                           "fallback)".format(x_cm.device))
        assert x_cm.dtype == torch.uint8 and x_cm.is_contiguous() and x_cm.numel() == n_rows * n_cols
        self.x, self.n_rows, self.n_cols, self.device = x_cm, int(n_rows), int(n_cols), x_cm.device

    def head(self, row_index: torch.Tensor):
        assert row_index.dtype == torch.int32 and row_index.is_contiguous() and row_index.device == self.device
        return (self.x.data_ptr(), self.n_rows, self.n_cols, row_index.data_ptr(), row_index.numel())


def _stream(device):
    return hip.stream_ptr(device)


def column_counts(data: DeviceData, row_index, item_col, item_row_off, item_n, kmax: int) -> torch.Tensor:
    """``[n_items, kmax]`` int32 counts (``dpl_column_counts``); the item tables are host arrays."""
    lib = load_library()
    n_items = len(item_col)
    t = upload(data.device, col=np.asarray(item_col, np.int32), off=np.asarray(item_row_off, np.int64),
               n=np.asarray(item_n, np.int32))
    counts = torch.empty((n_items, kmax), dtype=torch.int32, device=data.device)
    call(lib.dpl_column_counts, *data.head(row_index), t['col'].data_ptr(), t['off'].data_ptr(), t['n'].data_ptr(), n_items,
         kmax, counts.data_ptr(), _stream(data.device))
    COUNTERS['kernels'] += 1
    return counts


def pair_g(data: DeviceData, row_index, col_i, col_j, row_off, n, ki, kj) -> torch.Tensor:
    """``[n_pairs]`` float64 G statistics (``dpl_pair_g``); the pair tables are host arrays."""
    lib = load_library()
    n_pairs = len(col_i)
    t = upload(data.device, ci=np.asarray(col_i, np.int32), cj=np.asarray(col_j, np.int32), off=np.asarray(row_off, np.int64),
               n=np.asarray(n, np.int32), ki=np.asarray(ki, np.int32), kj=np.asarray(kj, np.int32))
    g = torch.empty(n_pairs, dtype=torch.float64, device=data.device)
    call(lib.dpl_pair_g, *data.head(row_index), t['ci'].data_ptr(), t['cj'].data_ptr(), t['off'].data_ptr(), t['n'].data_ptr(),
         t['ki'].data_ptr(), t['kj'].data_ptr(), n_pairs, g.data_ptr(), _stream(data.device))
    COUNTERS['kernels'] += 1
    return g


def pair_maxcorr(data: DeviceData, row_index, col_i, col_j, row_off, n, ki, kj) -> torch.Tensor:
    """``[n_pairs]`` float64 maximal correlations (``dpl_pair_maxcorr``); the pair tables are host arrays."""
    lib = load_library()
    n_pairs = len(col_i)
    t = upload(data.device, ci=np.asarray(col_i, np.int32), cj=np.asarray(col_j, np.int32), off=np.asarray(row_off, np.int64),
               n=np.asarray(n, np.int32), ki=np.asarray(ki, np.int32), kj=np.asarray(kj, np.int32))
    score = torch.empty(n_pairs, dtype=torch.float64, device=data.device)
    call(lib.dpl_pair_maxcorr, *data.head(row_index), t['ci'].data_ptr(), t['cj'].data_ptr(), t['off'].data_ptr(),
         t['n'].data_ptr(), t['ki'].data_ptr(), t['kj'].data_ptr(), n_pairs, score.data_ptr(), _stream(data.device))
    COUNTERS['kernels'] += 1
    return score


def partition_rows(row_index, src_off, src_n, label_off, label, dst_off, dst_n, labels, n_out: int) -> torch.Tensor:
    """The next generation's ``[n_out]`` int32 row-index array (``dpl_partition_rows``); ``labels``: a device uint8
    tensor or None."""
    lib = load_library()
    device = row_index.device
    t = upload(device, so=np.asarray(src_off, np.int64), sn=np.asarray(src_n, np.int32), lo=np.asarray(label_off, np.int64),
               lb=np.asarray(label, np.int32), do=np.asarray(dst_off, np.int64), dn=np.asarray(dst_n, np.int32))
    out = torch.empty(n_out, dtype=torch.int32, device=device)
    call(lib.dpl_partition_rows, row_index.data_ptr(), row_index.numel(), t['so'].data_ptr(), t['sn'].data_ptr(),
         t['lo'].data_ptr(), t['lb'].data_ptr(), t['do'].data_ptr(), t['dn'].data_ptr(), len(src_n),
         None if labels is None else labels.data_ptr(), 0 if labels is None else labels.numel(), out.data_ptr(), n_out,
         _stream(device))
    COUNTERS['kernels'] += 1
    return out


class KMeansBatch:
    """The k-means of all row-splitting tasks of one generation (header: "k-means").  ``tasks``: a list of
    ``(row_off, n, cols, ks, seeds)`` with ``seeds`` an ``[n_restarts, n_clusters]`` array of row positions."""

    MAX_ITER = 100

    def __init__(self, data: DeviceData, row_index, tasks, n_restarts: int, n_clusters: int, kmax: int):
        self.data, self.row_index, self.R, self.C, self.kmax = data, row_index, n_restarts, n_clusters, max(int(kmax), 2)
        self.T = len(tasks)
        col_off, cols, ks, cent_off, lab_off = [0], [], [], [], []
        n_cent = n_lab = 0
        for row_off, n, tcols, tks, seeds in tasks:
            cols += list(tcols)
            ks += list(tks)
            col_off.append(len(cols))
            cent_off.append(n_cent)
            lab_off.append(n_lab)
            n_cent += n_restarts * n_clusters * len(tcols) * self.kmax
            n_lab += n
        self.n_cent, self.n_lab = n_cent, n_lab
        block_task, block_row0, item_task, item_p = [], [], [], []
        for t, (row_off, n, tcols, _, _) in enumerate(tasks):
            for r0 in range(0, n, 256):
                block_task.append(t)
                block_row0.append(r0)
            item_task += [t] * len(tcols)
            item_p += list(range(len(tcols)))
        self.n_blocks, self.n_items = len(block_task), len(item_task)
        self.tab = upload(
            data.device, col_off=np.asarray(col_off, np.int32), cols=np.asarray(cols, np.int32), ks=np.asarray(ks, np.int32),
            row_off=np.asarray([t[0] for t in tasks], np.int64), n=np.asarray([t[1] for t in tasks], np.int32),
            cent_off=np.asarray(cent_off, np.int64), lab_off=np.asarray(lab_off, np.int64),
            seeds=np.concatenate([np.asarray(t[4], np.int32).reshape(-1) for t in tasks]),
            block_task=np.asarray(block_task, np.int32), block_row0=np.asarray(block_row0, np.int32),
            item_task=np.asarray(item_task, np.int32), item_p=np.asarray(item_p, np.int32))
        self.lab_off = lab_off

    def run(self):
        """``(inertia [T, R] float64, sizes [T, R, C] int32, labels [R, n_lab] device uint8, iterations)``."""
        lib, d, p = load_library(), self.data, {k: v.data_ptr() for k, v in self.tab.items()}
        dev, st = d.device, _stream(d.device)
        head = d.head(self.row_index)
        cent = torch.empty(self.n_cent, dtype=torch.float64, device=dev)
        labels = torch.empty((self.R, self.n_lab), dtype=torch.uint8, device=dev)
        changed = torch.zeros(self.MAX_ITER, dtype=torch.int32, device=dev)
        COUNTERS['kernels'] += 1        # (the fill of `changed`)
        call(lib.dpl_kmeans_init, *head, p['col_off'], p['cols'], p['row_off'], p['n'], p['cent_off'], p['seeds'], self.T,
             self.R, self.C, self.kmax, cent.data_ptr(), self.n_cent, st)
        COUNTERS['kernels'] += 1
        iterations = 0
        for it in range(self.MAX_ITER):
            call(lib.dpl_kmeans_assign, *head, p['col_off'], p['cols'], p['ks'], p['row_off'], p['n'], p['cent_off'],
                 p['lab_off'], p['block_task'], p['block_row0'], self.n_blocks, self.R, self.C, self.kmax, cent.data_ptr(),
                 labels.data_ptr(), self.n_lab, 1 if it == 0 else 0, changed[it:].data_ptr(), st)
            COUNTERS['lloyd_kernels'] += 1
            iterations = it + 1
            if int(read(changed[it:it + 1], lloyd=True)[0]) == 0 or it == self.MAX_ITER - 1:
                break
            call(lib.dpl_kmeans_update, *head, p['col_off'], p['cols'], p['row_off'], p['n'], p['cent_off'], p['lab_off'],
                 p['item_task'], p['item_p'], self.n_items, self.R, self.C, self.kmax, labels.data_ptr(), self.n_lab,
                 cent.data_ptr(), st)
            COUNTERS['lloyd_kernels'] += 1
        inertia = torch.empty((self.T, self.R), dtype=torch.float64, device=dev)
        sizes = torch.empty((self.T, self.R, self.C), dtype=torch.int32, device=dev)
        call(lib.dpl_kmeans_inertia, *head, p['col_off'], p['cols'], p['ks'], p['row_off'], p['n'], p['cent_off'], p['lab_off'],
             self.T, self.R, self.C, self.kmax, cent.data_ptr(), labels.data_ptr(), self.n_lab, inertia.data_ptr(),
             sizes.data_ptr(), st)
        COUNTERS['kernels'] += 1
        return read(inertia), read(sizes), labels, iterations
