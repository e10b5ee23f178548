"""ctypes binding of ``libdeeprob_learn.so`` (the C ABI declared in ``include/deeprob_learn.h``, prefix ``dpl_``): the
LearnSPN statistics kernels.  The prototypes and the ``DPL_*`` constants are read from the header with the parser of
``deeprob.hip``; nothing of them is written down a second time.  There is no CPU fallback: a missing library raises.

The operators below take the training set as :class:`DeviceData` and a generation's row-index array, allocate their
outputs with ``torch.empty`` and return them; the small integer tables of a launch go up in ONE host-to-device copy
(``upload``).  ``COUNTERS`` counts kernel launches, host reads and uploads for ``learn_spn``'s ``info``.
"""

import numpy as np
import torch

from deeprob import hip
from deeprob.hip import HipError

BINDING = hip.LEARN
SIGNATURES, CONSTANTS = BINDING.signatures, BINDING.constants
globals().update(CONSTANTS)
load_library, call, _read_header = BINDING.load, BINDING.call, BINDING.read_header
hip.bound_module(__name__)         # LIB_PATH, HEADER_PATH, ABI_VERSION and _lib are views of BINDING


#: kernel launches outside the Lloyd loop, kernel launches inside it, device-to-host reads, host-to-device uploads; and the
#: launches, reads and uploads of the EM loop of the Gaussian-mixture row split, counted apart (``GmmBatch``)
COUNTERS = {'kernels': 0, 'lloyd_kernels': 0, 'reads': 0, 'lloyd_reads': 0, 'uploads': 0,
            'gmm_kernels': 0, 'gmm_reads': 0, 'gmm_uploads': 0}


def reset_counters():
    for k in COUNTERS:
        COUNTERS[k] = 0


def read(t: torch.Tensor, lloyd: bool = False, gmm: bool = False) -> np.ndarray:
    """One device-to-host read (it waits for the stream)."""
    COUNTERS['gmm_reads' if gmm else 'lloyd_reads' if lloyd else 'reads'] += 1
    return t.cpu().numpy()


def upload(device, _counter='uploads', **arrays):
    """Host tables of one launch (int32, int64, uint8, float32 or float64), packed into one int64-aligned buffer and copied
    in ONE transfer: a dict of device views of the host arrays' types."""
    COUNTERS[_counter] += 1
    parts, spans, o = [], {}, 0
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        if a.dtype not in (np.int32, np.int64, np.uint8, np.float32, np.float64):
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
        out[name] = view.view({np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8,
                               np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}[np.dtype(dtype)]).reshape(shape)
    out['_buffer'] = dev
    return out


class DeviceData:
    """The training set on the device, column major: uint8 domain positions, or float32 values (see the header,
    "continuous data").  The dtype tells the two apart; every operator asserts the one it takes."""

    def __init__(self, x_cm: torch.Tensor, n_rows: int, n_cols: int):
        if not x_cm.is_cuda:
            raise HipError("data lives on '{}': the deeprob HIP path only works on a HIP device (there is no CPU "
                           "fallback)".format(x_cm.device))
        assert x_cm.dtype in (torch.uint8, torch.float32) and x_cm.is_contiguous() and x_cm.numel() == n_rows * n_cols
        self.x, self.n_rows, self.n_cols, self.device = x_cm, int(n_rows), int(n_cols), x_cm.device
        self.is_float = x_cm.dtype == torch.float32

    def head(self, row_index: torch.Tensor):
        assert row_index.dtype == torch.int32 and row_index.is_contiguous() and row_index.device == self.device
        return (self.x.data_ptr(), self.n_rows, self.n_cols, row_index.data_ptr(), row_index.numel())


def _stream(device):
    return hip.stream_ptr(device)


def _items(device, item_col, item_row_off, item_n, **more):
    """The ``col`` / ``off`` / ``n`` tables of a launch over items (one column of one row segment each), with whatever
    else the launch needs, in one upload."""
    return upload(device, col=np.asarray(item_col, np.int32), off=np.asarray(item_row_off, np.int64),
                  n=np.asarray(item_n, np.int32), **more)


def _row_blocks(ns):
    """(item of each 256-row block, its first row) for items of ``ns`` rows."""
    item, row0 = [], []
    for i, n in enumerate(ns):
        for r0 in range(0, int(n), 256):
            item.append(i)
            row0.append(r0)
    return np.asarray(item, np.int32), np.asarray(row0, np.int32)


def column_counts(data: DeviceData, row_index, item_col, item_row_off, item_n, kmax: int) -> torch.Tensor:
    """``[n_items, kmax]`` int32 counts (``dpl_column_counts``); the item tables are host arrays."""
    assert not data.is_float
    t = _items(data.device, item_col, item_row_off, item_n)
    counts = torch.empty((len(item_col), kmax), dtype=torch.int32, device=data.device)
    call(load_library().dpl_column_counts, *data.head(row_index), t['col'].data_ptr(), t['off'].data_ptr(), t['n'].data_ptr(),
         len(item_col), kmax, counts.data_ptr(), _stream(data.device))
    COUNTERS['kernels'] += 1
    return counts


def _pair_statistic(entry, data: DeviceData, row_index, col_i, col_j, row_off, n, ki, kj) -> torch.Tensor:
    """``[n_pairs]`` float64 from the entry point ``entry`` over column pairs; the six pair tables are host arrays."""
    assert not data.is_float
    t = upload(data.device, ci=np.asarray(col_i, np.int32), cj=np.asarray(col_j, np.int32), off=np.asarray(row_off, np.int64),
               n=np.asarray(n, np.int32), ki=np.asarray(ki, np.int32), kj=np.asarray(kj, np.int32))
    out = torch.empty(len(col_i), dtype=torch.float64, device=data.device)
    call(getattr(load_library(), entry), *data.head(row_index), t['ci'].data_ptr(), t['cj'].data_ptr(), t['off'].data_ptr(),
         t['n'].data_ptr(), t['ki'].data_ptr(), t['kj'].data_ptr(), len(col_i), out.data_ptr(), _stream(data.device))
    COUNTERS['kernels'] += 1
    return out


def pair_g(data: DeviceData, row_index, col_i, col_j, row_off, n, ki, kj) -> torch.Tensor:
    """``[n_pairs]`` float64 G statistics (``dpl_pair_g``)."""
    return _pair_statistic('dpl_pair_g', data, row_index, col_i, col_j, row_off, n, ki, kj)


def pair_maxcorr(data: DeviceData, row_index, col_i, col_j, row_off, n, ki, kj) -> torch.Tensor:
    """``[n_pairs]`` float64 maximal correlations (``dpl_pair_maxcorr``)."""
    return _pair_statistic('dpl_pair_maxcorr', data, row_index, col_i, col_j, row_off, n, ki, kj)


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


def pair_ones(data: DeviceData, row_index, blocks, row_chunk: int = None):
    """The co-occurrence counts of every block (``dpl_pair_ones``): ``blocks`` is a list of ``(row_off, n, cols)``, one
    leaf task each.  Returns ``(ones, out_off)``: a device int32 tensor with block t's ``[m, m]`` counts, row major, at
    ``ones[out_off[t] : out_off[t] + m * m]``.  One table upload and one call (a zeroing launch and the counting launch);
    ``row_chunk``: the rows of one unit, ``DPL_PAIR_ROW_CHUNK`` when None."""
    assert not data.is_float and data.x.dtype == torch.uint8
    tile = CONSTANTS['DPL_PAIR_TILE']
    row_chunk = int(CONSTANTS['DPL_PAIR_ROW_CHUNK'] if row_chunk is None else row_chunk)
    ms = [len(cols) for _, _, cols in blocks]
    assert blocks and min(ms) >= 1 and min(int(n) for _, n, _ in blocks) >= 1 and row_chunk >= 1
    col_off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum([m * m for m in ms])]).astype(np.int64)
    unit = {key: [] for key in ('blk', 'ti', 'tj', 'row0')}
    for b, ((_, n, _), m) in enumerate(zip(blocks, ms)):
        tiles = -(-m // tile)
        for ti in range(tiles):
            for tj in range(ti, tiles):
                for row0 in range(0, int(n), row_chunk):
                    for key, v in zip(('blk', 'ti', 'tj', 'row0'), (b, ti, tj, row0)):
                        unit[key].append(v)
    t = upload(data.device, col=np.concatenate([np.asarray(cols, np.int32).reshape(-1) for _, _, cols in blocks]),
               col_off=col_off[:-1].copy(), m=np.asarray(ms, np.int32), row_off=np.asarray([b[0] for b in blocks], np.int64),
               n=np.asarray([b[1] for b in blocks], np.int32), out_off=out_off[:-1].copy(),
               **{'unit_' + key: np.asarray(v, np.int32) for key, v in unit.items()})
    ones = torch.empty(int(out_off[-1]), dtype=torch.int32, device=data.device)
    call(load_library().dpl_pair_ones, *data.head(row_index), t['col'].data_ptr(), t['col_off'].data_ptr(), t['m'].data_ptr(),
         t['row_off'].data_ptr(), t['n'].data_ptr(), t['out_off'].data_ptr(), len(blocks), t['unit_blk'].data_ptr(),
         t['unit_ti'].data_ptr(), t['unit_tj'].data_ptr(), t['unit_row0'].data_ptr(), len(unit['blk']), row_chunk,
         ones.data_ptr(), ones.numel(), _stream(data.device))
    COUNTERS['kernels'] += 2        # (the zeroing kernel and the counting kernel)
    return ones, out_off[:-1]


class KMeansBatch:
    """The k-means of all row-splitting tasks of one generation (header: "k-means", "k-means on float columns").
    ``tasks``: a list of ``(row_off, n, cols, ks, seeds)`` with ``seeds`` an ``[n_restarts, n_clusters]`` array of row
    positions.  uint8 data: ``ks`` the domain sizes of ``cols`` and a centroid ``kmax`` value frequencies per column
    (``dpl_kmeans_*``); float32 data: ``ks`` and ``kmax`` None and a centroid one mean per column (``dpl_kmeansf_*``)."""

    MAX_ITER = 100

    def __init__(self, data: DeviceData, row_index, tasks, n_restarts: int, n_clusters: int, kmax: int = None):
        assert data.is_float == (kmax is None)
        self.data, self.row_index, self.R, self.C, self.T = data, row_index, n_restarts, n_clusters, len(tasks)
        self.kmax = None if kmax is None else max(int(kmax), 2)
        col_off, cols, ks, cent_off, lab_off, item_task, item_p = [0], [], [], [], [], [], []
        n_cent = n_lab = 0
        for t, (row_off, n, tcols, tks, seeds) in enumerate(tasks):
            assert data.is_float == (tks is None)
            cols += list(tcols)
            ks += [] if tks is None else list(tks)
            col_off.append(len(cols))
            cent_off.append(n_cent)
            lab_off.append(n_lab)
            n_cent += n_restarts * n_clusters * len(tcols) * (self.kmax or 1)
            n_lab += n
            item_task += [t] * len(tcols)
            item_p += list(range(len(tcols)))
        self.n_cent, self.n_lab, self.lab_off, self.cent_off = n_cent, n_lab, lab_off, cent_off
        block_task, block_row0 = _row_blocks([t[1] for t in tasks])
        self.n_blocks, self.n_items = len(block_task), len(item_task)
        self.tab = upload(
            data.device, col_off=np.asarray(col_off, np.int32), cols=np.asarray(cols, np.int32),
            **({} if data.is_float else {'ks': np.asarray(ks, np.int32)}),
            row_off=np.asarray([t[0] for t in tasks], np.int64), n=np.asarray([t[1] for t in tasks], np.int32),
            cent_off=np.asarray(cent_off, np.int64), lab_off=np.asarray(lab_off, np.int64),
            seeds=np.concatenate([np.asarray(t[4], np.int32).reshape(-1) for t in tasks]),
            block_task=block_task, block_row0=block_row0,
            item_task=np.asarray(item_task, np.int32), item_p=np.asarray(item_p, np.int32))

    def run(self):
        """``(inertia [T, R] float64, sizes [T, R, C] int32, labels [R, n_lab] device uint8, iterations)``; the centroids
        stay in ``self.cent``."""
        lib, d, p = load_library(), self.data, {k: v.data_ptr() for k, v in self.tab.items()}
        init, assign, update, inertia_of = (getattr(lib, ('dpl_kmeansf_' if d.is_float else 'dpl_kmeans_') + name)
                                            for name in ('init', 'assign', 'update', 'inertia'))
        ks, kmax = (() if d.is_float else (p['ks'],)), (() if d.is_float else (self.kmax,))
        dev, st = d.device, _stream(d.device)
        head = d.head(self.row_index)
        cent = self.cent = torch.empty(self.n_cent, dtype=torch.float64, device=dev)
        labels = torch.empty((self.R, self.n_lab), dtype=torch.uint8, device=dev)
        changed = torch.zeros(self.MAX_ITER, dtype=torch.int32, device=dev)
        COUNTERS['kernels'] += 1        # (the fill of `changed`)
        call(init, *head, p['col_off'], p['cols'], p['row_off'], p['n'], p['cent_off'], p['seeds'], self.T, self.R,
             self.C, *kmax, cent.data_ptr(), self.n_cent, st)
        COUNTERS['kernels'] += 1
        iterations = 0
        for it in range(self.MAX_ITER):
            call(assign, *head, p['col_off'], p['cols'], *ks, p['row_off'], p['n'], p['cent_off'], p['lab_off'],
                 p['block_task'], p['block_row0'], self.n_blocks, self.R, self.C, *kmax, cent.data_ptr(), labels.data_ptr(),
                 self.n_lab, 1 if it == 0 else 0, changed[it:].data_ptr(), st)
            COUNTERS['lloyd_kernels'] += 1
            iterations = it + 1
            if int(read(changed[it:it + 1], lloyd=True)[0]) == 0 or it == self.MAX_ITER - 1:
                break
            call(update, *head, p['col_off'], p['cols'], p['row_off'], p['n'], p['cent_off'], p['lab_off'],
                 p['item_task'], p['item_p'], self.n_items, self.R, self.C, *kmax, labels.data_ptr(), self.n_lab,
                 cent.data_ptr(), st)
            COUNTERS['lloyd_kernels'] += 1
        inertia = torch.empty((self.T, self.R), dtype=torch.float64, device=dev)
        sizes = torch.empty((self.T, self.R, self.C), dtype=torch.int32, device=dev)
        call(inertia_of, *head, p['col_off'], p['cols'], *ks, p['row_off'], p['n'], p['cent_off'], p['lab_off'], self.T,
             self.R, self.C, *kmax, cent.data_ptr(), labels.data_ptr(), self.n_lab, inertia.data_ptr(), sizes.data_ptr(), st)
        COUNTERS['kernels'] += 1
        return read(inertia), read(sizes), labels, iterations


#: the Gaussian-mixture row split: scikit-learn's GaussianMixture(covariance_type='full', n_init=3) defaults
GMM_N_INIT, GMM_TOL, GMM_REG_COVAR, GMM_MAX_ITER = 3, 1e-3, 1e-6, 100
#: rows of one unit of ``dpl_gmm_mstats``, and the units whose partial sums fit in 256 MiB
GMM_ROW_CHUNK = 1024
GMM_MAX_UNITS = (256 << 20) // (8 * CONSTANTS['DPL_GMM_PARTIAL'])
#: whether the products of ``dpl_gmm_mstats`` run on v_mfma_f64_16x16x4_f64 (else on the VALU): see DESIGN.md 14.5
GMM_USE_MFMA = True


def gmm_features(cols, ks):
    """``(feat_col, feat_val)`` of a task's columns: a column with K <= 2 (or a float column, ``ks`` None) is one feature
    (value -1: the column's value), a column with K > 2 is K indicator features (header, "Gaussian-mixture row splits")."""
    fc, fv = [], []
    for p, col in enumerate(cols):
        k = 1 if ks is None else int(ks[p])
        if k <= 2:
            fc.append(int(col))
            fv.append(-1)
        else:
            fc += [int(col)] * k
            fv += list(range(k))
    return fc, fv


def gmm_m_step(stats: np.ndarray, pivot: np.ndarray, n: int) -> np.ndarray:
    """The parameters ``[C, 1 + F + F * F]`` (``k_c``, ``mu_c``, ``L_c^-1``: the layout ``dpl_gmm_estep`` takes) from the
    moments ``stats [C, 1 + F + F * F]`` about ``pivot [C, F]`` over ``n`` rows: the M-step of DESIGN.md 14.5 with the
    covariance as ``M / N_c - (mu - p)(mu - p)^T + 1e-6 I`` from the LOWER triangle of ``M``.  ValueError when a covariance
    has no Cholesky factor (scikit-learn's rule)."""
    C, F = pivot.shape
    out = np.zeros((C, 1 + F + F * F))
    for c in range(C):
        n_c = stats[c, 0] + 10.0 * np.finfo(np.float64).eps
        d = stats[c, 1:1 + F] / n_c
        low = np.tril(stats[c, 1 + F:].reshape(F, F))
        sigma = (low + np.tril(low, -1).T) / n_c - np.outer(d, d)
        sigma[np.diag_indices(F)] += GMM_REG_COVAR
        try:
            chol = np.linalg.cholesky(sigma)
        except np.linalg.LinAlgError:
            raise ValueError("Fitting the mixture model failed because some components have ill-defined empirical covariance "
                             "(for instance caused by singleton or collapsed samples): use fewer components") from None
        out[c, 0] = np.log(n_c / n) - 0.5 * F * np.log(2.0 * np.pi) - np.sum(np.log(np.diag(chol)))
        out[c, 1:1 + F] = pivot[c] + d
        out[c, 1 + F:] = np.tril(np.linalg.inv(chol)).reshape(-1)
    return out


class GmmBatch:
    """The Gaussian-mixture EM of all row-splitting tasks of one generation, ``GMM_N_INIT`` initialisations each (header:
    "Gaussian-mixture row splits"; the definition: DESIGN.md 14.5).  ``tasks`` as for :class:`KMeansBatch`, ``seeds`` an
    ``[GMM_N_INIT, n_comp]`` array.  A PAIR is ``(task, initialisation)``.  ``launch`` is one E-step and / or one moments
    pass over listed pairs; ``run`` is the whole loop."""

    def __init__(self, data: DeviceData, row_index, tasks, n_comp: int, kmax: int = None):
        self.data, self.row_index, self.tasks, self.C, self.T, self.R = data, row_index, tasks, int(n_comp), len(tasks), GMM_N_INIT
        self.kmax = kmax
        feat_off, fc, fv, lab_off, n_lab = [], [], [], [], 0
        for row_off, n, cols, ks, _ in tasks:
            c, v = gmm_features(cols, ks)
            feat_off.append(len(fc))
            fc, fv = fc + c, fv + v
            lab_off.append(n_lab)
            n_lab += int(n)
        self.fs = [b - a for a, b in zip(feat_off, feat_off[1:] + [len(fc)])]
        self.feat_off, self.feat_col, self.feat_val, self.lab_off, self.n_lab = feat_off, fc, fv, lab_off, n_lab
        self.ns = [int(t[1]) for t in tasks]
        self.tab = upload(data.device, 'gmm_uploads', row_off=np.asarray([t[0] for t in tasks], np.int64),
                          n=np.asarray(self.ns, np.int32), lab_off=np.asarray(lab_off, np.int64),
                          feat_off=np.asarray(feat_off, np.int32), f=np.asarray(self.fs, np.int32),
                          feat_col=np.asarray(fc, np.int32), feat_val=np.asarray(fv, np.int32))
        dev = data.device
        self.resp = torch.empty((self.R, n_lab, self.C), dtype=torch.float64, device=dev)
        self.labels = torch.empty((self.R, n_lab), dtype=torch.uint8, device=dev)
        self.lse = torch.empty((self.R, n_lab), dtype=torch.float64, device=dev)

    def per(self, t):
        return 1 + self.fs[t] + self.fs[t] * self.fs[t]

    def launch(self, e_pairs, m_pairs, par, row_chunk: int = GMM_ROW_CHUNK, max_units: int = GMM_MAX_UNITS, mfma: bool = None):
        """One E-step over the pairs ``e_pairs`` and one moments pass over ``m_pairs`` (lists of ``(task, init)``; either
        may be empty), under the parameters ``par[(task, init)]`` (``[C, 1 + F + F * F]``: the E-step reads all of it, the
        moments pass its means as the pivot): ONE upload of parameters and tables.  Returns ``(out, stat_off, partials)``:
        ``out`` one device float64 tensor holding the summed ``lse`` of ``e_pairs`` and then, for ``m_pairs[i]`` at
        ``len(e_pairs) + stat_off[i]``, its ``[C, 1 + F + F * F]`` moments."""
        lib, d, C = load_library(), self.data, self.C
        listed = list(dict.fromkeys(list(e_pairs) + list(m_pairs)))
        par_off, at = {}, 0
        for a in listed:
            par_off[a] = at
            at += C * self.per(a[0])
        flat = np.concatenate([np.asarray(par[a], np.float64).reshape(-1) for a in listed])
        assert len(flat) == at
        stat_off = np.concatenate([[0], np.cumsum([C * self.per(t) for t, _ in m_pairs])]).astype(np.int64)
        block_pair, block_row0 = _row_blocks([self.ns[t] for t, _ in e_pairs])
        groups = []                 # (pair position, component, i0, j0) of the moments pass, tile pairs i0 <= j0
        for a, (t, _) in enumerate(m_pairs):
            for c in range(C):
                for i0 in range(0, self.fs[t], CONSTANTS['DPL_GRAM_TILE']):
                    for j0 in range(i0, self.fs[t], CONSTANTS['DPL_GRAM_TILE']):
                        groups.append((a, c, i0, j0))
        calls, g = [], 0
        while g < len(groups):
            unit, group, n_units = {key: [] for key in ('pair', 'comp', 'i0', 'j0', 'row0', 'rows')}, {'unit0': [], 'units': []}, 0
            while g < len(groups):
                a, c, i0, j0 = groups[g]
                n = self.ns[m_pairs[a][0]]
                chunks = -(-n // row_chunk)
                if chunks > max_units:
                    raise HipError("gmm: a task of {} rows needs {} partial sums per tile, over the 256 MiB of one call"
                                   .format(n, chunks))
                if n_units + chunks > max_units:
                    break
                group['unit0'].append(n_units)
                group['units'].append(chunks)
                for k in range(chunks):
                    for key, v in zip(('pair', 'comp', 'i0', 'j0', 'row0', 'rows'),
                                      (a, c, i0, j0, k * row_chunk, min(row_chunk, n - k * row_chunk))):
                        unit[key].append(v)
                n_units += chunks
                g += 1
            calls.append((unit, group, n_units))
        tables = dict(par=flat)
        if e_pairs:
            tables.update(e_task=np.asarray([t for t, _ in e_pairs], np.int32), e_init=np.asarray([i for _, i in e_pairs], np.int32),
                          e_par=np.asarray([par_off[a] for a in e_pairs], np.int64), block_pair=block_pair, block_row0=block_row0)
        if m_pairs:
            tables.update(m_task=np.asarray([t for t, _ in m_pairs], np.int32), m_init=np.asarray([i for _, i in m_pairs], np.int32),
                          m_par=np.asarray([par_off[a] for a in m_pairs], np.int64), m_stat=stat_off[:-1].copy())
        for k, (unit, group, _) in enumerate(calls):
            tables.update({'u{}_{}'.format(k, key): np.asarray(v, np.int32) for key, v in list(unit.items()) + list(group.items())})
        up = upload(d.device, 'gmm_uploads', **tables)
        p, q = {k: v.data_ptr() for k, v in self.tab.items()}, {k: v.data_ptr() for k, v in up.items()}
        head = (d.x.data_ptr(), int(d.is_float)) + d.head(self.row_index)[1:]
        task = (p['row_off'], p['n'], p['lab_off'], p['feat_off'], p['f'], p['feat_col'], p['feat_val'])
        out = torch.empty(len(e_pairs) + int(stat_off[-1]), dtype=torch.float64, device=d.device)
        st = _stream(d.device)
        if e_pairs:
            call(lib.dpl_gmm_estep, *head, *task, q['e_task'], q['e_init'], q['e_par'], len(e_pairs), q['block_pair'],
                 q['block_row0'], len(block_pair), self.R, C, q['par'], self.resp.data_ptr(), self.labels.data_ptr(),
                 self.lse.data_ptr(), self.n_lab, out.data_ptr(), st)
            COUNTERS['gmm_kernels'] += 2
        partials = []
        for k, (unit, group, n_units) in enumerate(calls):
            partial = torch.empty(n_units * CONSTANTS['DPL_GMM_PARTIAL'], dtype=torch.float64, device=d.device)
            u = {key: q['u{}_{}'.format(k, key)] for key in list(unit) + list(group)}
            call(lib.dpl_gmm_mstats, *head, *task, q['m_task'], q['m_init'], q['m_par'], q['m_stat'], len(m_pairs), u['pair'],
                 u['comp'], u['i0'], u['j0'], u['row0'], u['rows'], n_units, u['unit0'], u['units'], len(group['units']), C,
                 q['par'], self.resp.data_ptr(), self.n_lab, int(GMM_USE_MFMA if mfma is None else mfma), partial.data_ptr(),
                 out.data_ptr() + 8 * len(e_pairs), st)
            COUNTERS['gmm_kernels'] += 2
            partials.append(partial)
        return out, stat_off[:-1], partials

    def pivots(self, cent: np.ndarray, km):
        """``{(task, init): [C, F]}``: the k-means centroids as feature vectors."""
        out = {}
        for t, (_, _, cols, ks, _) in enumerate(self.tasks):
            width = len(cols) * (km.kmax or 1)
            for i in range(self.R):
                cen = cent[km.cent_off[t] + i * self.C * width:][:self.C * width].reshape(self.C, len(cols), -1)
                feats = []
                for p in range(len(cols)):
                    k = 1 if ks is None else int(ks[p])
                    feats += [cen[:, p, 0 if ks is None else 1]] if k <= 2 else [cen[:, p, v] for v in range(k)]
                out[(t, i)] = np.stack(feats, axis=1)
        return out

    def run(self):
        """``(best [T] winning initialisation, lower [T, R] bounds, sizes [T, R, C] int64, labels [R, n_lab] device uint8,
        EM iterations)``; ``self.host_labels`` is the host copy of the labels the sizes were counted from: the Lloyd initialisations, then the loop of DESIGN.md 14.5 with every pair advancing together and
        a converged pair leaving the launch tables after the label pass under its final parameters."""
        C, R = self.C, self.R
        km = KMeansBatch(self.data, self.row_index, self.tasks, R, C, self.kmax)
        _, _, km_labels, _ = km.run()
        self.km_labels = km_labels
        self.resp.zero_()
        self.resp.scatter_(2, km_labels.long().unsqueeze(-1), 1.0)       # the hard labels as 0/1 responsibilities
        pivot = self.pivots(read(km.cent, gmm=True), km)
        pairs = [(t, i) for t in range(self.T) for i in range(R)]
        # the pivot of the first moments pass is the centroid (only the means of `par` are read there)
        par = {a: np.concatenate([np.zeros((C, 1)), pivot[a], np.zeros((C, self.fs[a[0]] ** 2))], axis=1) for a in pairs}
        out, stat_off, _ = self.launch([], pairs, par)
        host = read(out, gmm=True)
        for k, a in enumerate(pairs):
            stats = host[stat_off[k]:stat_off[k] + C * self.per(a[0])].reshape(C, -1)
            par[a] = gmm_m_step(stats, pivot[a], self.ns[a[0]])
        lower = {a: -np.inf for a in pairs}
        active, final, iterations = list(pairs), [], 0
        while active or final:
            listed = active + final
            out, stat_off, _ = self.launch(listed, active, par)
            host = read(out, gmm=True)
            final, still = [], []
            iterations += 1 if active else 0
            for k, a in enumerate(active):
                t = a[0]
                bound = host[k] / float(self.ns[t])
                stats = host[len(listed) + stat_off[k]:][:C * self.per(t)].reshape(C, -1)
                par[a] = gmm_m_step(stats, par[a][:, 1:1 + self.fs[t]], self.ns[t])
                change = bound - lower[a]
                lower[a] = bound
                if abs(change) < GMM_TOL or iterations == GMM_MAX_ITER:
                    final.append(a)
                else:
                    still.append(a)
            active = still
        bounds = np.array([[lower[(t, i)] for i in range(R)] for t in range(self.T)])
        labels = self.host_labels = read(self.labels, gmm=True)
        sizes = np.array([[np.bincount(labels[i, self.lab_off[t]:self.lab_off[t] + self.ns[t]], minlength=C)[:C]
                           for i in range(R)] for t in range(self.T)], np.int64)
        return np.argmax(bounds, axis=1), bounds, sizes, self.labels, iterations


# ---- continuous data (the last section of the header) ---------------------------------------------------------------------
def column_moments(data: DeviceData, row_index, item_col, item_row_off, item_n) -> torch.Tensor:
    """``[n_items, 2]`` float64: mean and population variance of every item (``dpl_column_moments``)."""
    assert data.is_float
    t = _items(data.device, item_col, item_row_off, item_n)
    moments = torch.empty((len(item_col), 2), dtype=torch.float64, device=data.device)
    call(load_library().dpl_column_moments, *data.head(row_index), t['col'].data_ptr(), t['off'].data_ptr(), t['n'].data_ptr(),
         len(item_col), moments.data_ptr(), _stream(data.device))
    COUNTERS['kernels'] += 1
    return moments


def _sorted_items(data: DeviceData, row_index, t, n_items: int, total: int) -> torch.Tensor:
    """The values of all items of the tables ``t`` (``col``, ``off``, ``n``, ``out``), item major, each item's in
    non-decreasing order: gathered and sorted on the device with ``torch.sort`` (by value, then stably by item); no row
    is sorted on the host."""
    item_of = torch.repeat_interleave(torch.arange(n_items, device=data.device), t['n'].long(), output_size=total)
    pos = torch.arange(total, device=data.device) - t['out'][item_of]
    rows = row_index[t['off'][item_of] + pos].long()
    values = data.x[t['col'][item_of].long() * data.n_rows + rows]
    by_value, order = torch.sort(values, stable=True)
    _, by_item = torch.sort(item_of[order], stable=True)
    return by_value[by_item].contiguous()


def ecdf_ranks(data: DeviceData, row_index, item_col, item_row_off, item_n):
    """``(ranks, out_off)``: the int32 "max" ranks of every item, item i at ``ranks[out_off[i] : out_off[i] + item_n[i]]``
    in segment order (``dpl_ecdf_ranks``).  The values of all items are gathered and sorted on the device with
    ``torch.sort`` (by value, then stably by item); no row is sorted on the host."""
    assert data.is_float
    lib = load_library()
    n_items = len(item_col)
    out_off = np.concatenate([[0], np.cumsum(np.asarray(item_n, np.int64))]).astype(np.int64)
    total = int(out_off[-1])
    block_item, block_row0 = _row_blocks(item_n)
    t = _items(data.device, item_col, item_row_off, item_n, out=out_off[:-1].copy(), bi=block_item, br=block_row0)
    in_order = _sorted_items(data, row_index, t, n_items, total)
    ranks = torch.empty(total, dtype=torch.int32, device=data.device)
    call(lib.dpl_ecdf_ranks, *data.head(row_index), t['col'].data_ptr(), t['off'].data_ptr(), t['n'].data_ptr(),
         t['out'].data_ptr(), n_items, t['bi'].data_ptr(), t['br'].data_ptr(), len(block_item), in_order.data_ptr(),
         ranks.data_ptr(), total, _stream(data.device))
    COUNTERS['kernels'] += 1
    return ranks, out_off[:-1]


#: rows of one unit of ``dpl_rdc_gram``, and the units whose partial sums fit in 256 MiB
GRAM_ROW_CHUNK = 1024
GRAM_MAX_UNITS = (256 << 20) // (8 * CONSTANTS['DPL_GRAM_PARTIAL'])
#: whether the products of ``dpl_rdc_gram`` run on v_mfma_f64_16x16x4_f64 (else on the VALU): picked by measurement
GRAM_USE_MFMA = True


def rdc_gram(ranks: torch.Tensor, tasks, k: int, w: np.ndarray, b: np.ndarray, row_chunk: int = GRAM_ROW_CHUNK,
             max_units: int = GRAM_MAX_UNITS, mfma: bool = None):
    """The column sums and raw Gram matrices of the random features of every task (``dpl_rdc_gram``).  ``tasks``: a list of
    ``(n, m, rank_off)``: task t has its ``m`` rank arrays of ``n`` rows at ``ranks[rank_off ...]``; ``w``, ``b``: the
    float32 draws of all tasks, ``m * k`` each, one after the other.  Returns a dict: ``G`` (device float64, task t's
    ``[F, F]`` matrix at ``g_off[t]``), ``S`` (device float64, task t's ``[F]`` sums at ``feat_off[t]``), ``g_off``,
    ``feat_off`` and ``partials`` (the scratch of every call).  The tile pairs are split over calls so that the partial
    sums of one call stay under 256 MiB."""
    lib = load_library()
    device, tile = ranks.device, CONSTANTS['DPL_GRAM_TILE']
    k = int(k)
    fs = [int(m) * k for _, m, _ in tasks]
    feat_off = np.concatenate([[0], np.cumsum(fs)]).astype(np.int64)
    g_off = np.concatenate([[0], np.cumsum([f * f for f in fs])]).astype(np.int64)
    w, b = np.ascontiguousarray(w, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1)
    assert len(w) == len(b) == int(feat_off[-1])
    tt = upload(device, n=np.asarray([t[0] for t in tasks], np.int32), f=np.asarray(fs, np.int32),
                rank_off=np.asarray([t[2] for t in tasks], np.int64), feat_off=feat_off[:-1].copy(), g_off=g_off[:-1].copy(),
                w=w, b=b)
    G = torch.empty(int(g_off[-1]), dtype=torch.float64, device=device)
    S = torch.empty(int(feat_off[-1]), dtype=torch.float64, device=device)
    groups = []                 # (task, i0, j0) in task order, tile pairs i0 <= j0
    for t, f in enumerate(fs):
        for i0 in range(0, f, tile):
            for j0 in range(i0, f, tile):
                groups.append((t, i0, j0))
    partials, g = [], 0
    while g < len(groups):
        unit, group, n_units = {key: [] for key in ('task', 'i0', 'j0', 'row0', 'rows')}, {'unit0': [], 'units': []}, 0
        while g < len(groups):
            t, i0, j0 = groups[g]
            n = int(tasks[t][0])
            chunks = -(-n // row_chunk)
            if chunks > max_units:
                raise HipError("rdc_gram: a task of {} rows needs {} partial sums per tile, over the 256 MiB of one call"
                               .format(n, chunks))
            if n_units + chunks > max_units:
                break
            group['unit0'].append(n_units)
            group['units'].append(chunks)
            for c in range(chunks):
                for key, v in zip(('task', 'i0', 'j0', 'row0', 'rows'), (t, i0, j0, c * row_chunk, min(row_chunk, n - c * row_chunk))):
                    unit[key].append(v)
            n_units += chunks
            g += 1
        ut = upload(device, **{key: np.asarray(v, np.int32) for key, v in list(unit.items()) + list(group.items())})
        partial = torch.empty(n_units * CONSTANTS['DPL_GRAM_PARTIAL'], dtype=torch.float64, device=device)
        call(lib.dpl_rdc_gram, ranks.data_ptr(), ranks.numel(), tt['w'].data_ptr(), tt['b'].data_ptr(), len(w), k,
             tt['n'].data_ptr(), tt['f'].data_ptr(), tt['rank_off'].data_ptr(), tt['feat_off'].data_ptr(), tt['g_off'].data_ptr(),
             len(tasks), ut['task'].data_ptr(), ut['i0'].data_ptr(), ut['j0'].data_ptr(), ut['row0'].data_ptr(),
             ut['rows'].data_ptr(), n_units, ut['unit0'].data_ptr(), ut['units'].data_ptr(), len(group['units']),
             int(GRAM_USE_MFMA if mfma is None else mfma), partial.data_ptr(), G.data_ptr(), G.numel(), S.data_ptr(), _stream(device))
        COUNTERS['kernels'] += 2
        partials.append(partial)
    return {'G': G, 'S': S, 'g_off': g_off[:-1], 'feat_off': feat_off[:-1], 'fs': fs, 'partials': partials}


# ---- histograms of float columns (the header's last section) ---------------------------------------------------------------
def order_statistics(data: DeviceData, row_index, item_col, item_row_off, item_n, positions) -> torch.Tensor:
    """``[n_items, P]`` float32: for every item its values at the ``P`` positions ``positions[i]`` of its sorted order
    (0 the minimum, ``n - 1`` the maximum), from the device sort of ``ecdf_ranks``.  One upload; the caller reads."""
    assert data.is_float
    n_items = len(item_col)
    out_off = np.concatenate([[0], np.cumsum(np.asarray(item_n, np.int64))]).astype(np.int64)
    at = np.asarray(positions, np.int64).reshape(n_items, -1) + out_off[:-1, None]
    t = _items(data.device, item_col, item_row_off, item_n, out=out_off[:-1].copy(), at=at)
    return _sorted_items(data, row_index, t, n_items, int(out_off[-1]))[t['at']]


def check_bins(item_col, item_bins):
    """ValueError, naming the column, for an item of more than ``DPL_HIST_MAX_BINS`` bins (or of none)."""
    for col, bins in zip(item_col, item_bins):
        if not 1 <= int(bins) <= CONSTANTS['DPL_HIST_MAX_BINS']:
            raise ValueError("column {} has {} histogram bins, at most {} are built (a heavy tail or a tiny quartile range "
                             "against the column's span)".format(int(col), int(bins), CONSTANTS['DPL_HIST_MAX_BINS']))


def hist_codes(data: DeviceData, row_index, item_col, item_row_off, item_n, item_lo, item_hi, item_bins):
    """``(codes, out_off)``: the uint16 bin of every row of every item under numpy's uniform bins ``(lo, hi, bins)``,
    item i at ``codes[out_off[i] : out_off[i] + item_n[i]]`` in segment order (``dpl_hist_codes``).  ValueError before any
    launch for a column over ``DPL_HIST_MAX_BINS``."""
    assert data.is_float
    check_bins(item_col, item_bins)
    n_items = len(item_col)
    out_off = np.concatenate([[0], np.cumsum(np.asarray(item_n, np.int64))]).astype(np.int64)
    total = int(out_off[-1])
    block_item, block_row0 = _row_blocks(item_n)
    t = _items(data.device, item_col, item_row_off, item_n, out=out_off[:-1].copy(), lo=np.asarray(item_lo, np.float32),
               hi=np.asarray(item_hi, np.float32), bins=np.asarray(item_bins, np.int32), bi=block_item, br=block_row0)
    codes = torch.empty(total, dtype=torch.uint16, device=data.device)
    call(load_library().dpl_hist_codes, *data.head(row_index), t['col'].data_ptr(), t['off'].data_ptr(), t['n'].data_ptr(),
         t['out'].data_ptr(), t['lo'].data_ptr(), t['hi'].data_ptr(), t['bins'].data_ptr(), n_items, t['bi'].data_ptr(),
         t['br'].data_ptr(), len(block_item), codes.data_ptr(), total, _stream(data.device))
    COUNTERS['kernels'] += 1
    return codes, out_off[:-1]


def code_counts(codes: torch.Tensor, code_off, item_n, item_bins):
    """``(counts, count_off)``: the int32 histogram of every item's codes, item i's ``item_bins[i]`` counts at
    ``counts[count_off[i] ...]`` (``dpl_code_counts``)."""
    assert codes.dtype == torch.uint16 and codes.is_contiguous()
    check_bins(range(len(item_bins)), item_bins)
    count_off = np.concatenate([[0], np.cumsum(np.asarray(item_bins, np.int64))]).astype(np.int64)
    t = upload(codes.device, code_off=np.asarray(code_off, np.int64), n=np.asarray(item_n, np.int32),
               bins=np.asarray(item_bins, np.int32), count_off=count_off[:-1].copy())
    counts = torch.empty(int(count_off[-1]), dtype=torch.int32, device=codes.device)
    call(load_library().dpl_code_counts, codes.data_ptr(), codes.numel(), t['code_off'].data_ptr(), t['n'].data_ptr(),
         t['bins'].data_ptr(), t['count_off'].data_ptr(), len(item_bins), counts.data_ptr(), counts.numel(), _stream(codes.device))
    COUNTERS['kernels'] += 1
    return counts, count_off[:-1]


def check_cells(col_a, col_b, bins_a, bins_b):
    """ValueError, naming the two columns, for a pair whose joint table has more than ``DPL_HIST_MAX_CELLS`` cells."""
    for ca, cb, ba, bb in zip(col_a, col_b, bins_a, bins_b):
        if int(ba) * int(bb) > CONSTANTS['DPL_HIST_MAX_CELLS']:
            raise ValueError("columns {} and {} have {} and {} histogram bins: a joint table of {} cells, at most {} are built"
                             .format(int(ca), int(cb), int(ba), int(bb), int(ba) * int(bb), CONSTANTS['DPL_HIST_MAX_CELLS']))


def pair_g_codes(codes: torch.Tensor, off_a, off_b, n, bins_a, bins_b, col_a=None, col_b=None) -> torch.Tensor:
    """``[n_pairs]`` float64 G statistics of pairs of coded columns (``dpl_pair_g_codes``); ``col_a``, ``col_b`` name the
    columns in the ValueError raised, before any launch, for a table over ``DPL_HIST_MAX_CELLS``."""
    assert codes.dtype == torch.uint16 and codes.is_contiguous()
    bins_a, bins_b = np.asarray(bins_a, np.int32), np.asarray(bins_b, np.int32)
    check_bins(range(len(bins_a)) if col_a is None else col_a, bins_a)
    check_bins(range(len(bins_b)) if col_b is None else col_b, bins_b)
    check_cells(range(len(bins_a)) if col_a is None else col_a, range(len(bins_b)) if col_b is None else col_b, bins_a, bins_b)
    t = upload(codes.device, oa=np.asarray(off_a, np.int64), ob=np.asarray(off_b, np.int64), n=np.asarray(n, np.int32),
               ba=bins_a, bb=bins_b)
    out = torch.empty(len(bins_a), dtype=torch.float64, device=codes.device)
    call(load_library().dpl_pair_g_codes, codes.data_ptr(), codes.numel(), t['oa'].data_ptr(), t['ob'].data_ptr(),
         t['n'].data_ptr(), t['ba'].data_ptr(), t['bb'].data_ptr(), len(bins_a), int((bins_a + bins_b).max()),
         int((bins_a.astype(np.int64) * bins_b).max()), out.data_ptr(), _stream(codes.device))
    COUNTERS['kernels'] += 1
    return out
