"""The XPC entry points of ``libdeeprob_clt.so`` (``dpc_xpc_*`` of ``include/deeprob_clt.h``), on top of the binding of
``deeprob.hip.clt``: one library, one header, one loader.

:class:`Split` is one horizontal split of one or more tasks by a conjunction of binary variables: the histogram of the
rows' codes (``dpc_xpc_code_counts``) and the stable split of every task's rows into its children
(``dpc_xpc_partition``).  It works from the bit planes of the WHOLE training matrix (``deeprob.hip.clt.pack_bits``, packed
once per learner call) through a row-index array, the convention of :class:`deeprob.hip.cnet.Generation`.  Everything takes
and returns device tensors; there is no CPU fallback.
"""
import numpy as np
import torch

from deeprob import hip
from deeprob.hip.clt import DPC_MAX_D, DPC_XPC_CHUNK, DPC_XPC_MAX_CONJ, call, load_library


class Split:
    """The tasks of one split over the ``n`` training rows whose planes are ``planes`` ``[D, (n + 63) / 64]`` int64:
    ``rows`` int32 ``[sum(sizes)]`` on the device, task t owning the next ``sizes[t]`` of them, and its conjunction columns
    ``conj_cols[t]`` (``[T, conj_len]``, ``1 <= conj_len <= DPC_XPC_MAX_CONJ``).  The offsets and columns go up in one
    copy."""

    def __init__(self, planes: torch.Tensor, n: int, rows: torch.Tensor, sizes, conj_cols):
        sizes = np.asarray(sizes, np.int64)
        conj_cols = np.asarray(conj_cols, np.int64)
        if planes.dtype != torch.int64 or planes.dim() != 2 or not planes.is_cuda or not planes.is_contiguous() \
                or not 1 <= planes.shape[0] <= DPC_MAX_D or not 1 <= n < 2 ** 31 or planes.shape[1] != (n + 63) // 64:
            raise ValueError("expected the int64 bit planes [1 .. {}, (n + 63) / 64] of n rows on a HIP device".format(DPC_MAX_D))
        if sizes.ndim != 1 or len(sizes) < 1 or (sizes < 0).any() or int(sizes.sum()) >= 2 ** 31:
            raise ValueError("expected the sizes of one or more tasks, fewer than 2^31 rows in all")
        if conj_cols.ndim != 2 or conj_cols.shape[0] != len(sizes) or not 1 <= conj_cols.shape[1] <= DPC_XPC_MAX_CONJ:
            raise ValueError("expected 1 .. {} conjunction columns per task".format(DPC_XPC_MAX_CONJ))
        if (conj_cols < 0).any() or (conj_cols >= planes.shape[0]).any():
            raise ValueError("a conjunction names a column outside 0 .. {}".format(planes.shape[0] - 1))
        if rows.dtype != torch.int32 or rows.device != planes.device or rows.dim() != 1 \
                or rows.shape[0] != int(sizes.sum()) or not rows.is_contiguous():
            raise ValueError("expected rows as {} int32 on '{}'".format(int(sizes.sum()), planes.device))
        self.planes, self.n, self.rows, self.sizes = planes, int(n), rows, sizes
        self.n_tasks, self.d, self.conj_len = len(sizes), int(planes.shape[0]), int(conj_cols.shape[1])
        self.n_codes = 1 << self.conj_len
        self.seg_off = np.concatenate([[0], np.cumsum(sizes)])
        self.chunk_off = np.concatenate([[0], np.cumsum((sizes + DPC_XPC_CHUNK - 1) // DPC_XPC_CHUNK)])
        self.n_chunks = int(self.chunk_off[-1])
        table = torch.from_numpy(np.concatenate([self.seg_off, self.chunk_off, conj_cols.reshape(-1)]).astype(np.int32))
        table = table.to(planes.device)
        t1 = self.n_tasks + 1
        self._seg, self._chunk, self._cols = table[:t1], table[t1:2 * t1], table[2 * t1:]
        self._st = hip.stream_ptr(planes.device)
        self.chunk_hist = None

    def _head(self):
        return (self.planes.data_ptr(), self.planes.shape[1], self.n, self.d, self.rows.data_ptr(), self._seg.data_ptr(),
                self._chunk.data_ptr(), self._cols.data_ptr(), self.conj_len)

    def counts(self) -> torch.Tensor:
        """``[T, 2^conj_len]`` int32: the rows of every task per code (``dpc_xpc_code_counts``); the per-chunk histograms
        stay on the device for :meth:`partition`."""
        dev = self.planes.device
        self.chunk_hist = torch.empty((self.n_chunks, self.n_codes), dtype=torch.int32, device=dev)
        hist = torch.empty((self.n_tasks, self.n_codes), dtype=torch.int32, device=dev)
        call(load_library().dpc_xpc_code_counts, *self._head(), self.n_tasks, self.n_chunks,
             self.chunk_hist.data_ptr() if self.n_chunks else None, hist.data_ptr(), self._st)
        return hist

    def partition(self, child_of_code, hist) -> torch.Tensor:
        """The rows of every task, child by child, each child's rows in the order they had (``dpc_xpc_partition``): task
        after task, within a task child 0, 1, ...  ``child_of_code``: ``[T, 2^conj_len]`` children ``0 .. 2^conj_len - 1``;
        ``hist``: the counts of :meth:`counts` on the host (they size the children)."""
        child_of_code, hist = np.asarray(child_of_code, np.int64), np.asarray(hist, np.int64)
        shape = (self.n_tasks, self.n_codes)
        if child_of_code.shape != shape or (child_of_code < 0).any() or (child_of_code >= self.n_codes).any():
            raise ValueError("expected one child 0 .. {} per task and code".format(self.n_codes - 1))
        if hist.shape != shape or (hist.sum(axis=1) != self.sizes).any():
            raise ValueError("the counts are not those of these tasks")
        assert self.chunk_hist is not None, "counts() comes first"
        child_n = np.zeros(shape, np.int64)
        for t in range(self.n_tasks):
            np.add.at(child_n[t], child_of_code[t], hist[t])
        out_off = (np.cumsum(child_n.reshape(-1)) - child_n.reshape(-1)).reshape(shape)
        dev = self.planes.device
        table = torch.from_numpy(np.concatenate([child_of_code.reshape(-1), out_off.reshape(-1)]).astype(np.int32)).to(dev)
        k = self.n_tasks * self.n_codes
        rows_out = torch.empty(int(self.sizes.sum()), dtype=torch.int32, device=dev)
        call(load_library().dpc_xpc_partition, *self._head(), self.chunk_hist.data_ptr() if self.n_chunks else None,
             table[:k].data_ptr(), table[k:].data_ptr(), self.n_tasks, self.n_chunks, rows_out.data_ptr(), self._st)
        #: rows of every child, ``[T, 2^conj_len]``: child k of task t owns the next ``child_n[t, k]`` rows of the result
        self.child_n = child_n
        return rows_out
