"""The cutset-network entry points of ``libdeeprob_clt.so`` (``dpc_cnet_*`` and ``dpc_cut_*`` of
``include/deeprob_clt.h``), on top of the binding of ``deeprob.hip.clt``: one library, one header, one loader.

:class:`Generation` is one level of the level-synchronous learner -- the row segments of its tasks, their bit planes,
counts, scores and the partition into the next level; :class:`DeviceCNet` holds a fitted model as one concatenated
table, uploaded in one copy; :func:`log_likelihood`, :func:`mpe`, :func:`sample` and :func:`marginals` are the queries
(``dpc_cnet_log_likelihood``, the ``dpc_cnq_*`` entries -- exact MPE and exact conditional sampling -- and ``dpc_mar_cnet``,
the exact posterior marginals: one launch per piece of the batch).  Everything takes and returns device tensors; there is
no CPU fallback.
"""
import numpy as np
import torch

from deeprob import hip
from deeprob.hip import HipError, clt
from deeprob.hip.clt import DPC_MAX_D, call, load_library

#: int32 counts of scratch per launch of the segmented pair counts (256 MiB): a generation is counted and scored in
#: chunks of COUNT_INTS / D^2 tasks
COUNT_INTS = 1 << 26
#: bytes of scratch per query launch (128 MiB): a long batch is evaluated in pieces
WORK_BYTES = 1 << 27
MAX_CHUNK_TASKS = 65535         # (grid.z of the count kernel)


def chunk_tasks(d: int) -> int:
    """Tasks per chunk of a generation for ``d`` columns: at least 1."""
    return max(1, min(MAX_CHUNK_TASKS, COUNT_INTS // (d * d)))


def query_rows(row_bytes: int) -> int:
    """Rows per query launch for ``row_bytes`` of scratch per row: a multiple of 64, at least 1024."""
    return max(1024, WORK_BYTES // row_bytes // 64 * 64)


class Generation:
    """The tasks of one depth over the rows ``x`` ``[N, D]``: ``rows`` int32 ``[sum(sizes)]`` on the device, task t owning
    the next ``sizes[t]`` of them.  The offsets go up in one copy."""

    def __init__(self, x: torch.Tensor, rows: torch.Tensor, sizes):
        x = hip.require_device_f32(x, 'data')
        sizes = np.asarray(sizes, np.int64)
        if x.dim() != 2 or not 1 <= x.shape[1] <= DPC_MAX_D or not 1 <= x.shape[0] < 2 ** 31:
            raise ValueError("expected data [1 .. 2^31 - 1, 1 .. {}], got {}".format(DPC_MAX_D, tuple(x.shape)))
        if sizes.ndim != 1 or len(sizes) < 1 or (sizes < 0).any() or int(sizes.sum()) >= 2 ** 31:
            raise ValueError("expected the sizes of one or more tasks, fewer than 2^31 rows in all")
        if rows.dtype != torch.int32 or rows.device != x.device or rows.dim() != 1 or rows.shape[0] != int(sizes.sum()) \
                or not rows.is_contiguous():
            raise ValueError("expected rows as {} int32 on '{}'".format(int(sizes.sum()), x.device))
        self.x, self.rows, self.sizes = x, rows, sizes
        self.n_tasks, self.d = len(sizes), int(x.shape[1])
        self.seg_off = np.concatenate([[0], np.cumsum(sizes)])
        self.word_off = np.concatenate([[0], np.cumsum((sizes + 63) // 64)])
        self.n_words = int(self.word_off[-1])
        offs = torch.from_numpy(np.concatenate([self.seg_off, self.word_off]).astype(np.int32)).to(x.device)
        self._seg, self._word = offs[:self.n_tasks + 1], offs[self.n_tasks + 1:]
        self._st = hip.stream_ptr(x.device)
        self.planes = None

    def pack(self) -> torch.Tensor:
        """``[D, n_words]`` int64 bit planes of the generation's rows (``dpc_cnet_gather_pack``)."""
        planes = torch.empty((self.d, self.n_words), dtype=torch.int64, device=self.x.device)
        call(load_library().dpc_cnet_gather_pack, self.x.data_ptr(), self.x.shape[0], self.d, self.rows.data_ptr(),
             self._seg.data_ptr(), self._word.data_ptr(), self.n_tasks, self.n_words, planes.data_ptr(), self._st)
        self.planes = planes
        return planes

    def counts(self, t0: int, n: int) -> torch.Tensor:
        """``[n, D, D]`` int32 co-occurrence counts of the tasks ``t0 .. t0 + n`` (``dpc_cnet_pair_counts``)."""
        assert self.planes is not None and 0 <= t0 and n >= 1 and t0 + n <= self.n_tasks
        ones = torch.empty((n, self.d, self.d), dtype=torch.int32, device=self.x.device)
        call(load_library().dpc_cnet_pair_counts, self.planes.data_ptr(), self.n_words, self.d,
             self._word[t0:].data_ptr(), n, ones.data_ptr(), self._st)
        return ones

    def cut_counts(self, entry_task, entry_col) -> torch.Tensor:
        """``[E, D, D]`` int32: for entry e the co-occurrence counts of the rows of task ``entry_task[e]`` with
        ``x[entry_col[e]] = 1`` (``dpc_cut_pair_counts``); one launch for at most ``MAX_CHUNK_TASKS`` entries, the table in
        one copy.  An entry costs as many ints as a task: size the entry chunks with :func:`chunk_tasks`."""
        entry_task, entry_col = np.asarray(entry_task, np.int64), np.asarray(entry_col, np.int64)
        e = len(entry_task)
        if entry_task.shape != (e,) or entry_col.shape != (e,) or not 1 <= e <= MAX_CHUNK_TASKS:
            raise ValueError("expected 1 .. {} entries, a task and a column each".format(MAX_CHUNK_TASKS))
        if (entry_task < 0).any() or (entry_task >= self.n_tasks).any() or (entry_col < 0).any() or (entry_col >= self.d).any():
            raise ValueError("an entry names a task outside 0 .. {} or a column outside 0 .. {}".format(self.n_tasks - 1,
                                                                                                        self.d - 1))
        assert self.planes is not None
        table = torch.from_numpy(np.concatenate([entry_task, entry_col]).astype(np.int32)).to(self.x.device)
        ones1 = torch.empty((e, self.d, self.d), dtype=torch.int32, device=self.x.device)
        call(load_library().dpc_cut_pair_counts, self.planes.data_ptr(), self.n_words, self.d, self._word.data_ptr(),
             self.n_tasks, table[:e].data_ptr(), table[e:].data_ptr(), e, ones1.data_ptr(), self._st)
        return ones1

    def scores(self, ones: torch.Tensor, t0: int, active, alpha: float):
        """``(gains [n, D] float64, stats [n, 2] float64, best [n, 2] int32)`` of the tasks ``t0 .. t0 + n`` from their
        counts (``dpc_cnet_scores``); ``active``: ``[n, D]`` bool / uint8, numpy or on the device."""
        n = ones.shape[0]
        if not isinstance(active, torch.Tensor):
            active = torch.from_numpy(np.ascontiguousarray(active, np.uint8))
        active = active.to(device=self.x.device, dtype=torch.uint8).contiguous()
        assert ones.shape == (n, self.d, self.d) and active.shape == (n, self.d) and t0 + n <= self.n_tasks
        dev = self.x.device
        gains = torch.empty((n, self.d), dtype=torch.float64, device=dev)
        stats = torch.empty((n, 2), dtype=torch.float64, device=dev)
        best = torch.empty((n, 2), dtype=torch.int32, device=dev)
        call(load_library().dpc_cnet_scores, ones.data_ptr(), self._seg[t0:].data_ptr(), active.data_ptr(), n, self.d,
             float(alpha), gains.data_ptr(), stats.data_ptr(), best.data_ptr(), self._st)
        return gains, stats, best

    def partition(self, cut):
        """``(rows_out int32, child_n [T, 2] int32)``: the segments of the tasks with ``cut[t] >= 0`` split stably by that
        column, zeros first, laid out back to back in task order (``dpc_cnet_partition``)."""
        cut = np.asarray(cut, np.int64)
        if cut.shape != (self.n_tasks,) or (cut < -1).any() or (cut >= self.d).any():
            raise ValueError("expected one cut column (or -1) per task")
        assert self.planes is not None
        moved = np.where(cut >= 0, self.sizes, 0)
        out_off = np.concatenate([[0], np.cumsum(moved)[:-1]])
        dev = self.x.device
        args = torch.from_numpy(np.concatenate([cut, out_off]).astype(np.int32)).to(dev)
        rows_out = torch.empty(int(moved.sum()), dtype=torch.int32, device=dev)
        child_n = torch.empty((self.n_tasks, 2), dtype=torch.int32, device=dev)
        call(load_library().dpc_cnet_partition, self.planes.data_ptr(), self.n_words, self.rows.data_ptr(),
             self._seg.data_ptr(), self._word.data_ptr(), args[:self.n_tasks].data_ptr(), args[self.n_tasks:].data_ptr(),
             self.n_tasks, rows_out.data_ptr(), child_n.data_ptr(), self._st)
        return rows_out, child_n


class DeviceCNet:
    """A cutset network over ``d`` columns as the tables of ``dpc_cnet_log_likelihood`` and of the ``dpc_cnq_*`` queries
    (``node_parent`` ``[M]``: ``2 * parent + side``, -1 at the root, is derived here), in one host-to-device copy.

    ``node_col`` ``[M]``: the cut column of node k, -1 at a leaf; ``node_child`` ``[M, 2]``: its children (at a leaf,
    ``[leaf number, -1]``); ``node_logw`` ``[M, 2]`` float64; ``leaves``: per leaf number ``(cols, bfs, parent, params)``,
    ``cols`` the column of every position of the leaf's scope.  Checked on the host -- the kernel indexes device memory
    with these tables: node 0 roots one binary tree that reaches every node once, and along every path the cut columns and
    the leaf's columns are distinct columns of ``0 .. d - 1``.  ``covered`` records whether every path also accounts for
    EVERY column, as a cut or in its leaf's scope -- learned networks always do; :func:`marginals` needs it."""

    def __init__(self, d, node_col, node_child, node_logw, leaves, device):
        node_col, node_child = np.asarray(node_col, np.int64), np.asarray(node_child, np.int64)
        node_logw = np.ascontiguousarray(node_logw, np.float64)
        m = len(node_col)
        if not 1 <= d <= DPC_MAX_D:
            raise HipError("a model of {} variables is outside 1..{} (DPC_MAX_D)".format(d, DPC_MAX_D))
        if m < 1 or node_child.shape != (m, 2) or node_logw.shape != (m, 2):
            raise ValueError("the node tables do not describe one cutset network")
        ints, params, meta = [], [], []
        n_ints = n_params = 0
        for cols, bfs, parent, par in leaves:
            bfs, parent, par = clt.check_tree(bfs, parent, par)
            cols = np.asarray(cols, np.int64)
            if cols.shape != (len(parent),):
                raise ValueError("the node tables do not describe one cutset network")
            off, idx = clt.children_csr(bfs, parent)
            ints += [cols.astype(np.int32), bfs.astype(np.int32), parent.astype(np.int32), off, idx]
            params.append(par.reshape(-1))
            meta.append((len(parent), n_ints, n_params))
            n_ints, n_params = n_ints + 5 * len(parent), n_params + 4 * len(parent)
        # one walk from the root: every node once, columns distinct along a path
        seen, levels, stack = np.zeros(m, bool), 0, [(0, 1, frozenset(), -1)]
        node_parent = np.full(m, -1, np.int32)
        leaf_seen = np.zeros(len(meta), bool)
        covered = True
        while stack:
            k, level, used, up = stack.pop()
            ok = 0 <= k < m and not seen[k]
            if ok:
                seen[k] = True
                node_parent[k] = up
                levels = max(levels, level)
                col = int(node_col[k])
                if col < 0:
                    l = int(node_child[k, 0])
                    ok = 0 <= l < len(meta) and not leaf_seen[l]
                    if ok:
                        leaf_seen[l] = True
                        cols = leaves[l][0]
                        ok = len(set(int(c) for c in cols)) == len(cols) and all(0 <= int(c) < d and int(c) not in used
                                                                                 for c in cols)
                        covered = covered and len(used) + len(cols) == d
                else:
                    ok = col < d and col not in used
                    stack += [(int(node_child[k, 1]), level + 1, used | {col}, 2 * k + 1),
                              (int(node_child[k, 0]), level + 1, used | {col}, 2 * k)]
            if not ok:
                raise ValueError("the node tables do not describe one cutset network")
        if not seen.all() or not leaf_seen.all():
            raise ValueError("the node tables do not describe one cutset network")
        ints_all = np.concatenate([node_col.astype(np.int32), node_child.astype(np.int32).reshape(-1), node_parent,
                                   np.asarray(meta, np.int32).reshape(-1)] + ints)
        buf = torch.from_numpy(np.concatenate([node_logw.reshape(-1).view(np.uint8), ints_all.view(np.uint8),
                                               np.concatenate(params).view(np.uint8)])).to(device)
        self.d, self.n_nodes, self.levels, self.device, self._buf = int(d), m, levels, buf.device, buf
        self.max_leaf_d = max(k for k, _, _ in meta)
        self.node_logw = buf[:16 * m].view(torch.float64)
        ints_d = buf[16 * m:16 * m + 4 * len(ints_all)].view(torch.int32)
        self.node_col, self.node_child, self.node_parent = ints_d[:m], ints_d[m:3 * m], ints_d[3 * m:4 * m]
        self.leaf_meta, self.leaf_ints = ints_d[4 * m:4 * m + 3 * len(meta)], ints_d[4 * m + 3 * len(meta):]
        self.leaf_params = buf[16 * m + 4 * len(ints_all):].view(torch.float32)
        self.row_bytes = 12 * self.levels + 8 * self.max_leaf_d
        #: scratch per row of ``dpc_cnq_mpe`` / ``dpc_cnq_sample``: one more int32 per level, the leaf carried upward
        self.query_row_bytes = 16 * self.levels + 8 * self.max_leaf_d
        #: scratch per row of ``dpc_mar_cnet``: a second float64 per level (the prefix weight) and the D float64 accumulators
        self.marginals_row_bytes = 20 * self.levels + 8 * self.max_leaf_d + 8 * self.d
        #: whether every root-to-leaf path accounts for every column, as a cut or in the leaf's scope
        self.covered = bool(covered)

    def pointers(self, parent: bool = False):
        """The table arguments of a query in ABI order; ``parent``: with ``node_parent`` (the ``dpc_cnq_*`` entries)."""
        nodes = (self.node_col, self.node_child) + ((self.node_parent,) if parent else ()) + (self.node_logw,)
        return tuple(t.data_ptr() for t in nodes + (self.leaf_meta, self.leaf_ints, self.leaf_params)) \
            + (self.levels, self.max_leaf_d)


def _pieces(model: DeviceCNet, x: torch.Tensor, row_bytes: int, out_shape, want_choice: bool = False):
    """A query over a long batch, in pieces of ``query_rows(row_bytes)`` rows that share one ``work`` buffer: checks ``x`` and
    returns ``(out, choice or None, pieces)``, ``out`` float32 of ``out_shape(b, d)``, ``choice`` ``[B]`` int32 and a piece
    ``(r0, xs, codes, n, work pointer, out pointer, choice pointer or None, stream)`` -- its packed codes and its slices."""
    x = hip.require_device_f32(x, 'x')
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] != model.d:
        raise ValueError("expected inputs [B, {}], got {}".format(model.d, tuple(x.shape)))
    if x.device != model.device:
        raise HipError("x lives on '{}', the model on '{}'".format(x.device, model.device))
    b, d = x.shape
    st = hip.stream_ptr(x.device)
    out = torch.empty(out_shape(b, d), dtype=torch.float32, device=x.device)
    choice = torch.empty(b, dtype=torch.int32, device=x.device) if want_choice else None
    step = query_rows(row_bytes)
    work = torch.empty(row_bytes * min(b, step), dtype=torch.uint8, device=x.device)

    def pieces():
        for r0 in range(0, b, step):
            xs = x[r0:r0 + step]
            yield (r0, xs, clt.pack_query(xs), xs.shape[0], work.data_ptr(), out[r0:r0 + step].data_ptr(),
                   choice[r0:r0 + step].data_ptr() if want_choice else None, st)
    return out, choice, pieces()


def log_likelihood(model: DeviceCNet, x: torch.Tensor) -> torch.Tensor:
    """``[B]`` float32 (``dpc_cnet_log_likelihood``); NaN entries are marginalised."""
    lib = load_library()
    out, _, pieces = _pieces(model, x, model.row_bytes, lambda b, d: b)
    for _, _, codes, n, work, os_, _, st in pieces:
        call(lib.dpc_cnet_log_likelihood, codes.data_ptr(), n, model.d, model.n_nodes, *model.pointers(), work, os_, st)
    return out


def mpe(model: DeviceCNet, x: torch.Tensor, return_choice: bool = False):
    """``[B, D]`` float32: ``x`` with its NaN entries filled by a most probable completion (``dpc_cnq_mpe``, exact: the OR
    nodes are deterministic).  With ``return_choice`` also ``[B]`` int32, the node number of the winning leaf."""
    lib = load_library()
    out, choice, pieces = _pieces(model, x, model.query_row_bytes, lambda b, d: (b, d), return_choice)
    for _, xs, codes, n, work, os_, ch, st in pieces:
        call(lib.dpc_cnq_mpe, xs.data_ptr(), codes.data_ptr(), n, model.d, model.n_nodes, *model.pointers(parent=True), work,
             os_, ch, st)
    return (out, choice) if return_choice else out


def sample(model: DeviceCNet, x: torch.Tensor, seed: int, return_choice: bool = False):
    """``[B, D]`` float32: ``x`` with its NaN entries drawn from the exact posterior given the observed ones
    (``dpc_cnq_sample``); the same seed gives the same bytes: a piece starts its counters at its first row (``row0``).  With
    ``return_choice`` also ``[B]`` int32, the node number of the drawn leaf."""
    lib = load_library()
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out, choice, pieces = _pieces(model, x, model.query_row_bytes, lambda b, d: (b, d), return_choice)
    for r0, xs, codes, n, work, os_, ch, st in pieces:
        call(lib.dpc_cnq_sample, xs.data_ptr(), codes.data_ptr(), n, model.d, model.n_nodes, *model.pointers(parent=True),
             seed, r0, work, os_, ch, st)
    return (out, choice) if return_choice else out


def marginals(model: DeviceCNet, x: torch.Tensor) -> torch.Tensor:
    """``[B, D]`` float32: ``x`` with every NaN entry replaced by ``p(x_j = 1 | the row's observed entries)``, exact
    (``dpc_mar_cnet``); NaN where the row's evidence has probability zero.  A long batch goes in pieces of
    ``query_rows(model.marginals_row_bytes)`` rows.

    :raises ValueError: If a path of the model leaves a column out (``model.covered`` is false): the sum over the leaves
                        would not be a marginal."""
    if not model.covered:
        raise ValueError("marginals need every root-to-leaf path to account for every column, as a cut or in the leaf's "
                         "scope: these tables leave a column out on some path")
    lib = load_library()
    out, _, pieces = _pieces(model, x, model.marginals_row_bytes, lambda b, d: (b, d))
    for _, xs, codes, n, work, os_, _, st in pieces:
        call(lib.dpc_mar_cnet, xs.data_ptr(), codes.data_ptr(), n, model.d, model.n_nodes, *model.pointers(), work, os_, st)
    return out
