"""The random partition tree of an XPC (reference spn/utils/partitioning.py) with the rows on the HIP device.

``generate_random_partitioning`` stays a sequential loop on the host and consumes ``random_state`` draw for draw as the
reference does -- ``randint(len(leaves))``, the shuffle of ``uncond_vars`` when not ``sd``, the shuffle of the assignments,
and no draw for a partition that is too small -- so the same ``RandomState`` gives the reference's tree.  What it does NOT
do is touch the data on the host: the rows of every partition are a segment of a row-index array on the device, and a
horizontal split is one ``dpc_xpc_code_counts`` (the histogram of the rows' codes under the conjunction: ``2^conj_len``
ints read back) and one ``dpc_xpc_partition`` (the stable split into the discarded rows and the chosen assignments' rows).
The reference filters the rows variable by variable and tests ``min_part_inst`` after each; the counts only go down, so
the count of the full assignment decides, and that is the histogram's entry.

The histogram also holds everything the leaves under the conjunction variables need (``Partition.code_counts``): the
column counts of a naive leaf, the unique assignments and their counts of a deterministic disjunction, the one assignment
of an ``is_conj`` leaf.  ``row_ids`` of every partition -- ascending, as the reference's are: the split is stable -- are read
back once, when the tree is complete.
"""
import itertools
from typing import Optional

import numpy as np


class DeviceRows:
    """Binary training data on the device, uploaded and packed ONCE per learner call: ``x`` ``[N, D]`` float32 and its
    bit planes ``[D, (N + 63) / 64]`` (``dpc_pack_bits``).  ValueError for data that are not binary; HipError for a CPU
    tensor or a missing library."""

    def __init__(self, data):
        import torch
        from deeprob.hip import clt
        from deeprob.utils.statistics import device_binary_rows
        if len(data.shape) != 2 or data.shape[0] < 1 or data.shape[1] < 1:
            raise ValueError("The data must be a matrix of samples by features")
        if data.shape[1] > clt.DPC_MAX_D:
            raise ValueError("expected at most {} variables (DPC_MAX_D), got {}".format(clt.DPC_MAX_D, data.shape[1]))
        x = device_binary_rows(data)
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.to(torch.float32).contiguous()
        self.x, self.shape = x, (int(x.shape[0]), int(x.shape[1]))
        self.planes = clt.pack_bits(x)
        self.all_rows = torch.arange(self.shape[0], dtype=torch.int32, device=x.device)


class Partition:
    """A data slice by its indices: a plain record with the reference's fields and predicates.  ``row_ids`` is filled in
    when ``generate_random_partitioning`` returns; until then ``n_rows`` is the number of rows and ``device_rows`` the
    int32 row indices on the device."""

    def __init__(self, row_ids, col_ids, uncond_vars, parent_partition: Optional['Partition'] = None,
                 is_naive: Optional[bool] = False, is_conj: Optional[bool] = False):
        self.row_ids = None if row_ids is None else np.array(row_ids)
        self.col_ids = np.array(col_ids)
        self.uncond_vars = list(uncond_vars)
        self.parent_partition = parent_partition
        self.set_parent_partition(parent_partition)
        self.sub_partitions = []
        self.is_naive = is_naive
        self.is_conj = is_conj
        #: the assignments (over ``col_ids``, sorted) not taken by a sibling conjunction; see ``xpc.build_leaf``
        self.disc_assignments = None
        self.n_rows = 0 if row_ids is None else len(self.row_ids)
        self.device_rows = None
        #: for a partition over conjunction variables: ``(conj_vars, counts [2^conj_len])``, the rows per code with bit i
        #: of a code the value of ``conj_vars[i]``
        self.code_counts = None

    def set_parent_partition(self, parent_partition: Optional['Partition']):
        if parent_partition is not None:
            parent_partition.sub_partitions.append(self)

    def is_partitioned(self) -> bool:
        return len(self.sub_partitions) != 0

    def is_horizontally_partitioned(self) -> bool:
        return self.is_partitioned() and self.n_rows > self.sub_partitions[0].n_rows

    def get_slice(self, data: np.ndarray) -> np.ndarray:
        return data[self.row_ids][:, self.col_ids]

    def get_vertical_split(self) -> list:
        """``[conjunction columns, the other columns]`` if the partition holds both kinds, else ``[]``."""
        cond_vars = [c for c in self.col_ids if c not in self.uncond_vars]
        if len(cond_vars) != 0 and len(cond_vars) != len(self.col_ids):
            return [np.asarray(cond_vars), np.asarray(self.uncond_vars)]
        return []

    def assignment_of(self, code: int) -> tuple:
        """The values of ``col_ids`` (in their order) under ``code`` of ``code_counts``."""
        conj_vars = self.code_counts[0]
        return tuple((code >> conj_vars.index(c)) & 1 for c in self.col_ids.tolist())


def _choose(hist, n_rows, assignments, min_part_inst, arity):
    """The codes that become sub-partitions, in the order of ``assignments``: ``None`` for no split, ``[]`` when one
    assignment holds every row, else the chosen codes (the discarded rows are the rest)."""
    left, chosen = n_rows, []
    for assignment in assignments:
        code = sum(bit << i for i, bit in enumerate(assignment))
        count = int(hist[code]) if hist[code] >= min_part_inst else 0
        if count == n_rows:
            return []
        if count != 0 and left - count >= min_part_inst:
            left -= count
            chosen.append(code)
            if len(chosen) == arity - 1 or left < 2 * min_part_inst:
                break
    return chosen if chosen else None


def generate_random_partitioning(data, min_part_inst: int, n_max_parts: int, conj_len: int, arity: int, sd: bool,
                                 uncond_vars: list, random_state: np.random.RandomState):
    """
    Create a random partition tree.

    :param data: The binary data: a numpy array, a device tensor, or the :class:`DeviceRows` of either.
    :param min_part_inst: The minimum number of instances allowed per partition.
    :param n_max_parts: The maximum number of partitions in the tree.
    :param conj_len: The conjunction length.
    :param arity: The maximum number of sub-partitions of a horizontal split.
    :param sd: True if the tree will model a structured-decomposable circuit.
    :param uncond_vars: Ordered list of variables; the first ``conj_len`` split the root.
    :param random_state: The random state.
    :return: ``(partition_root, cl_parts_l, conj_vars_l, n_partitions)`` as the reference returns them.
    """
    import torch
    from deeprob.hip import xpc
    dev = data if isinstance(data, DeviceRows) else DeviceRows(data)
    root = Partition(None, uncond_vars, uncond_vars)
    root.n_rows, root.device_rows = dev.shape[0], dev.all_rows
    every, n_partitions, conj_vars_l, cl_parts_l, leaves = [root], 0, [], [], [root]
    while leaves and n_partitions + len(leaves) < n_max_parts:
        part = leaves.pop(random_state.randint(len(leaves)))
        chosen = None
        if len(part.uncond_vars) >= conj_len and part.n_rows >= 2 * min_part_inst:
            order = part.uncond_vars.copy()
            if not sd:
                random_state.shuffle(order)
            conj_vars = order[:conj_len]
            assignments = [list(a) for a in itertools.product([0, 1], repeat=conj_len)]
            random_state.shuffle(assignments)
            split = xpc.Split(dev.planes, dev.shape[0], part.device_rows, [part.n_rows], [conj_vars])
            hist = split.counts().cpu().numpy().astype(np.int64)          # the one read-back of a split
            chosen = _choose(hist[0], part.n_rows, assignments, min_part_inst, arity)
        if chosen is None:
            n_partitions += 1
            cl_parts_l.append(part)
            continue

        if conj_vars not in conj_vars_l:
            conj_vars_l.append(conj_vars)
        rest = [v for v in part.uncond_vars if v not in conj_vars]
        child_of_code = np.zeros((1, 1 << conj_len), np.int64)
        for k, code in enumerate(chosen):
            child_of_code[0, code] = k + 1
        if chosen:
            rows = split.partition(child_of_code, hist)
            sizes = split.child_n[0, :len(chosen) + 1].tolist()
            pieces = torch.split(rows, sizes)
        else:                                   # one assignment holds every row: the partition is only cut vertically
            sizes, pieces = [part.n_rows], [part.device_rows]
        taken = set()
        for k, (n, piece) in enumerate(zip(sizes, pieces)):
            sub = Partition(None, part.col_ids.copy(), rest.copy(), parent_partition=part)
            sub.n_rows, sub.device_rows = int(n), piece
            every.append(sub)
            vertical = sub.get_vertical_split()
            if not vertical:
                leaves.append(sub)
                continue
            n_partitions += 1
            naive = Partition(None, vertical[0].copy(), [], parent_partition=sub, is_naive=True, is_conj=k > 0)
            naive.n_rows, naive.device_rows = sub.n_rows, piece
            naive.code_counts = (list(conj_vars), np.where(child_of_code[0] == k, hist[0], 0))
            if k > 0:
                taken.add(naive.assignment_of(chosen[k - 1]))
            other = Partition(None, vertical[1].copy(), vertical[1].copy(), parent_partition=sub)
            other.n_rows, other.device_rows = sub.n_rows, piece
            every += [naive, other]
            leaves.append(other)
        first = part.sub_partitions[0]
        if first.sub_partitions:
            first.sub_partitions[0].disc_assignments = np.array(
                sorted(set(itertools.product([0, 1], repeat=conj_len)) - taken)).reshape(-1, conj_len)

    n_partitions += len(leaves)
    cl_parts_l.extend(leaves)
    # the row ids of every partition in one read: each distinct device segment once
    segments = {}
    for p in every:
        segments.setdefault((p.device_rows.data_ptr(), p.n_rows), p.device_rows)
    host = torch.cat(list(segments.values())).cpu().numpy().astype(np.int64)
    at = {}
    for key, n in zip(segments, np.cumsum([0] + [k[1] for k in segments])):
        at[key] = host[n:n + key[1]]
    for p in every:
        p.row_ids = at[(p.device_rows.data_ptr(), p.n_rows)]
    return root, cl_parts_l, conj_vars_l, n_partitions
