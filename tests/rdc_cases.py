"""The contingency tables the maximal-correlation tests share: tests/test_rdc_host.py runs the two restatements of
tests/rdc_ref.py on them, tests/test_rdc_gpu.py runs ``dpl_pair_maxcorr`` on the rows they come from.  A helper
module: no test, no package import."""
import numpy as np

from tests import rdc_ref

N_ROWS = 1200
SEGMENTS = (1, 2, 63, 64, 65, 257, 1000)
#: stated domain size of every data column
KS = [2, 2, 3, 5, 16, 16, 2, 16, 5, 3, 3]
#: (column i, column j, what the pair is there for)
PAIRS = [(0, 1, '(2, 2), dependent'), (0, 2, '(2, 3)'), (2, 3, '(3, 5), dependent'), (4, 6, '(16, 2)'),
         (4, 5, '(16, 16), dependent'), (4, 7, '(16, 16), duplicate columns'), (8, 3, 'value 3 of column 8 is absent'),
         (9, 0, 'column 9 is constant'), (10, 3, 'column 10 stores values >= its K'), (2, 10, '(3, 3), values >= K')]

_cache = {}


def noisy_copy(rs, col, k, noise):
    return np.where(rs.rand(len(col)) < noise, rs.randint(0, k, size=len(col)), col)


def kernel_case():
    """dict: ``x`` [N_ROWS, 11] uint8, ``segs`` (the row segments, shuffled and sorted ones alternating), ``pairs`` (one
    record per (segment, column pair): columns, segment number, stated domain sizes) and ``tables`` (their joint counts)."""
    if 'kernel' in _cache:
        return _cache['kernel']
    rs = np.random.RandomState(20)
    x = np.zeros((N_ROWS, len(KS)), np.int64)
    x[:, 0] = rs.randint(0, 2, N_ROWS)
    x[:, 1] = noisy_copy(rs, x[:, 0], 2, 0.4)
    x[:, 3] = rs.randint(0, 5, N_ROWS)
    x[:, 2] = noisy_copy(rs, x[:, 3] % 3, 3, 0.5)
    x[:, 4] = rs.randint(0, 16, N_ROWS)
    x[:, 5] = noisy_copy(rs, (x[:, 4] * 5 + 3) % 16, 16, 0.5)
    x[:, 6] = noisy_copy(rs, x[:, 4] % 2, 2, 0.6)
    x[:, 7] = x[:, 4]
    x[:, 8] = np.array([0, 1, 2, 4])[rs.randint(0, 4, N_ROWS)]
    x[:, 9] = 1
    x[:, 10] = rs.randint(0, 5, N_ROWS)                   # stated K = 3: the values 3 and 4 are not counted
    segs = [np.sort(rs.permutation(N_ROWS)[:n]) if i % 2 else rs.permutation(N_ROWS)[:n] for i, n in enumerate(SEGMENTS)]
    pairs, tables = [], []
    for t, rows in enumerate(segs):
        for ci, cj, _ in PAIRS:
            pairs.append((ci, cj, t, KS[ci], KS[cj]))
            tables.append(rdc_ref.joint_counts(x[rows, ci], x[rows, cj], KS[ci], KS[cj]))
    _cache['kernel'] = dict(x=x.astype(np.uint8), segs=segs, pairs=pairs, tables=tables)
    return _cache['kernel']


def block_diagonal(block, times):
    b = np.asarray(block)
    out = np.zeros((b.shape[0] * times, b.shape[1] * times), np.int64)
    for i in range(times):
        out[i * b.shape[0]:(i + 1) * b.shape[0], i * b.shape[1]:(i + 1) * b.shape[1]] = b
    return out


def hand_tables():
    """[(name, joint counts, the known maximal correlation)]."""
    b = np.array([[3, 1], [1, 3]])                       # phi = (9 - 1) / 16 = 0.5
    k16 = np.arange(1, 17)
    return [
        ('identical K=2', np.diag([37, 63]), 1.0),
        ('identical K=16', np.diag(k16 * 3), 1.0),
        ('independent 3x5', np.outer([2, 5, 3], [1, 4, 2, 6, 7]), 0.0),
        ('independent 16x16', np.outer(k16, k16[::-1]), 0.0),
        # three blocks: the block indicators are perfectly correlated, a two-dimensional space of value 1
        ('block diagonal, top two equal 1', block_diagonal(b, 3), 1.0),
        # a product table: the singular values are the products {1, 0.5} x {1, 0.5} without the 1: 0.5, 0.5, 0.25
        ('product table, top two equal 0.5', np.kron(b, b), 0.5),
        ('one present value', np.array([[0, 0, 0], [4, 9, 2], [0, 0, 0]]), 0.0),
        ('one present value, other side', np.array([[0, 4], [0, 9], [0, 2]]), 0.0),
        ('2x2 inside 3x3', np.array([[5, 0, 1], [0, 0, 0], [2, 0, 7]]), abs(5 * 7 - 1 * 2) / np.sqrt(6 * 9 * 7 * 8)),
    ]


def rows_of(joint):
    """The rows (value of column i, value of column j) a joint table counts, in row-major cell order."""
    joint = np.asarray(joint)
    a, b = np.divmod(np.repeat(np.arange(joint.size), joint.reshape(-1)), joint.shape[1])
    return np.stack([a, b], axis=1).astype(np.uint8)
