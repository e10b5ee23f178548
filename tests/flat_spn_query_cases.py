"""Inputs for the node-graph SPN query tests (test helper): values drawn inside the leaves' supports, so that few rows
sit on the -1e31 floor (tests/flat_spn_cases.py::random_inputs draws a category outside the support in a sixth of the
Categorical entries and Uniform inputs regardless of the leaves' intervals), plus a few deliberate outsiders."""
import numpy as np

RANDOM_CASES = [(5, 0, 1), (7, 1, 63), (9, 2, 65), (12, 3, 1000), (17, 4, 4097)]      # n_features, seed, B
OUTSIDE_RATE = 0.01       # share of rows that get one out-of-support entry


def support_inputs(d, family, B: int, seed: int, nan_rate: float = 0.5) -> np.ndarray:
    """[B, n_features] float32: Gaussian randn * 2.5, Bernoulli {0, 1}, Categorical inside the categories, Uniform
    start + width * rand of a leaf of that variable picked at random per row; `nan_rate` of the entries NaN; row 0
    all NaN; about OUTSIDE_RATE of the rows carry one entry outside every support (category 5, or 1e3)."""
    rs = np.random.RandomState(seed)
    uniform = {}
    for n in d['nodes']:
        if n['class'] == 'Uniform':
            uniform.setdefault(n['scope'][0], []).append((n['params']['start'], n['params']['width']))
    cols = []
    for v, f in enumerate(family):
        if f == 'Gaussian':
            cols.append(rs.randn(B) * 2.5)
        elif f == 'Bernoulli':
            cols.append(rs.randint(0, 2, B).astype(np.float64))
        elif f == 'Categorical':
            cols.append(rs.randint(0, 5, B).astype(np.float64))
        else:
            iv = np.asarray(uniform.get(v, [(0.0, 1.0)]))
            pick = iv[rs.randint(len(iv), size=B)]
            cols.append(pick[:, 0] + pick[:, 1] * rs.rand(B))
    x = np.stack(cols, axis=1).astype(np.float32)
    x[rs.rand(*x.shape) < nan_rate] = np.nan
    bounded = [v for v, f in enumerate(family) if f != 'Gaussian']       # (a Gaussian has no outside, only a far tail)
    for r in np.flatnonzero(rs.rand(B) < OUTSIDE_RATE):
        if bounded:
            v = bounded[rs.randint(len(bounded))]
            x[r, v] = 5.0 if family[v] == 'Categorical' else 1e3
    x[0, :] = np.nan
    return x
