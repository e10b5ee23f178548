"""What the histogram column splits share (entropy.py, gini.py, gvs.py of this package): numpy's uniform bins for float32
columns restated, the statistics of a histogram, and the one-task driver behind the functions called alone.  Host code
on numpy only; the device is reached through the column-kind objects of ``learn_spn``.

numpy's bins for a float32 column (``np.histogram(col, 'scott')``, ``np.histogram_bin_edges(col, 'fd')``):
``lo, hi = min, max`` (``lo - 0.5, hi + 0.5`` when equal); the width is Scott's ``(24 sqrt(pi) / n)^(1/3) * std`` or
Freedman-Diaconis' ``2 * (q75 - q25) * n^(-1/3)`` with ``np.percentile``'s linear interpolation; ``bins = ceil((hi - lo) /
width)``, 1 for a width of 0; the edges are float32, ``edge[i] = fl32(fl32(i) * step + lo)`` with ``step = fl32(fl32(hi -
lo) / fl32(bins))`` and ``edge[bins] = hi``; a value's bin is (the number of edges <= x) - 1, the last one for ``x ==
hi``.  The width is formed here in float64 from the device's statistics (numpy forms it in float32: the two differ in the
last digits, which moves a bin count only when ``(hi - lo) / width`` is within about 1e-4 of an integer).
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
#: tag of each built function's split in ``learn_spn`` (the strings of the reference stay unbuilt names)
ENTROPY, ENTROPY_ADAPTIVE, GINI, GINI_ADAPTIVE = 'entropy_cols', 'entropy_adaptive_cols', 'gini_cols', 'gini_adaptive_cols'
STAT_SPLITS = (ENTROPY, ENTROPY_ADAPTIVE, GINI, GINI_ADAPTIVE)
GTEST_SPLITS = ('gvs', 'rgvs')
DEFAULTS = {ENTROPY: {'e': 0.3, 'alpha': 0.1}, GINI: {'e': 0.3, 'alpha': 0.1},
            ENTROPY_ADAPTIVE: {'e': 0.3, 'alpha': 0.1, 'size': None}, GINI_ADAPTIVE: {'e': 0.3, 'alpha': 0.1, 'size': None},
            'gvs': {'p': 5.0}, 'rgvs': {'p': 5.0}}
MISSING_SIZE = {ENTROPY_ADAPTIVE: "Missing data size for Adaptive Entropy column splitting method",      # entropy.py:74
                GINI_ADAPTIVE: "Missing data size for Adaptive Gini column splitting method"}            # gini.py:76


# ---- numpy's bins -------------------------------------------------------------------------------------------------------------
def outer_edges(lo, hi):
    """``(lo, hi)`` as float32, moved apart by 0.5 each when equal (numpy's ``_get_outer_edges``)."""
    lo, hi = np.float32(lo), np.float32(hi)
    if lo == hi:
        lo, hi = np.float32(lo - np.float32(0.5)), np.float32(hi + np.float32(0.5))
    return lo, hi


def scott_width(n: int, variance: float) -> float:
    """Scott's bin width from the population variance, float64."""
    return (24.0 * np.pi ** 0.5 / n) ** (1.0 / 3.0) * float(np.sqrt(variance))


def quartile_positions(n: int):
    """(lower position, upper position, weight) of the 25th and of the 75th percentile among ``n`` sorted values
    (``np.percentile``, method 'linear')."""
    out = []
    for q in (0.25, 0.75):
        virtual = (n - 1) * q
        below = int(np.floor(virtual))
        out.append((below, min(below + 1, n - 1), virtual - below))
    return out


def lerp(a: float, b: float, t: float) -> float:
    """numpy's ``_lerp``, float64."""
    a, b = float(a), float(b)
    return b - (b - a) * (1.0 - t) if t >= 0.5 else a + (b - a) * t


def fd_width(n: int, q25: float, q75: float) -> float:
    """The Freedman-Diaconis bin width from the two quartiles, float64."""
    return 2.0 * (float(q75) - float(q25)) * n ** (-1.0 / 3.0)


def bin_count(lo, hi, width: float) -> int:
    """``ceil((hi - lo) / width)`` for the outer edges ``lo``, ``hi``; 1 for a width of 0."""
    if not width:
        return 1
    return int(np.ceil((float(hi) - float(lo)) / width))


def bin_edges(lo, hi, bins: int) -> np.ndarray:
    """The ``bins + 1`` float32 edges ``np.linspace`` gives: one float32 multiply, one float32 add, the last one ``hi``."""
    lo, hi = np.float32(lo), np.float32(hi)
    step = np.float32(np.float32(hi - lo) / np.float32(bins))
    edges = (np.arange(bins + 1, dtype=np.float32) * step).astype(np.float32) + lo
    edges[-1] = hi
    return edges.astype(np.float32)


def bin_codes(x: np.ndarray, lo, hi, bins: int) -> np.ndarray:
    """The bin of every value of ``x`` (float32, ``lo <= x <= hi``): the number of edges <= x, minus one; ``x == hi``
    falls in the last bin.  What ``dpl_hist_codes`` computes."""
    edges = bin_edges(lo, hi, bins)
    return np.minimum(np.searchsorted(edges[:-1], np.asarray(x, np.float32), side='right') - 1, bins - 1).astype(np.int64)


def column_bins(col: np.ndarray, rule: str):
    """``(lo, hi, bins)`` of a float32 column under 'scott' or 'fd', with the width in float64 from float64 statistics:
    the host restatement of what the Gaussian column kind does with the device's moments and sorted values."""
    col = np.asarray(col, np.float32)
    n = len(col)
    lo, hi = outer_edges(col.min(), col.max())
    if rule == 'scott':
        width = scott_width(n, float(np.var(col.astype(np.float64))))
    else:
        s = np.sort(col)
        (a0, a1, ta), (b0, b1, tb) = quartile_positions(n)
        width = fd_width(n, lerp(s[a0], s[a1], ta), lerp(s[b0], s[b1], tb))
    return lo, hi, bin_count(lo, hi, width)


# ---- the statistics of a histogram ----------------------------------------------------------------------------------------
def entropy_of(counts: np.ndarray, n: int, alpha: float, normalised: bool) -> float:
    """entropy.py:36-37 (discrete) and :40-41 (continuous, divided by ``log2(bins)``: nan for one bin)."""
    hist = np.asarray(counts, np.int64)
    probs = (hist + alpha) / (n + len(hist) * alpha)
    with np.errstate(divide='ignore', invalid='ignore'):
        entropy = -np.sum(probs * np.log2(probs))
        return entropy / np.log2(len(hist)) if normalised else entropy


def gini_of(counts: np.ndarray, n: int, alpha: float, normalised: bool = False) -> float:
    """gini.py:37-45 with ``compute_gini`` (utils/statistics.py:112-122)."""
    hist = np.asarray(counts, np.int64)
    probs = (hist + alpha) / (n + len(hist) * alpha)
    if not np.isclose(np.sum(probs), 1.0):
        raise ValueError("Probabilities must sum up to one")
    return 1.0 - np.sum(probs ** 2.0)


def threshold(split: str, kw: dict, n: int) -> float:
    """``e``, or the adaptive ``max(e * n / size, float32 eps)`` (entropy.py:78, gini.py:80)."""
    if split in (ENTROPY_ADAPTIVE, GINI_ADAPTIVE):
        return max(kw['e'] * (n / kw['size']), np.finfo(np.float32).eps)
    return kw['e']


def stat_clusters(split: str, kw: dict, histograms, n: int, normalised: bool) -> np.ndarray:
    """The clusters of one task from the histograms of its columns: 1 where the statistic is below the threshold."""
    stat = entropy_of if split in (ENTROPY, ENTROPY_ADAPTIVE) else gini_of
    e = threshold(split, kw, n)
    partition = np.zeros(len(histograms), np.int64)
    for i, hist in enumerate(histograms):
        if stat(hist, n, kw['alpha'], normalised) < e:
            partition[i] = 1
    return partition


def g_of_table(joint: np.ndarray, n: int) -> float:
    """The G statistic of an integer table in float64, in the order ``dpl_pair_g_codes`` states."""
    ba, bb = joint.shape
    h = joint.astype(np.float64) + EPS32
    m1, m2 = np.zeros(ba), np.zeros(bb)
    for a in range(ba):
        s = h[a, 0]
        for b in range(1, bb):
            s += h[a, b]
        m1[a] = s
    for b in range(bb):
        s = h[0, b]
        for a in range(1, ba):
            s += h[a, b]
        m2[b] = s
    terms = (h * np.log(h / (m1[:, None] * m2[None, :] / float(n)))).reshape(-1)
    partial = np.zeros(256)
    for lane in range(min(256, len(terms))):
        s = 0.0
        for v in terms[lane::256]:
            s += v
        partial[lane] = s
    total = partial[0]
    for lane in range(1, 256):
        total += partial[lane]
    return 2.0 * total


# ---- a function called alone: one task over the whole matrix ----------------------------------------------------------------
def split_alone(split: str, data, distributions, domains, random_state, kw: dict, pair=None):
    """The clusters of ``split`` on the whole of ``data`` (one upload, one task, the result on the host); with ``pair = (i,
    j)`` instead ``(g, dof)`` of that one pair of columns."""
    import torch
    from deeprob.spn.learning import learnspn as LS
    from deeprob.spn.learning.splitting import rdc as R
    if split in MISSING_SIZE and kw.get('size') is None:
        raise ValueError(MISSING_SIZE[split])
    if len(distributions) == 0:
        raise ValueError("The list of distribution classes must be non-empty")
    if len(domains) == 0:
        raise ValueError("The list of domains must be non-empty")
    if len(data.shape) != 2:
        raise ValueError("The data must be a matrix of samples by features")
    if len(distributions) != data.shape[1] or len(domains) != data.shape[1]:
        raise ValueError("Each data column should correspond to a random variable having a distribution and a domain")
    if R.all_gaussian(distributions):
        from deeprob.spn.learning.learnspn_cont import GaussianColumns
        kind = GaussianColumns(distributions, domains)
    else:
        kind = LS.DiscreteColumns(distributions, domains)
    kind.check_columns(None)
    random_state = LS.check_random_state(random_state)
    dev = kind.upload(data)
    row_index = torch.arange(dev.n_rows, dtype=torch.int32, device=dev.device)
    task = LS._Task(None, dev.n_rows, list(range(dev.n_cols)))
    task.counts, _ = kind.column_stats(row_index, *LS.item_tables([task]))
    if pair is not None:
        task.draw = (np.asarray(pair, np.int64), 0, None)
        g, dof = kind.gtest_values(row_index, [task])
        return float(g[0]), int(dof[0])
    task.draw = kind.draw_split_cols(random_state, task, split, kw)
    return np.asarray(kind.split_cols_clusters(row_index, [task], split, kw)[0], np.int64)
