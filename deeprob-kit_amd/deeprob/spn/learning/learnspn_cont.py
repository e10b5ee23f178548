"""The Gaussian column kind of ``learn_spn`` (learnspn.py): what its generation loop asks when every distribution is
``Gaussian``.  The float64 moments of all columns of a generation come from one launch (``dpl_column_moments``: the
zero-variance rule ``var <= 1e-8`` and the MLE leaves ``Gaussian(mean, max(sqrt(var), 1e-5))``); the ECDF ranks and the
random-feature Gram matrices of all column-splitting tasks from ``dpl_ecdf_ranks`` and ``dpl_rdc_gram`` (the score from
them is ``splitting.rdc.scores_from_gram``); the row splits from the float k-means (``dpl_kmeansf_*``).  The histogram
splits (the functions of splitting/entropy.py, gini.py and gvs.py): per generation the minimum, the maximum and the
quartiles of every tested column from the device sort of the ranks (one read: the host derives numpy's bin count from them
in float64 and checks the caps), the bin codes of all of them from ``dpl_hist_codes``, then the counts
(``dpl_code_counts``) or the G statistics of all column pairs (``dpl_pair_g_codes``) and one read.  See DESIGN.md,
"LearnSPN on continuous data".
"""
import numpy as np
import torch

from deeprob.hip import HipError, learn as L
from deeprob.spn.learning.learnspn import KNOWN_COLS, KMEANS_RESTARTS, _method, item_tables, last_info, new_node  # noqa: F401
from deeprob.spn.learning.learnspn import gvs_draws, hist_split, pair_clusters
from deeprob.spn.learning.splitting import rdc as R, hist as H

BUILT_COLS_CONT = ('random',)
ZERO_VARIANCE = 1e-8          # np.isclose(var, 0.0) (learnspn.py:132)
MIN_STDDEV = 1e-5             # leaf.py:530


def to_device_f(data, who='learn_spn'):
    """The data as float32, column major, on the device (one upload); ValueError on NaN or inf; HipError for a CPU
    tensor."""
    if len(data.shape) != 2:
        raise ValueError("The data must be a matrix of samples by features")
    if isinstance(data, torch.Tensor):
        if not data.is_cuda:
            raise HipError("data lives on '{}': the deeprob HIP path only works on tensors on a HIP device (there is no "
                           "CPU fallback); pass a numpy array or a device tensor".format(data.device))
        x = data.to(torch.float32)
        if not bool(torch.isfinite(x).all()):
            raise ValueError("The data contains NaN or inf: {} needs complete, finite data".format(who))
        x = x.t().contiguous()
    else:
        host = np.asarray(data).astype(np.float32)
        if not np.isfinite(host).all():
            raise ValueError("The data contains NaN or inf: {} needs complete, finite data".format(who))
        if not torch.cuda.is_available():
            raise HipError("{} needs a HIP device (there is no CPU fallback)".format(who))
        x = torch.from_numpy(np.ascontiguousarray(host.T)).cuda()
    return L.DeviceData(x.reshape(-1), data.shape[0], data.shape[1])


class GaussianColumns:
    """The methods of ``learnspn.DiscreteColumns``, for ``Gaussian`` columns."""

    launches_per_generation = None          # (no bound has been derived for this kind)
    smoothed_leaves = False                 # (alpha is not used by a Gaussian leaf and not checked)

    def __init__(self, distributions, domains):
        self.domains = domains

    def check_split_cols(self, name):
        if hist_split(name) is not None:
            return
        if name in ('gvs', 'rgvs'):
            raise NotImplementedError("split_cols '{}' is not built for Gaussian columns: a G-test needs a contingency table "
                                      "(built: random, or the function rdc_cols)".format(name))
        _method(name, KNOWN_COLS, BUILT_COLS_CONT, "Unknown split rows method called {}", 'split_cols')

    def check_columns(self, rdc_kw):
        R.check_continuous(self.domains)
        if rdc_kw is not None:
            R.check_parameters_continuous(**rdc_kw)

    def upload(self, data):
        self.data = to_device_f(data)
        L.load_library()
        return self.data

    def column_stats(self, row_index, item_col, item_off, item_n):
        """([mean, variance], whether the variance is zero) of every item, from one launch and one read."""
        moments = L.read(L.column_moments(self.data, row_index, item_col, item_off, item_n))
        return moments, moments[:, 1] <= ZERO_VARIANCE

    def leaf(self, var, moments, n, alpha):
        """learning/leaf.py:64-68 with structure/leaf.py:529-530 from the column's moments."""
        return new_node('Gaussian', [var], params={'mean': float(moments[0]),
                                                   'stddev': max(float(np.sqrt(moments[1])), MIN_STDDEV)})

    def draw_split_cols(self, random_state, t, split_cols, cols_kw):
        if split_cols in H.STAT_SPLITS:
            return None                                 # (the entropy and Gini splits draw nothing)
        if split_cols in H.GTEST_SPLITS:
            return gvs_draws(random_state, len(t.scope), split_cols)                              # gvs.py:30, 76, 89
        return R.draw_features(random_state, len(t.scope), int(cols_kw['k']), cols_kw['s'])       # rdc.py:170-176

    def binned(self, row_index, tasks, columns_of, rule):
        """The bin codes of the columns ``columns_of(t)`` (positions in the scope) of every task under numpy's 'scott' or
        'fd' bins: ``(codes, code offset of every item, bins of every item, column of every item)``, the items task by
        task.  One read (the order statistics the bin counts need) and one launch."""
        col, off, n, var = [], [], [], []
        for t in tasks:
            for p in columns_of(t):
                col.append(t.scope[p])
                off.append(t.row_off)
                n.append(t.n)
                var.append(float(t.counts[p][1]))
        quartiles = [H.quartile_positions(m) for m in n]
        at = [[0, m - 1, q[0][0], q[0][1], q[1][0], q[1][1]] for m, q in zip(n, quartiles)]
        stats = L.read(L.order_statistics(self.data, row_index, col, off, n, at))
        lo, hi, bins = [], [], []
        for i, (m, q) in enumerate(zip(n, quartiles)):
            a, b = H.outer_edges(stats[i, 0], stats[i, 1])
            if rule == 'scott':
                width = H.scott_width(m, var[i])
            else:
                width = H.fd_width(m, H.lerp(stats[i, 2], stats[i, 3], q[0][2]), H.lerp(stats[i, 4], stats[i, 5], q[1][2]))
            lo.append(a)
            hi.append(b)
            bins.append(H.bin_count(a, b, width))
        codes, code_off = L.hist_codes(self.data, row_index, col, off, n, lo, hi, bins)
        return codes, code_off, np.asarray(bins, np.int64), np.asarray(col, np.int64), np.asarray(n, np.int64)

    def gtest_values(self, row_index, tasks):
        """``(g, dof)`` of the column pairs a < b of the tested columns of every task, in task order (gvs.py:184-205 with
        'fd' bins)."""
        if not tasks:
            return np.zeros(0), np.zeros(0, np.int64)
        codes, code_off, bins, col, n = self.binned(row_index, tasks, lambda t: t.draw[0], 'fd')
        ia_all, ib_all, first = [], [], 0
        for t in tasks:
            ia, ib = np.triu_indices(len(t.draw[0]), 1)        # the pairs a < b, in the order of two nested loops
            ia_all.append(ia + first)
            ib_all.append(ib + first)
            first += len(t.draw[0])
        ia, ib = np.concatenate(ia_all), np.concatenate(ib_all)
        dof = (bins[ia] - 1) * (bins[ib] - 1)
        if not len(ia):
            return np.zeros(0), dof
        return L.read(L.pair_g_codes(codes, code_off[ia], code_off[ib], n[ia], bins[ia], bins[ib], col[ia], col[ib])), dof

    def stat_clusters(self, row_index, tasks, split_cols, cols_kw):
        """The clusters of every entropy / Gini task from ``np.histogram(col, 'scott')`` of its columns
        (entropy.py:39-41, gini.py:39-40)."""
        codes, code_off, bins, _, n = self.binned(row_index, tasks, lambda t: range(len(t.scope)), 'scott')
        counts, count_off = L.code_counts(codes, code_off, n, bins)
        counts = L.read(counts)
        out, first = [], 0
        for t in tasks:
            items = range(first, first + len(t.scope))
            first += len(t.scope)
            out.append(H.stat_clusters(split_cols, cols_kw, [counts[count_off[i]:count_off[i] + bins[i]] for i in items], t.n,
                                       True))
        return out

    def split_cols_clusters(self, row_index, tasks, split_cols, cols_kw):
        """The column clusters of every rdc task: ranks, Gram matrices, scores, components (rdc.py:43-48); of every
        histogram task: bin codes, then counts or G statistics."""
        if not tasks:
            return []
        if split_cols in H.STAT_SPLITS:
            return self.stat_clusters(row_index, tasks, split_cols, cols_kw)
        if split_cols in H.GTEST_SPLITS:
            return pair_clusters(tasks, split_cols, cols_kw, *self.gtest_values(row_index, tasks))
        k = int(cols_kw['k'])
        ranks, out_off = L.ecdf_ranks(self.data, row_index, *item_tables(tasks))
        gram_tasks, first = [], 0
        for t in tasks:
            gram_tasks.append((t.n, len(t.scope), int(out_off[first])))
            first += len(t.scope)
        gram = L.rdc_gram(ranks, gram_tasks, k, np.concatenate([t.draw[0].reshape(-1) for t in tasks]),
                          np.concatenate([t.draw[1].reshape(-1) for t in tasks]))
        G, S = L.read(gram['G']), L.read(gram['S'])
        out = []
        for i, t in enumerate(tasks):
            f = gram['fs'][i]
            g0, s0 = int(gram['g_off'][i]), int(gram['feat_off'][i])
            out.append(R.components(R.scores_from_gram(G[g0:g0 + f * f], S[s0:s0 + f], t.n, len(t.scope), k) > cols_kw['d']))
        return out

    def kmeans_batch(self, row_index, tasks, n_clusters):
        return L.KMeansBatch(self.data, row_index, [(t.row_off, t.n, t.scope, None, t.draw) for t in tasks], KMEANS_RESTARTS,
                             n_clusters)

    def gmm_batch(self, row_index, tasks, n_clusters):
        return L.GmmBatch(self.data, row_index, [(t.row_off, t.n, t.scope, None, t.draw) for t in tasks], n_clusters)
