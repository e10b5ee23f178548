"""The Gaussian column kind of ``learn_spn`` (learnspn.py): what its generation loop asks when every distribution is
``Gaussian``.  The float64 moments of all columns of a generation come from one launch (``dpl_column_moments``: the
zero-variance rule ``var <= 1e-8`` and the MLE leaves ``Gaussian(mean, max(sqrt(var), 1e-5))``); the ECDF ranks and the
random-feature Gram matrices of all column-splitting tasks from ``dpl_ecdf_ranks`` and ``dpl_rdc_gram`` (the score from
them is ``splitting.rdc.scores_from_gram``); the row splits from the float k-means (``dpl_kmeansf_*``).  See DESIGN.md,
"LearnSPN on continuous data".
"""
import numpy as np
import torch

from deeprob.hip import HipError, learn as L
from deeprob.spn.learning.learnspn import KNOWN_COLS, KMEANS_RESTARTS, _method, item_tables, last_info, new_node  # noqa: F401
from deeprob.spn.learning.splitting import rdc as R

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
        return R.draw_features(random_state, len(t.scope), int(cols_kw['k']), cols_kw['s'])       # rdc.py:170-176

    def split_cols_clusters(self, row_index, tasks, split_cols, cols_kw):
        """The column clusters of every rdc task: ranks, Gram matrices, scores, components (rdc.py:43-48)."""
        if not tasks:
            return []
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
