"""LearnSPN (reference deeprob/spn/learning/learnspn.py:41-222) for all-continuous data -- every distribution ``Gaussian`` --
with the statistics of every task on the HIP device and the task queue, every random draw, the score algebra and the graph
on the host.  ``learn_spn`` dispatches here; the discrete path (learnspn.py) is not involved.

A generation of the task queue is processed as a whole, as on the discrete path: the float64 moments of all its columns in
one launch (``dpl_column_moments``: the zero-variance rule ``var <= 1e-8`` and the MLE leaves
``Gaussian(mean, max(sqrt(var), 1e-5))``), the draws on the host in queue order, the ECDF ranks and the random-feature Gram
matrices of all column-splitting tasks (``dpl_ecdf_ranks``, ``dpl_rdc_gram``; the score from them is
``splitting.rdc.scores_from_gram``), the float k-means of all row-splitting tasks (``dpl_kmeansf_*``) and one partition
launch (``dpl_partition_rows``).  See DESIGN.md, "LearnSPN on continuous data".
"""
import numpy as np

from deeprob.spn.learning.learnspn import (KNOWN_LEAF, BUILT_LEAF, KNOWN_ROWS, BUILT_ROWS, KNOWN_COLS, KMEANS_RESTARTS,
                                            _Task, _kwargs, _method, check_random_state, new_node, to_flat)

BUILT_COLS_CONT = ('random',)
ZERO_VARIANCE = 1e-8          # np.isclose(var, 0.0) (learnspn.py:132)
MIN_STDDEV = 1e-5             # leaf.py:530

_last_info = {}


def last_info() -> dict:
    """What the last continuous ``learn_spn`` recorded: ``generations``, ``tasks_per_generation``, ``kernels`` (launches of
    this library; ``torch.sort`` and the gathers in front of it are not counted), ``reads``, ``uploads``,
    ``lloyd_launches`` and ``lloyd_iterations``."""
    return dict(_last_info)


def check_arguments(data, distributions, domains, learn_leaf, split_rows, split_cols, learn_leaf_kwargs, split_rows_kwargs,
                    split_cols_kwargs, min_rows_slice, min_cols_slice):
    """The argument checks of ``learn_spn`` in the reference's order, then what the continuous path does not build;
    returns ``(leaf kwargs, rows kwargs, cols kwargs)`` with the defaults filled in.  Touches no device."""
    if len(domains) == 0:
        raise ValueError("The list of domains must be non-empty")
    if min_rows_slice <= 0:
        raise ValueError("The minimum number of samples required to split horizontally must be positive")
    if min_cols_slice <= 0:
        raise ValueError("The minimum number of samples required to split vertically must be positive")
    if len(data.shape) != 2:
        raise ValueError("The data must be a matrix of samples by features")
    n_samples, n_features = data.shape
    if len(distributions) != n_features or len(domains) != n_features:
        raise ValueError("Each data column should correspond to a random variable having a distribution and a domain")
    _method(learn_leaf, KNOWN_LEAF, BUILT_LEAF, "Unknown learn leaf method called {}", 'learn_leaf')
    _method(split_rows, KNOWN_ROWS, BUILT_ROWS, "Unknown split rows method called {}", 'split_rows')
    from deeprob.spn.learning.splitting import rdc as R
    rdc = split_cols is R.rdc_cols
    if not rdc:
        if split_cols in ('gvs', 'rgvs'):
            raise NotImplementedError("split_cols '{}' is not built for Gaussian columns: a G-test needs a contingency table "
                                      "(built: random, or the function rdc_cols)".format(split_cols))
        _method(split_cols, KNOWN_COLS, BUILT_COLS_CONT, "Unknown split rows method called {}", 'split_cols')
    leaf_kw = _kwargs(learn_leaf_kwargs, {'alpha': 0.1}, 'learn_mle')
    rows_kw = _kwargs(split_rows_kwargs, {'n': 2} if split_rows == 'kmeans' else {'a': 2.0, 'b': 2.0}, split_rows)
    if rdc:
        cols_kw = _kwargs(split_cols_kwargs, {'d': R.D_DEFAULT, 'k': R.K_DEFAULT, 's': R.S_DEFAULT}, 'rdc_cols')
    else:
        cols_kw = _kwargs(split_cols_kwargs, {'a': 2.0, 'b': 2.0}, split_cols)
    from deeprob.hip import learn as L
    if split_rows == 'kmeans' and not 1 <= int(rows_kw['n']) <= L.DPL_MAX_CLUSTERS:
        raise ValueError("k-means on the HIP path takes 1..{} clusters".format(L.DPL_MAX_CLUSTERS))
    R.check_continuous(domains)
    if rdc:
        R.check_parameters_continuous(**cols_kw)
    return leaf_kw, rows_kw, cols_kw


def to_device_f(data, who='learn_spn'):
    """The data as float32, column major, on the device (one upload); ValueError on NaN or inf; HipError for a CPU
    tensor."""
    import torch
    from deeprob.hip import HipError, learn as L
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
    return L.DeviceDataF(x.reshape(-1), data.shape[0], data.shape[1])


def gaussian_leaf(var, mean, variance):
    """learning/leaf.py:64-68 with structure/leaf.py:529-530 from the column's moments."""
    return new_node('Gaussian', [var], params={'mean': float(mean), 'stddev': max(float(np.sqrt(variance)), MIN_STDDEV)})


def naive_factorization(scope, moments):
    node = new_node('Product', scope)
    for i, s in enumerate(scope):
        node['children'].append(gaussian_leaf(s, moments[i][0], moments[i][1]))
    return node


def learn_spn_cont(data, distributions, domains, learn_leaf='mle', split_rows='kmeans', split_cols='rdc', learn_leaf_kwargs=None,
                   split_rows_kwargs=None, split_cols_kwargs=None, min_rows_slice=256, min_cols_slice=2, random_state=None,
                   verbose=True):
    """``learn_spn`` on all-``Gaussian`` data; the arguments are ``learn_spn``'s.  Returns a FlatSpn."""
    leaf_kw, rows_kw, cols_kw = check_arguments(data, distributions, domains, learn_leaf, split_rows, split_cols,
                                                learn_leaf_kwargs, split_rows_kwargs, split_cols_kwargs, min_rows_slice,
                                                min_cols_slice)
    random_state = check_random_state(random_state)
    import torch
    from deeprob.hip import learn as L
    from deeprob.spn.learning.splitting import rdc as R
    if split_cols is R.rdc_cols:
        split_cols = 'rdc'
    dev_data = to_device_f(data)
    L.load_library()
    device = dev_data.device
    n_total, n_features = dev_data.n_rows, dev_data.n_cols
    L.reset_counters()
    row_index = torch.arange(n_total, dtype=torch.int32, device=device)

    tmp_node = new_node('Product', range(n_features))
    generation = [_Task(tmp_node, n_total, list(range(n_features)), is_first=True)]
    tasks_per_generation, lloyd_iterations = [], 0
    while generation:
        tasks_per_generation.append(len(generation))
        # ---- moments of every column of every task, the operation of every task (learnspn.py:130-147) ---------------------
        item_col, item_off, item_n = [], [], []
        for t in generation:
            item_col += t.scope
            item_off += [t.row_off] * len(t.scope)
            item_n += [t.n] * len(t.scope)
        moments = L.read(L.column_moments(dev_data, row_index, item_col, item_off, item_n))
        o = 0
        for t in generation:
            t.counts = moments[o:o + len(t.scope)]          # ([mean, variance] of each column)
            o += len(t.scope)
            zero_var = t.counts[:, 1] <= ZERO_VARIANCE
            t.draw = zero_var
            if zero_var.all():
                t.op = 'naive'
            elif zero_var.any():
                t.op = 'rem'
            elif t.no_rows_split or len(t.scope) < min_cols_slice or t.n < min_rows_slice:
                t.op = 'leaf'
            elif t.no_cols_split or t.is_first:
                t.op = 'rows'
            else:
                t.op = 'cols'
        # ---- the draws, in queue order (random.py:31-32, 56-57; rdc.py:170-176; k-means seeds) ---------------------------
        for t in generation:
            nf = len(t.scope)
            if t.op == 'rows' and split_rows == 'random':
                p = random_state.beta(rows_kw['a'], rows_kw['b'])
                t.draw = random_state.binomial(1, p, size=t.n)
            elif t.op == 'rows':
                c = int(rows_kw['n'])
                if t.n < c:
                    raise ValueError("n_samples={} should be >= n_clusters={}".format(t.n, c))
                t.draw = np.stack([random_state.choice(t.n, c, replace=False) for _ in range(KMEANS_RESTARTS)])
            elif t.op == 'cols' and split_cols == 'random':
                p = random_state.beta(cols_kw['a'], cols_kw['b'])
                t.draw = random_state.binomial(1, p, size=nf)
            elif t.op == 'cols':
                t.draw = R.draw_features(random_state, nf, int(cols_kw['k']), cols_kw['s'])
        # ---- ranks, Gram matrices and scores of every rdc task -------------------------------------------------------------
        rdc_tasks = [t for t in generation if t.op == 'cols' and split_cols == 'rdc']
        rdc_scores = {}
        if rdc_tasks:
            k = int(cols_kw['k'])
            r_col, r_off, r_n = [], [], []
            for t in rdc_tasks:
                r_col += t.scope
                r_off += [t.row_off] * len(t.scope)
                r_n += [t.n] * len(t.scope)
            ranks, out_off = L.ecdf_ranks(dev_data, row_index, r_col, r_off, r_n)
            gram_tasks, first = [], 0
            for t in rdc_tasks:
                gram_tasks.append((t.n, len(t.scope), int(out_off[first])))
                first += len(t.scope)
            gram = L.rdc_gram(ranks, gram_tasks, k, np.concatenate([t.draw[0].reshape(-1) for t in rdc_tasks]),
                              np.concatenate([t.draw[1].reshape(-1) for t in rdc_tasks]))
            G, S = L.read(gram['G']), L.read(gram['S'])
            for i, t in enumerate(rdc_tasks):
                f = gram['fs'][i]
                g0, s0 = int(gram['g_off'][i]), int(gram['feat_off'][i])
                rdc_scores[id(t)] = R.scores_from_gram(G[g0:g0 + f * f], S[s0:s0 + f], t.n, len(t.scope), k)
        # ---- k-means of every row-splitting task --------------------------------------------------------------------------
        km_tasks = [t for t in generation if t.op == 'rows' and split_rows == 'kmeans']
        km_labels, km_result = None, {}
        if km_tasks:
            batch = L.KMeansBatchF(dev_data, row_index, [(t.row_off, t.n, t.scope, t.draw) for t in km_tasks], KMEANS_RESTARTS,
                                   int(rows_kw['n']))
            inertia, sizes, km_labels, iters = batch.run()
            lloyd_iterations += iters
            for i, t in enumerate(km_tasks):
                best = int(np.argmin(inertia[i]))              # the lowest inertia, the first one on a tie
                km_result[id(t)] = (best * batch.n_lab + batch.lab_off[i], sizes[i, best])
        # ---- the nodes and the children of every task, in queue order (learnspn.py:149-210) -----------------------------
        children, host_labels, n_host_labels = [], [], 0

        def child(task, parent_task, label_off=0, label=-1):
            task.child_src = (parent_task.row_off, parent_task.n, label_off, label)
            children.append(task)

        for t in generation:
            scope, nf = t.scope, len(t.scope)
            if t.op == 'rem':
                zero_var = t.draw
                node = new_node('Product', scope)
                rem = [i for i in range(nf) if zero_var[i]]
                node['children'].append(naive_factorization([scope[i] for i in rem], [t.counts[i] for i in rem]))
                child(_Task(node, t.n, [scope[i] for i in range(nf) if not zero_var[i]], is_first=t.is_first), t)
                t.parent['children'].append(node)
            elif t.op == 'leaf' and nf == 1:
                t.parent['children'].append(gaussian_leaf(scope[0], t.counts[0][0], t.counts[0][1]))
            elif t.op in ('leaf', 'naive'):
                t.parent['children'].append(naive_factorization(scope, t.counts))
            elif t.op == 'rows':
                if split_rows == 'random':
                    labels = t.draw.astype(np.uint8)
                    sizes_t = np.bincount(labels, minlength=2)
                    label_off = n_host_labels
                    host_labels.append(labels)
                    n_host_labels += t.n
                else:
                    label_off, sizes_t = km_result[id(t)]
                present = [c for c in range(len(sizes_t)) if sizes_t[c] > 0]
                if len(present) == 1:
                    child(_Task(t.parent, t.n, scope, no_cols_split=False, no_rows_split=True), t)
                    continue
                node = new_node('Sum', scope, weights=[int(sizes_t[c]) / t.n for c in present])
                for c in present:
                    child(_Task(node, int(sizes_t[c]), scope), t, label_off, c)
                t.parent['children'].append(node)
            else:
                if split_cols == 'random':
                    clusters = np.asarray(t.draw)
                else:
                    clusters = R.components(rdc_scores[id(t)] > cols_kw['d'])            # rdc.py:43-48
                present = np.unique(clusters)
                if len(present) == 1:
                    child(_Task(t.parent, t.n, scope, no_cols_split=True, no_rows_split=False), t)
                    continue
                node = new_node('Product', scope)
                for c in present:
                    child(_Task(node, t.n, [scope[i] for i in range(nf) if clusters[i] == c]), t)
                t.parent['children'].append(node)
        # ---- the next generation's row index ------------------------------------------------------------------------------
        if children:
            off = 0
            for c in children:
                c.row_off = off
                off += c.n
            if host_labels:
                km_labels = L.upload(device, labels=np.concatenate(host_labels))['labels']
            src = np.array([c.child_src for c in children], np.int64)
            row_index = L.partition_rows(row_index, src[:, 0], src[:, 1], src[:, 2], src[:, 3], [c.row_off for c in children],
                                         [c.n for c in children], None if km_labels is None else km_labels.reshape(-1), off)
        generation = children

    c = L.COUNTERS
    _last_info.clear()
    _last_info.update(generations=len(tasks_per_generation), kernels=c['kernels'], reads=c['reads'], uploads=c['uploads'],
                      lloyd_launches=c['lloyd_kernels'] + c['lloyd_reads'], lloyd_iterations=lloyd_iterations,
                      tasks_per_generation=tasks_per_generation)
    return to_flat(tmp_node['children'][0])
