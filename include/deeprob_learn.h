/*
 * deeprob_learn.h -- C ABI of libdeeprob_learn.so (gfx950 / MI355X): the device side of LearnSPN
 * (deeprob.spn.learning.learnspn.learn_spn) for discrete data and, in its last section, for continuous
 * (all-Gaussian) data, with the histograms of float columns (the entropy, Gini and G-test column splits there) and the
 * Gaussian-mixture row split at the end.
 *
 * The reference is Python on numpy (deeprob/spn/learning/learnspn.py:121-222); the statistics it
 * gathers per task -- column histograms (leaf.py:162, 263; learnspn.py:132), the joint histograms
 * of the G-test (splitting/gvs.py:178-208) and of the RDC score (splitting/rdc.py:85-134, here as the
 * exact maximal correlation) and the clustering of rows (splitting/cluster.py:41-65) -- are what the entry points below compute, for ALL tasks of one generation of the task queue in
 * one launch each.  The task loop itself, every random draw and the graph stay on the host
 * (deeprob/spn/learning/learnspn.py of this package).
 *
 * Data layout
 *   - `x` is the training set as uint8 DOMAIN POSITIONS (value v of a variable with domain
 *     range(K) is stored as v), COLUMN MAJOR: x[col * n_rows + row].  A task reads a few columns
 *     over a subset of rows, so a column is one contiguous run and an unused column costs nothing;
 *   - `row_index` is the generation's row-index array: a task owns the segment
 *     [row_off, row_off + n) of it, its rows in increasing order of the original row number;
 *   - every pointer is a DEVICE pointer; `stream` is a hipStream_t passed as void*; kernels are
 *     enqueued asynchronously on it and no entry point synchronises or allocates.
 *
 * Buffer contract (the one of include/deeprob_hip.h, repeated):
 *   1. an entry point writes only its output arguments, over their documented extent;
 *   2. it writes every element of every output, for every legal shape (n = 1, one column, ragged
 *      tails included);
 *   3. nothing it does depends on what the outputs held on entry, except the arguments documented
 *      as updated in place: `labels` and `changed` of dpl_kmeans_assign, `cent` of
 *      dpl_kmeans_update, the same three of the dpl_kmeansf_ entries, and `resp`, `labels`, `lse` of dpl_gmm_estep (written
 *      for the listed pairs only);
 *   4. it leaves its `const` inputs alone.
 * There is no workspace.  Index arrays handed in are trusted to lie inside the arrays they index,
 * a value x >= the K stated for its column is not counted.  Counts are exact integers (LDS integer
 * atomics; global ones in dpl_pair_ones, onto an output the entry zeroes itself); no floating-point
 * value is accumulated atomically, every float64 sum has a fixed order.
 *
 * The return value is 0 on success and a negative DPL_E* code otherwise; dpl_last_error() returns
 * a thread-local message for the last failure.
 */
#ifndef DEEPROB_LEARN_H
#define DEEPROB_LEARN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPL_OK 0
#define DPL_EINVAL (-1)  /* bad argument (null pointer, size out of domain) */
#define DPL_ELAUNCH (-3) /* hipLaunch / runtime error                        */

#define DPL_MAX_K 16       /* largest domain size of a variable               */
#define DPL_MAX_CLUSTERS 8 /* largest number of k-means clusters              */

const char *dpl_last_error(void);
int dpl_abi_version(void);

/* Column counts: for item i (a column of a task) counts[i * kmax + v] = number of rows r in the
 * item's segment with x[item_col[i]][row_index[item_row_off[i] + r]] == v, v < kmax <= DPL_MAX_K.
 * They answer the zero-variance test (learnspn.py:132), give the MLE leaves (leaf.py:162, 263) and
 * the marginals of the G-test.  counts: [n_items * kmax] int32. */
int dpl_column_counts(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                      const int32_t *item_col, const int64_t *item_row_off, const int32_t *item_n, int64_t n_items,
                      int kmax, int32_t *counts, void *stream);

/* G statistics (gvs.py:190-197): for pair q the joint counts c[a][b] of columns pair_col_i[q],
 * pair_col_j[q] (domain sizes pair_ki[q], pair_kj[q] <= DPL_MAX_K) over the pair's row segment, in
 * exact integers, then in float64, in this order of operations:
 *   h[a][b] = c[a][b] + 2^-23;  m1[a] = h[a][0] + h[a][1] + ...;  m2[b] = h[0][b] + h[1][b] + ...;
 *   e = m1[a] * m2[b] / n;  g = 2 * (t[0][0] + t[0][1] + ... row major),  t = h * log(h / e).
 * g: [n_pairs] float64. */
int dpl_pair_g(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
               const int32_t *pair_col_i, const int32_t *pair_col_j, const int64_t *pair_row_off, const int32_t *pair_n,
               const int32_t *pair_ki, const int32_t *pair_kj, int64_t n_pairs, double *g, void *stream);

/* Maximal correlation (the exact value of the RDC score of two discrete columns, rdc.py:85-134: the
 * largest canonical correlation of the two indicator spaces; the reference's random projections
 * cancel out of it).  The pair tables are those of dpl_pair_g.  For pair q, in this order:
 *   1. c[a][b]: the joint counts over the pair's row segment, exact int32 (as for dpl_pair_g);
 *   2. r[a] = c[a][0] + c[a][1] + ..., s[b] = c[0][b] + c[1][b] + ..., n' = r[0] + r[1] + ..., integers
 *      (n' is the number of counted rows);
 *   3. the PRESENT values: the a with r[a] > 0 and the b with s[b] > 0, each in increasing order;
 *   4. fewer than two present values on either side: score = 0.0;
 *   5. a 2 x 2 present table: score = min(1, |c00 c11 - c01 c10| / sqrt(f64(r0 r1) * f64(s0 s1))), the
 *      determinant and the two products exact in int64;
 *   6. otherwise, over present values, M[a][b] = f64(c[a][b] n' - r[a] s[b]) / (f64(n') * sqrt(f64(r[a]
 *      s[b]))), numerator and r[a] s[b] exact in int64.  The VECTORS are the rows of M when it has no
 *      more rows than columns, else its columns: p vectors of length len, p <= len.  One-sided
 *      (Hestenes) Jacobi on them, never on M M^T: sweeps over the pairs (i, j), i = 0 .. p - 2,
 *      j = i + 1 .. p - 1, in that order; for a pair alpha = w_i.w_i, beta = w_j.w_j, gamma = w_i.w_j,
 *      each summed from 0.0 over e = 0 .. len - 1 in order (one multiply, one add per term); the pair
 *      is rotated when |gamma| > 2^-48 * sqrt(alpha * beta), with zeta = (beta - alpha) / (2 gamma),
 *      t = sign(zeta) / (|zeta| + sqrt(1 + zeta * zeta)) (sign(0) = +1), c = 1 / sqrt(1 + t * t),
 *      s = c * t, w_i' = c * w_i - s * w_j, w_j' = s * w_i + c * w_j.  The sweeps stop after the first
 *      one that rotates no pair, or after 30;
 *   7. score = min(1, sqrt(the largest w_v.w_v)), the norms summed as in 6, v in order.
 * score: [n_pairs] float64, every element written (0 <= score <= 1). */
int dpl_pair_maxcorr(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                     const int32_t *pair_col_i, const int32_t *pair_col_j, const int64_t *pair_row_off, const int32_t *pair_n,
                     const int32_t *pair_ki, const int32_t *pair_kj, int64_t n_pairs, double *score, void *stream);

/* The next generation's row-index array.  Child c copies, in order, the rows of the source segment
 * [child_src_off[c], + child_src_n[c]) of `row_index` whose label equals child_label[c] -- the label
 * of source position s is labels[child_label_off[c] + s] -- or all of them when child_label[c] < 0,
 * to out_index[child_dst_off[c] ...]; child_dst_n[c] is the number of rows that match (no more are
 * written).  The destination segments tile [0, n_out).  A stable partition: a slice keeps the row
 * order that boolean indexing gives (rows.py:40).  `labels` may be null when no child filters. */
int dpl_partition_rows(const int32_t *row_index, int64_t n_index, const int64_t *child_src_off, const int32_t *child_src_n,
                       const int64_t *child_label_off, const int32_t *child_label, const int64_t *child_dst_off,
                       const int32_t *child_dst_n, int64_t n_children, const uint8_t *labels, int64_t n_labels,
                       int32_t *out_index, int64_t n_out, void *stream);

/* ---- k-means (this project's definition: DESIGN.md, "LearnSPN on the device") ------------------
 * Task t has columns col_index[task_col_off[t] .. task_col_off[t + 1]) with domain sizes col_k[same
 * positions], rows row_index[task_row_off[t] .. + task_n[t]), labels at labels[r * n_lab +
 * task_lab_off[t] + i] for restart r, and centroids at cent[task_cent_off[t] + ((r * n_clusters + c)
 * * ncols_t + p) * kmax + k]: the frequency of value k of the task's p-th column in cluster c.
 * A column with K <= 2 is ONE feature (its value, centroid coordinate = frequency of 1), a column
 * with K > 2 is K one-hot features (cluster.py:58-60, utils/data.py:152-172).  The squared distance
 * of a row to a centroid is accumulated in float64 over columns in order, values in order. */

/* cent = the one-hot image of the row at position seeds[(t * n_restarts + r) * n_clusters + c] of
 * task t's segment.  cent: [n_cent] float64, every element written. */
int dpl_kmeans_init(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                    const int32_t *task_col_off, const int32_t *col_index, const int64_t *task_row_off,
                    const int32_t *task_n, const int64_t *task_cent_off, const int32_t *seeds, int n_tasks,
                    int n_restarts, int n_clusters, int kmax, double *cent, int64_t n_cent, void *stream);

/* One assignment step of every (task, restart): block b covers rows block_row0[b] .. + 256 of task
 * block_task[b].  A row joins the nearest centroid, ties to the lower index.  With first != 0 every
 * label is written and *changed is set to 1; otherwise a label is compared with the one stored and
 * *changed is set to 1 when any differs (never cleared here: the caller hands in a zeroed word).
 * labels: [n_restarts * n_lab] uint8. */
int dpl_kmeans_assign(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                      const int32_t *task_col_off, const int32_t *col_index, const int32_t *col_k,
                      const int64_t *task_row_off, const int32_t *task_n, const int64_t *task_cent_off,
                      const int64_t *task_lab_off, const int32_t *block_task, const int32_t *block_row0, int64_t n_blocks,
                      int n_restarts, int n_clusters, int kmax, const double *cent, uint8_t *labels, int64_t n_lab,
                      int first, int32_t *changed, void *stream);

/* Centroids from labels: item i is column position item_p[i] of task item_task[i]; per restart and
 * cluster the counts of the column's values over the cluster's rows (exact), centroid = count / size;
 * a cluster without rows keeps its centroid. */
int dpl_kmeans_update(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                      const int32_t *task_col_off, const int32_t *col_index, const int64_t *task_row_off,
                      const int32_t *task_n, const int64_t *task_cent_off, const int64_t *task_lab_off,
                      const int32_t *item_task, const int32_t *item_p, int64_t n_items, int n_restarts, int n_clusters,
                      int kmax, const uint8_t *labels, int64_t n_lab, double *cent, void *stream);

/* inertia[t * n_restarts + r] = sum of the squared distances of the rows to their labelled centroid:
 * 256 partial sums (partial l takes rows l, l + 256, ... in order), added in order of l; and
 * sizes[(t * n_restarts + r) * n_clusters + c] = rows labelled c. */
int dpl_kmeans_inertia(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                       const int32_t *task_col_off, const int32_t *col_index, const int32_t *col_k,
                       const int64_t *task_row_off, const int32_t *task_n, const int64_t *task_cent_off,
                       const int64_t *task_lab_off, int n_tasks, int n_restarts, int n_clusters, int kmax,
                       const double *cent, const uint8_t *labels, int64_t n_lab, double *inertia, int32_t *sizes,
                       void *stream);

/* ---- Chow-Liu tree leaves (learning/leaf.py:149-150: the counts behind BinaryCLT.fit) -------------
 * Co-occurrence counts of binary columns.  BLOCK t -- a leaf task -- has the rows row_index[blk_row_off[t]
 * .. + blk_n[t]) and the m = blk_m[t] columns blk_col[blk_col_off[t] .. + m), in any order; columns may
 * recur in other blocks.  ones[blk_out_off[t] + i * m + j] = number of rows of the segment with
 * x[col_i][row] == 1 and x[col_j][row] == 1: exact int32, symmetric, the diagonal holds the column
 * counts.  The caller lays the blocks' m * m outputs out so that they tile [0, n_ones).
 * A UNIT is the work of one work-group: block unit_blk[u], the pair of 64-column tiles unit_ti[u] <=
 * unit_tj[u] of that block's columns (tile k holds the column positions [64 k, 64 k + 64)), and the rows
 * [unit_row0[u], + row_chunk) of its segment, clipped to blk_n.  The caller lists, for every block,
 * every tile pair ti <= tj over every row chunk row0 = 0, row_chunk, 2 row_chunk, ... < blk_n; units of
 * one block add into the same elements by integer atomics (the order of integer additions is free), so
 * the entry first sets all of `ones` to zero with a kernel of its own: every element is written for
 * every shape, and nothing depends on what `ones` held.  The bit planes of a pass (64 columns x 1024
 * rows, two tiles) live in LDS only; a block of any width is tiled, none is refused.  The number of
 * work-groups is the number of units: the row and pair work, whatever the number of blocks.
 * ones: [n_ones] int32. */
#define DPL_PAIR_TILE 64
#define DPL_PAIR_ROW_CHUNK 8192 /* the row chunk the package passes */
int dpl_pair_ones(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                  const int32_t *blk_col, const int64_t *blk_col_off, const int32_t *blk_m, const int64_t *blk_row_off,
                  const int32_t *blk_n, const int64_t *blk_out_off, int64_t n_blocks, const int32_t *unit_blk,
                  const int32_t *unit_ti, const int32_t *unit_tj, const int32_t *unit_row0, int64_t n_units, int row_chunk,
                  int32_t *ones, int64_t n_ones, void *stream);

/* ==== continuous data (deeprob.spn.learning.learnspn_cont: all-Gaussian learn_spn) =================
 * `xf` is the training set as float32, COLUMN MAJOR: xf[col * n_rows + row]; `row_index`, segments and
 * the buffer contract are those above.  No float atomics; every float64 sum below has the stated order;
 * a run repeats bit for bit.  Scratch (`partial` of dpl_rdc_gram) is an output like any other: every
 * element of it is written, and what it holds on return is not specified further. */

/* Moments: for item i (column item_col[i] over its segment of n = item_n[i] rows), in float64 and two
 * passes: 256 partial sums (partial l takes rows l, l + 256, ... in order, from 0.0), added in order
 * of l, divided by n: the mean; then the same sum of (x - mean) * (x - mean), divided by n: the
 * POPULATION variance.  moments: [n_items * 2] float64, mean at 2 i, variance at 2 i + 1.
 * The host rules: a column with variance <= 1e-8 is constant (np.isclose(var, 0), learnspn.py:132);
 * the leaf is Gaussian(mean, max(sqrt(variance), 1e-5)) (leaf.py:529-530). */
int dpl_column_moments(const float *xf, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                       const int32_t *item_col, const int64_t *item_row_off, const int32_t *item_n, int64_t n_items,
                       double *moments, void *stream);

/* ECDF ranks (utils/data.py:182, scipy.stats.rankdata(method='max')): for item i and position r of its
 * segment, ranks[item_out_off[i] + r] = number of rows of the segment whose value is <= the value of
 * row r.  `sorted` holds, at [item_out_off[i], + item_n[i]), the item's values in non-decreasing order
 * (the caller sorts them on the device); the rank is the upper bound of the row's value in that run, so
 * a run of ties gets the position of its last member ("max").  Block b covers positions block_row0[b]
 * .. + 256 of item block_item[b].  ranks: [n_out] int32, n_out = the sum of item_n, every element
 * written (1 <= rank <= n). */
int dpl_ecdf_ranks(const float *xf, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                   const int32_t *item_col, const int64_t *item_row_off, const int32_t *item_n,
                   const int64_t *item_out_off, int64_t n_items, const int32_t *block_item, const int32_t *block_row0,
                   int64_t n_blocks, const float *sorted, int32_t *ranks, int64_t n_out, void *stream);

/* Random-feature Gram matrices of the continuous RDC score (rdc.py:137-177).  Task t has n = task_n[t]
 * rows and F = task_f[t] = m * k features, k per column; the ranks of its p-th column are at
 * ranks[task_rank_off[t] + p * n ...] (dpl_ecdf_ranks order), its draws at w[task_feat_off[t] + f],
 * b[same], f = p * k + j (float32, widened).  In float64, one operation at a time:
 *   u = f64(rank) / f64(n);   phi[r][f] = sin(u * w[f] + b[f]);
 *   S[f] = sum_r phi[r][f];   G[f][g] = sum_r phi[r][f] * phi[r][g].
 * phi is never stored: UNIT u forms it for rows [unit_row0[u], + unit_rows[u]) of task unit_task[u] and
 * the two 32-feature tiles that start at unit_i0[u] <= unit_j0[u], 32 rows at a time in LDS, and adds
 * the products into partial[u * DPL_GRAM_PARTIAL ...]: 32 x 32 products (row major) and then 32 column
 * sums of the tile at unit_i0 (features >= F and rows past the unit count as 0).  With use_mfma == 0 the
 * products are added on the VALU row by row in increasing row order; with use_mfma != 0 on
 * v_mfma_f64_16x16x4_f64, blocks of 4 rows in increasing order, the 4 rows of a block in the matrix
 * core's own (fixed) order.  The column sums are added row by row in both.  GROUP g -- one tile pair of one task -- adds the partials of its units
 * group_unit0[g] .. + group_units[g] in that order (the caller lists a group's units by increasing
 * row) and writes G[task_g_off[t] + f * F + g'] for the tile and, when the two tiles differ, its
 * mirror image; the group with unit_i0 == unit_j0 also writes S[task_feat_off[t] + f].  The caller
 * lists every tile pair i0 <= j0 of every task, so every element of G and S is written (products
 * commute exactly, so G is bitwise symmetric).  partial: [n_units * DPL_GRAM_PARTIAL] float64; the
 * caller keeps n_units * DPL_GRAM_PARTIAL * 8 bytes under 256 MiB by splitting the groups of a
 * generation, or of one wide task, over several calls.  Which of the two forms the package uses was
 * picked by measurement ("rdc on continuous columns"). */
#define DPL_GRAM_TILE 32
#define DPL_GRAM_PARTIAL 1056 /* 32 * 32 + 32 */
int dpl_rdc_gram(const int32_t *ranks, int64_t n_ranks, const float *w, const float *b, int64_t n_feat, int k,
                 const int32_t *task_n, const int32_t *task_f, const int64_t *task_rank_off,
                 const int64_t *task_feat_off, const int64_t *task_g_off, int n_tasks, const int32_t *unit_task,
                 const int32_t *unit_i0, const int32_t *unit_j0, const int32_t *unit_row0, const int32_t *unit_rows,
                 int64_t n_units, const int32_t *group_unit0, const int32_t *group_units, int64_t n_groups,
                 int use_mfma, double *partial, double *G, int64_t n_g, double *S, void *stream);

/* ---- k-means on float columns: the four entries above restated.  A column is ONE feature, unscaled
 * (cluster.py:58-65); centroids at cent[task_cent_off[t] + (r * n_clusters + c) * ncols_t + p]; the
 * squared distance (f64(x) - cent)^2 accumulates in float64 over the columns in order, ties to the
 * lower index; restarts, steps and the winner are DESIGN.md's. */

/* cent = the row at position seeds[(t * n_restarts + r) * n_clusters + c] of task t's segment. */
int dpl_kmeansf_init(const float *xf, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                     const int32_t *task_col_off, const int32_t *col_index, const int64_t *task_row_off,
                     const int32_t *task_n, const int64_t *task_cent_off, const int32_t *seeds, int n_tasks,
                     int n_restarts, int n_clusters, double *cent, int64_t n_cent, void *stream);

/* As dpl_kmeans_assign (`labels` and `changed` updated in place). */
int dpl_kmeansf_assign(const float *xf, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                       const int32_t *task_col_off, const int32_t *col_index, const int64_t *task_row_off,
                       const int32_t *task_n, const int64_t *task_cent_off, const int64_t *task_lab_off,
                       const int32_t *block_task, const int32_t *block_row0, int64_t n_blocks, int n_restarts,
                       int n_clusters, const double *cent, uint8_t *labels, int64_t n_lab, int first,
                       int32_t *changed, void *stream);

/* Centroids from labels (`cent` updated in place): item i is column position item_p[i] of task
 * item_task[i]; per restart and cluster c the mean of the column over the rows labelled c: 256
 * partial sums (partial l takes, in order, the rows among l, l + 256, ... that are labelled c, from
 * 0.0), added in order of l, divided by the number of such rows; a cluster without rows keeps its
 * centroid. */
int dpl_kmeansf_update(const float *xf, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                       const int32_t *task_col_off, const int32_t *col_index, const int64_t *task_row_off,
                       const int32_t *task_n, const int64_t *task_cent_off, const int64_t *task_lab_off,
                       const int32_t *item_task, const int32_t *item_p, int64_t n_items, int n_restarts,
                       int n_clusters, const uint8_t *labels, int64_t n_lab, double *cent, void *stream);

/* As dpl_kmeans_inertia: the same 256 partial sums, and the cluster sizes. */
int dpl_kmeansf_inertia(const float *xf, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                        const int32_t *task_col_off, const int32_t *col_index, const int64_t *task_row_off,
                        const int32_t *task_n, const int64_t *task_cent_off, const int64_t *task_lab_off, int n_tasks,
                        int n_restarts, int n_clusters, const double *cent, const uint8_t *labels, int64_t n_lab,
                        double *inertia, int32_t *sizes, void *stream);

/* ==== histograms of float columns (splitting/entropy.py, gini.py: np.histogram(col, 'scott'); gvs.py:184-190:
 * np.histogram_bin_edges(col, 'fd') and np.histogram2d on them) ====================================================
 * An ITEM is one column over one row segment, as above, with the three numbers of numpy's uniform bins: lo, hi
 * (float32: the item's min and max, or min - 0.5 and max + 0.5 when they are equal) and bins >= 1 (the host derives it
 * from the bin width in float64: deeprob/spn/learning/splitting/hist.py).  The EDGES are float32, what np.linspace
 * gives for float32 ends:
 *   step = fl32(fl32(hi - lo) / fl32(bins));  edge[i] = fl32(fl32(fl32(i) * step) + lo), i < bins;  edge[bins] = hi
 * -- one multiply, then one add, never fused.  The BIN of a value x (lo <= x <= hi) is (the number of i <= bins with
 * edge[i] <= x) - 1, and bins - 1 for x == hi: the largest b <= bins - 1 with edge[b] <= x.  That is the bin np.histogram
 * and np.histogram2d count x in.  A multiply-and-truncate guess is only the starting point of the search; the edges
 * decide.
 * Caps: a column has at most DPL_HIST_MAX_BINS bins (a code is a uint16 and the count table of an item lives in LDS);
 * a pair's joint table has at most DPL_HIST_MAX_CELLS cells: 48 KiB of int32 which, with the 1024 + 12 float64
 * marginals a table of that size can have at most and the 256 partial sums, stays under the 64 KiB a work-group gets
 * without asking for more, so two work-groups at the cap, and five at the 80 x 80 of 20 000 Gaussian rows, share the
 * 160 KiB of a compute unit (one resident work-group per compute unit was avoided).  The package
 * raises ValueError over a cap, naming the column, before any launch. */
#define DPL_HIST_MAX_BINS 1024
#define DPL_HIST_MAX_CELLS 12288

/* Bin codes: codes[item_out_off[i] + r] = the bin of row r of item i's segment, item major like the ranks of
 * dpl_ecdf_ranks.  Block b covers positions block_row0[b] .. + 256 of item block_item[b].  codes: [n_out] uint16,
 * n_out = the sum of item_n, every element written (code < bins). */
int dpl_hist_codes(const float *xf, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                   const int32_t *item_col, const int64_t *item_row_off, const int32_t *item_n,
                   const int64_t *item_out_off, const float *item_lo, const float *item_hi, const int32_t *item_bins,
                   int64_t n_items, const int32_t *block_item, const int32_t *block_row0, int64_t n_blocks,
                   uint16_t *codes, int64_t n_out, void *stream);

/* Counts of the codes: counts[item_count_off[i] + b] = the number of r < item_n[i] with codes[item_code_off[i] + r]
 * == b, b < item_bins[i] <= DPL_HIST_MAX_BINS: exact int32 (LDS integer atomics), one work-group per item.  The
 * caller lays the items' outputs out so that they tile [0, n_counts).  A code >= bins is not counted. */
int dpl_code_counts(const uint16_t *codes, int64_t n_codes, const int64_t *item_code_off, const int32_t *item_n,
                    const int32_t *item_bins, const int64_t *item_count_off, int64_t n_items, int32_t *counts,
                    int64_t n_counts, void *stream);

/* G statistic of two coded columns (gvs.py:190-197 on the table np.histogram2d gives): pair q has the codes of its two
 * columns at codes[pair_off_a[q] ...] and codes[pair_off_b[q] ...], n = pair_n[q] of each, with ba = pair_bins_a[q]
 * and bb = pair_bins_b[q] bins; ba * bb <= max_cells <= DPL_HIST_MAX_CELLS and ba + bb <= max_bins_sum, the largest
 * of the launch (they size the LDS of every work-group; a pair over them gets NaN).  One work-group per pair: the joint
 * counts c[a][b] in exact int32, then in float64, in this order of operations:
 *   h[a][b] = c[a][b] + 2^-23;  m1[a] = h[a][0] + h[a][1] + ...;  m2[b] = h[0][b] + h[1][b] + ...;
 *   t[a][b] = h * log(h / (m1[a] * m2[b] / n));  256 partial sums (partial l takes the cells l, l + 256, ... of the row
 *   major table in order, from 0.0), added in order of l (the convention of dpl_column_moments);  g = 2 * that sum.
 * Tables need not be square and are as a rule larger than the work-group.  g: [n_pairs] float64. */
int dpl_pair_g_codes(const uint16_t *codes, int64_t n_codes, const int64_t *pair_off_a, const int64_t *pair_off_b,
                     const int32_t *pair_n, const int32_t *pair_bins_a, const int32_t *pair_bins_b, int64_t n_pairs,
                     int max_bins_sum, int max_cells, double *g, void *stream);

/* ==== Gaussian-mixture row splits (splitting/cluster.py:14-38: GaussianMixture(n, n_init=3); this project's definition:
 * DESIGN.md 14.5) ==================================================================================================
 * One EM iteration of every listed (task, initialisation) PAIR of a generation: dpl_gmm_estep is the density pass,
 * dpl_gmm_mstats the weighted moments; the Cholesky factors, their inverses and the M-step arithmetic on the moments are
 * the host's.  `x` is the uint8 matrix (is_float == 0) or the float32 matrix `xf` (is_float != 0), column major as above.
 *
 * FEATURES are those of the k-means above: task t has F = task_f[t] features, feature f reads column
 * feat_col[task_feat_off[t] + f]; with uint8 data feat_val[same] < 0 takes the column's value itself (a column with K <= 2)
 * and feat_val = v >= 0 the indicator of value v (one of the K one-hot features of a column with K > 2); with float32 data
 * feat_val is not read and the feature is the value widened.  Feature values are float64.  The rows of task t are
 * row_index[task_row_off[t] .. + task_n[t]); row r of task t under initialisation i has its label, lse and
 * responsibilities at position i * n_lab + task_lab_off[t] + r.
 *
 * Pair a is task pair_task[a] under initialisation pair_init[a]; its PARAMETERS are at par[pair_par_off[a] + c * (1 + F +
 * F * F) ...] for component c < n_comp <= DPL_MAX_CLUSTERS: k_c = log pi_c - 0.5 F log(2 pi) - sum log diag L_c, then
 * mu_c[F], then W_c = L_c^-1 as an F x F row major matrix whose upper triangle holds 0.0.  A pair that is not listed is not
 * touched: `resp`, `labels` and `lse` are written for every row of every LISTED pair and are otherwise left alone (they
 * are outputs updated in place, like `labels` of dpl_kmeans_assign); lse_sum and stats are compact over the listed pairs and
 * every element of them is written. */

/* E-step.  Block b covers rows block_row0[b] .. + 256 of pair block_pair[b]; the caller lists every 256-row block of every
 * listed pair.  For a row with features x and each component c, in float64, one operation at a time:
 *   d_j = x_j - mu_c[j];   y_i = sum_j W_c[i][j] * d_j, from 0.0 over j = 0, 1, ... in order (one multiply, one add per term;
 *   the terms j > i are products with the stored 0.0, or skipped: whole 32-feature tiles above the diagonal are skipped);
 *   q = sum_i y_i * y_i from 0.0 in order of i;   lp_c = k_c + (-0.5 * q);
 * never the expanded form x^T P x - 2 x^T P mu + mu^T P mu.  Then m = the largest lp_c, label = the first c that attains
 * it, s = sum_c exp(lp_c - m) from 0.0 in order of c, lse = m + log(s), resp_c = exp(lp_c - lse).  W_c is taken through LDS
 * a 32 x 32 tile at a time and a thread holds the 32 y_i of one tile row: nothing is sized by F, any F is tiled.  Built on the
 * VALU only (a thread per row, the tile of W_c broadcast from LDS); no matrix-core form was built.
 * lse_sum[a] = the sum of pair a's lse: 256 partial sums (partial l takes rows l, l + 256, ... in order, from 0.0), added in
 * order of l (a second kernel over `lse`).  resp: [n_init * n_lab * n_comp] float64; labels: [n_init * n_lab] uint8; lse:
 * [n_init * n_lab] float64; lse_sum: [n_pairs] float64. */
int dpl_gmm_estep(const void *x, int is_float, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                  const int64_t *task_row_off, const int32_t *task_n, const int64_t *task_lab_off,
                  const int32_t *task_feat_off, const int32_t *task_f, const int32_t *feat_col, const int32_t *feat_val,
                  const int32_t *pair_task, const int32_t *pair_init, const int64_t *pair_par_off, int64_t n_pairs,
                  const int32_t *block_pair, const int32_t *block_row0, int64_t n_blocks, int n_init, int n_comp,
                  const double *par, double *resp, uint8_t *labels, double *lse, int64_t n_lab, double *lse_sum,
                  void *stream);

/* Weighted moments about a PIVOT (built: the one-pass pivoted form, not the two-pass one; never raw moments about the
 * origin).  For listed pair a and component c, with w_r = resp[(i * n_lab + task_lab_off[t] + r) * n_comp + c], the pivot
 * p = mu_c of the pair's parameters (par[pair_par_off[a] + c * (1 + F + F * F) + 1 ...]; k_c and W_c are not read) and
 * a_rf = x_rf - p_f, stats[pair_stat_off[a] + c * (1 + F + F * F) ...] receives
 *   N = sum_r w_r;   s[f] = sum_r w_r * a_rf;   M[g][f] = sum_r (w_r * a_rf) * a_rg,  F x F row major,
 * each product formed in that order.  Organised like dpl_rdc_gram, whose tile products, partial layout and group sums
 * it shares: UNIT u is rows [unit_row0[u], + unit_rows[u]) of pair unit_pair[u], component unit_comp[u], and the 32-feature
 * tiles at unit_i0[u] <= unit_j0[u]; the weighted factor w_r * a_rf runs over the tile at unit_i0, the plain factor a_rg
 * over the tile at unit_j0 (both tiles are staged even when they coincide).  A unit adds its rows 32 at a time into
 * partial[u * DPL_GMM_PARTIAL ...]: the DPL_GRAM_PARTIAL numbers of dpl_rdc_gram (products with use_mfma == 0 on the VALU
 * row by row, with use_mfma != 0 on v_mfma_f64_16x16x4_f64 in blocks of 4 rows; the sums s of the tile at unit_i0 row by
 * row) and then the sum of w_r row by row.  GROUP g adds the partials of its units group_unit0[g] .. + group_units[g] in
 * that order and writes M[g'][f'] for f' in the tile at i0 and g' in the tile at j0 and, when the tiles differ, the same
 * number at M[f'][g']; the group with i0 == j0 also writes s over its tile, and the one with i0 == j0 == 0 writes N.  The
 * caller lists every tile pair i0 <= j0 of every component of every listed pair, so every element of stats is written.  In
 * a diagonal tile M[g][f] and M[f][g] differ in the rounding of the weighted factor: the host reads the LOWER triangle
 * (g >= f), where the weighted factor is the one of the lower index.  partial: [n_units * DPL_GMM_PARTIAL] float64, scratch
 * like that of dpl_rdc_gram, kept under 256 MiB by splitting the groups over several calls. */
#define DPL_GMM_PARTIAL 1064 /* DPL_GRAM_PARTIAL + 1, rounded up to a multiple of 8 */
int dpl_gmm_mstats(const void *x, int is_float, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                   const int64_t *task_row_off, const int32_t *task_n, const int64_t *task_lab_off,
                   const int32_t *task_feat_off, const int32_t *task_f, const int32_t *feat_col, const int32_t *feat_val,
                   const int32_t *pair_task, const int32_t *pair_init, const int64_t *pair_par_off,
                   const int64_t *pair_stat_off, int64_t n_pairs, const int32_t *unit_pair, const int32_t *unit_comp,
                   const int32_t *unit_i0, const int32_t *unit_j0, const int32_t *unit_row0, const int32_t *unit_rows,
                   int64_t n_units, const int32_t *group_unit0, const int32_t *group_units, int64_t n_groups, int n_comp,
                   const double *par, const double *resp, int64_t n_lab, int use_mfma, double *partial, double *stats,
                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPROB_LEARN_H */
