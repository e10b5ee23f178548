/*
 * deeprob_clt.h -- C ABI of libdeeprob_clt.so (gfx950 / MI355X): binary Chow-Liu trees
 * (deeprob.spn.structure.cltree.BinaryCLT) learned and queried on the device.
 *
 * The reference is Python on numpy (deeprob/spn/structure/cltree.py, utils/statistics.py:64-109).
 * Learning needs one statistic of the data, the co-occurrence counts X^T X of the 0/1 matrix: they
 * are computed here in exact integers from bit planes (dpc_pack_bits, dpc_pair_counts); the float32
 * arithmetic after them, the spanning tree and the parameters stay on the host
 * (deeprob/utils/statistics.py, deeprob/utils/graph.py of this package).  The three queries -- log
 * likelihood with marginalised entries, MPE and conditional sampling -- run one THREAD PER ROW over
 * a column-major copy of the query rows (dpc_pack_query).
 *
 * The tree (D variables, D <= DPC_MAX_D; positions in the scope, not variable ids)
 *   bfs[D]          breadth-first order from the root, bfs[0] = root;
 *   parent[D]       parent[i] = parent of i, -1 at the root;
 *   params[D][2][2] float32, params[i][l][k] = log P(X_i = k | X_parent(i) = l); the two rows of the
 *                   root are equal;
 *   child_off[D+1], child_idx[D-1]   the children of i are child_idx[child_off[i] .. child_off[i+1]),
 *                   listed in DECREASING position in `bfs` (the order in which the reference's loop
 *                   over reversed(bfs[1:]) adds them to their parent, cltree.py:226-241).
 * The arrays are trusted to describe one tree: nothing here can check them without a host read.
 *
 * Order of operations of the queries (float32 unless stated; built with -ffp-contract=off)
 *   m_j[k]   = ((0 + t_c1[k]) + t_c2[k]) + ...  over the children c1, c2, ... of j in list order: a
 *              parent PULLS, nothing is added into a shared location;
 *   t_j[l]   = params[j][l][x_j] + m_j[x_j]                         when x_j is observed,
 *            = R(params[j][l][0] + m_j[0], params[j][l][1] + m_j[1]) when it is NaN, with
 *              R = lse for the log likelihood and for sampling, R = max for MPE;
 *   lse(a,b) = hi + log1pf(expf(lo - hi)), hi = max(a, b), lo = min(a, b); -inf when hi = -inf;
 *   nodes are visited in reversed `bfs` order on the way up and in `bfs` order on the way down.
 *
 * Every pointer is a DEVICE pointer; `stream` is a hipStream_t passed as void*; kernels are enqueued
 * asynchronously on it and no entry point synchronises or allocates.
 *
 * Buffer contract (the one of include/deeprob_hip.h, repeated):
 *   1. an entry point writes only its output arguments, over their documented extent;
 *   2. it writes every element of every output, for every legal shape (one row, one column, ragged
 *      tails included); `work` is scratch: it is an output whose contents on return are unspecified;
 *   3. nothing it does depends on what the outputs (or `work`) held on entry;
 *   4. it leaves its `const` inputs alone.
 * Counts are exact integers.  No floating-point value is accumulated atomically, every
 * floating-point sum has the fixed order stated above or at its entry point, and no kernel waits on
 * another work-group.
 *
 * The return value is 0 on success and a negative DPC_E* code otherwise; dpc_last_error() returns
 * a thread-local message for the last failure.
 */
#ifndef DEEPROB_CLT_H
#define DEEPROB_CLT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPC_OK 0
#define DPC_EINVAL (-1)  /* bad argument (null pointer, size out of domain) */
#define DPC_ELAUNCH (-3) /* hipLaunch / runtime error                        */

#define DPC_MAX_D 4096 /* largest number of variables: D * D counts and 2 * D floats of state per row */
#define DPC_MISSING 2  /* the code of a NaN entry in the output of dpc_pack_query                   */

const char *dpc_last_error(void);
int dpc_abi_version(void);

/* Training rows as bit planes.  x: [n, d] float32 row major (the layout users hold), entries 0 or 1.
 * planes: [d, W] uint64 with W = (n + 63) / 64; bit (r % 64) of planes[c * W + r / 64] is set iff
 * x[r][c] == 1.  The bits of the last word past row n - 1 are zero. */
int dpc_pack_bits(const float *x, int64_t n, int d, uint64_t *planes, void *stream);

/* Query rows, column major.  x: [b, d] float32 row major, entries 0, 1 or NaN (= marginalised).
 * codes: [d, b] uint8, codes[c * b + r] = DPC_MISSING for NaN, 0 for 0, 1 for anything else. */
int dpc_pack_query(const float *x, int64_t b, int d, uint8_t *codes, void *stream);

/* ones[i * d + j] = number of rows r < n with x[r][i] == x[r][j] == 1, from the planes of
 * dpc_pack_bits (n_words = W): AND + popcount, integer adds only, so the result is exact whatever
 * the order; symmetric, the diagonal holds the column counts.  n < 2^31.  ones: [d, d] int32. */
int dpc_pair_counts(const uint64_t *planes, int64_t n_words, int d, int32_t *ones, void *stream);

/* out[r] = log P(the observed entries of row r).  A row without NaN takes the gather path: the sum
 * of params[i][x_parent(i)][x_i] over i = 0 .. d-1 IN THIS ORDER, accumulated in float64 and rounded
 * once to float32.  A row with NaN takes the upward pass above with R = lse and ends at the root with
 * params[root][0][x] + m_root[x] (observed) or lse over both values (NaN): cltree.py:205-261.
 * codes: the output of dpc_pack_query for the same b, d.  work: [2 * d * b] float32 scratch. */
int dpc_clt_log_likelihood(const uint8_t *codes, int64_t b, int d, const int32_t *bfs, const int32_t *parent,
                           const float *params, const int32_t *child_off, const int32_t *child_idx, float *work,
                           float *out, void *stream);

/* MPE (cltree.py:297-316): the upward pass with R = max, then in `bfs` order every NaN entry j gets
 * the k with the larger params[j][x_parent(j)][k] + m_j[k] (row 0 at the root), k = 0 on a tie.
 * out: [b, d] float32; observed entries are copied from x bit for bit.  x: the rows `codes` was made
 * from. */
int dpc_clt_mpe(const float *x, const uint8_t *codes, int64_t b, int d, const int32_t *bfs, const int32_t *parent,
                const float *params, const int32_t *child_off, const int32_t *child_idx, float *work, float *out,
                void *stream);

/* Conditional sampling (cltree.py:318-337): the upward pass with R = lse, then in `bfs` order every
 * NaN entry j is set to 1 iff u < expf(params[j][x_parent(j)][1] + m_j[x_parent(j)]) in float32 (at
 * the root: params[root][0][1] + m_root[1]) -- the reference's expression, index of the message
 * included.  u = (splitmix64(seed + ctr * 0x9E3779B97F4A7C15) >> 40) / 2^24 with
 * ctr = (row0 + r) * d + j: the generator of dpk_flat_spn_topdown; `row0` lets a caller sample a
 * long batch in pieces.  out: [b, d] float32; observed entries are copied from x bit for bit. */
int dpc_clt_sample(const float *x, const uint8_t *codes, int64_t b, int d, const int32_t *bfs, const int32_t *parent,
                   const float *params, const int32_t *child_off, const int32_t *child_idx, uint64_t seed,
                   int64_t row0, float *work, float *out, void *stream);

/* ---- Cutset networks (deeprob.spn.structure.cnet.BinaryCNet; reference spn/structure/cnet.py) -------
 *
 * A cutset network is an OR tree that conditions on one binary variable per node, with a Chow-Liu
 * tree at every leaf.  Learning is LEVEL SYNCHRONOUS: a generation is every open node ("task") of one
 * depth.  Task t owns the rows rows[seg_off[t] .. seg_off[t+1]) of a row-index array (indices into
 * the training matrix x) and a set of still-active columns; the launches of a generation -- gather-pack,
 * pair counts, scores, partition -- do not depend on the number of tasks.
 *
 * Planes of a generation: [d, n_words] uint64.  Task t owns the words word_off[t] .. word_off[t+1) of
 * every plane, word_off[t+1] - word_off[t] = (n_t + 63) / 64 with n_t = seg_off[t+1] - seg_off[t]: every
 * segment starts on a word boundary, a task of 0 rows owns no word, word_off[n_tasks] = n_words.
 * seg_off, word_off: [n_tasks + 1] int32, non-decreasing; they and `rows` are trusted (they index
 * device memory), except that a row index outside 0 .. n-1 packs as a row of zeros. */

/* Bit (p % 64) of planes[c * n_words + word_off[t] + p / 64] is set iff x[rows[seg_off[t] + p]][c] == 1,
 * p < n_t; the bits of a task's last word past its last row are zero.  All d columns are packed.
 * x: [n, d] float32 row major. */
int dpc_cnet_gather_pack(const float *x, int64_t n, int d, const int32_t *rows, const int32_t *seg_off,
                         const int32_t *word_off, int n_tasks, int64_t n_words, uint64_t *planes, void *stream);

/* ones[t][i][j] = rows of task t with x_i = x_j = 1, for n_tasks <= 65535 consecutive tasks: AND +
 * popcount over the task's words only, exact integers, about d * d * n_words popcounts in all
 * whatever the number of tasks.  word_off: the [n_tasks + 1] entries of these tasks (a pointer into
 * the generation's array; the values stay offsets into the planes).  ones: [n_tasks, d, d] int32,
 * all zero for a task of 0 rows. */
int dpc_cnet_pair_counts(const uint64_t *planes, int64_t n_words, int d, const int32_t *word_off, int n_tasks,
                         int32_t *ones, void *stream);

/* The cut scores of cnet.py:168-198, in float64 from the exact counts (the reference evaluates them in
 * float32).  For task t with n = seg_off[t+1] - seg_off[t] rows, c_i = ones[t][i][i], over the columns
 * with active[t][i] != 0 only (d_a of them), a2 = 2 alpha, a4 = 4 alpha:
 *   p_i1 = (c_i + a2) / (n + a4), p_i0 = 1 - p_i1;
 *   mean_entropy = -S / d_a, S = sum over active i IN INCREASING i of (p_i0 ln p_i0 + p_i1 ln p_i1);
 *   cells of (x_i = a, x_j = b): c11 = ones[i][j], c10 = c_i - c11, c01 = c_j - c11,
 *                                c00 = ((n - c_i) - c_j) + c11;
 *   h_ij1 = -(q0 ln q0 + q1 ln q1) with q0 = (c10 + a2) / (c_i + a4), q1 = (c11 + a2) / (c_i + a4);
 *   h_ij0 = -(q0 ln q0 + q1 ln q1) with q0 = (c00 + a2) / ((n - c_i) + a4), q1 = (c01 + a2) / ((n - c_i) + a4);
 *   H_i,a = (sum over active j != i IN INCREASING j of h_ija) / (d_a - 1)   (0 when d_a = 1);
 *   gain_i = mean_entropy - ((c_i / n) H_i,1 + (1 - c_i / n) H_i,0)          (c_i / n := 0 when n = 0).
 * gains: [n_tasks, d] float64, -inf at an inactive column.  stats: [n_tasks, 2] float64 = (mean_entropy,
 * the largest gain).  best: [n_tasks, 2] int32 = (the smallest i with the largest gain, c_i of it);
 * (-1, 0) with a gain of -inf when no column is active.  n_tasks <= 65535.  active: [n_tasks, d] uint8. */
int dpc_cnet_scores(const int32_t *ones, const int32_t *seg_off, const uint8_t *active, int n_tasks, int d, double alpha,
                    double *gains, double *stats, int32_t *best, void *stream);

/* Stable partition of every task with cut[t] >= 0 by the bits of plane cut[t]:
 * rows_out[out_off[t] ..] = the task's row indices with x_cut = 0 in their order, then those with
 * x_cut = 1 in their order (n_t entries in all); child_n[t] = (zeros, ones).  A task with cut[t] = -1
 * copies nothing and gets child_n[t] = (0, 0).  The caller lays the splitting tasks out back to back
 * (out_off[t] = the rows of the splitting tasks before t), so that the segments tile rows_out.
 * cut, out_off: [n_tasks] int32; child_n: [n_tasks, 2] int32. */
int dpc_cnet_partition(const uint64_t *planes, int64_t n_words, const int32_t *rows, const int32_t *seg_off,
                       const int32_t *word_off, const int32_t *cut, const int32_t *out_off, int n_tasks,
                       int32_t *rows_out, int32_t *child_n, void *stream);

/* out[r] = log P(the observed entries of row r) under a cutset network.  The model (trusted tables):
 *   node_col[n_nodes]       the cut column of an OR node, -1 at a leaf; node 0 is the root;
 *   node_child[n_nodes][2]  the children for x_col = 0 / 1; at a leaf, node_child[k][0] = its leaf number;
 *   node_logw[n_nodes][2]   float64 log weights (unused at a leaf);
 *   leaf_meta[n_leaves][3]  (d_l, offset into leaf_ints, offset into leaf_params);
 *   leaf_ints               per leaf: col[d_l] (the column of each position of the leaf's scope), then
 *                           bfs[d_l], parent[d_l], child_off[d_l + 1], child_idx[d_l - 1] of its tree;
 *   leaf_params             per leaf: params[d_l][2][2] float32.
 * A row WITHOUT NaN descends one path: the float64 sum of node_logw[k][x_col] from the root to the
 * leaf, then of the leaf's params[i][x_parent(i)][x_i] over i = 0 .. d_l - 1, in this order, rounded once
 * to float32.  A row WITH NaN is evaluated depth first, V(root) rounded to float32, where
 *   V(leaf)    = the value dpc_clt_log_likelihood gives the leaf's tree on the leaf's columns (float32:
 *                the gather path if none of them is NaN, else the upward pass with R = lse);
 *   V(OR node) = node_logw[k][x] + V(child x)                                       x_col observed,
 *              = lse64(node_logw[k][0] + V(child 0), node_logw[k][1] + V(child 1))   x_col NaN,
 *   lse64(a,b) = hi + log1p(exp(lo - hi)) in float64, -inf when hi = -inf.
 * levels: the largest number of nodes on a path from the root to a leaf (1 for a lone leaf);
 * max_leaf_d: the largest d_l.  work: b * (12 * levels + 8 * max_leaf_d) bytes of scratch, 8-byte
 * aligned: per row a stack of `levels` (float64, int32) entries and the 2 * max_leaf_d floats of the
 * upward pass.  codes: the output of dpc_pack_query for the same b, d. */
int dpc_cnet_log_likelihood(const uint8_t *codes, int64_t b, int d, int n_nodes, const int32_t *node_col,
                            const int32_t *node_child, const double *node_logw, const int32_t *leaf_meta,
                            const int32_t *leaf_ints, const float *leaf_params, int levels, int max_leaf_d, void *work,
                            float *out, void *stream);

/* ---- Queries of a cutset network that fill a row in: exact MPE and exact conditional sampling, one launch each ----
 *
 * x: [b, d] float32 row major, NaN = unknown; codes: the output of dpc_pack_query for the same rows.  out: [b, d]
 * float32: an observed entry comes back bit for bit, a NaN entry becomes 0.0 or 1.0 -- except a column that is neither
 * cut on the chosen path nor in the chosen leaf's scope (hand-built tables only), which is returned as given.
 * choice: [b] int32 or null, the NODE number of the chosen leaf.  The model is the tables of
 * dpc_cnet_log_likelihood (M = n_nodes, nodes numbered breadth first, left child before right) and
 *   node_parent[M]   2 * parent + side (side = which child of the parent the node is), -1 at the root.
 * Both walk the OR tree depth first exactly as dpc_cnet_log_likelihood does for a row with NaN (a row without NaN
 * takes the same walk: one path).  Every node returns a pair (value, leaf):
 *   a leaf           (V(leaf), itself);
 *   x_col observed   (node_logw[k][x] + V(child x), the leaf child x returned);
 *   x_col NaN        both children return (value V_c, leaf_c), a_c = node_logw[k][c] + V_c in float64, and
 *     sampling:  t = lse64(a_0, a_1), p1 = exp(a_1 - t) in float64 (0 when t = -inf); the node returns
 *                (t, leaf_1 if (double)u(k) < p1 else leaf_0);
 *     MPE:       (a_1, leaf_1) if a_1 > a_0, else (a_0, leaf_0): a tie goes to child 0.
 * V(leaf) for sampling is the V(leaf) of dpc_cnet_log_likelihood; for MPE it is the same with R = max in the upward
 * pass (the gather path if none of the leaf's columns is NaN).  The leaf drawn inside a subtree is an exact draw given
 * that subtree and the draw at the parent picks between the two sides with their posterior odds, so the pair the root
 * returns names a leaf with exactly its posterior probability (or the leaf of a most probable completion), in ONE
 * bottom-up walk.  Then, from that leaf up to the root through node_parent, every NaN cut variable takes the side the
 * path went; and the leaf's NaN columns are filled in `bfs` order after the leaf's upward pass (R = lse / max): for
 * position j with parent value xp (row 0 at the leaf's root), a_k = params[j][xp][k] + m_j[k] in float32,
 *     sampling:  the entry is 1 iff u(M + col_j) < expf(a_1 - lse(a_0, a_1)) in float32: the normalised conditional
 *                (NOT the expression of dpc_clt_sample, which is exact only without evidence below j);
 *     MPE:       the entry is 1 iff a_1 > a_0 (the rule of dpc_clt_mpe).
 * u(i) = the generator of dpc_clt_sample with ctr = (row0 + r) * (M + d) + i: OR node k draws with i = k, column c with
 * i = M + c, so a row's output depends only on (seed, row0 + r, the row); `row0` lets a caller sample a long batch in
 * pieces.  levels, max_leaf_d: as for dpc_cnet_log_likelihood; a row whose stack would grow past `levels` gets NaN in
 * all of out[r] and choice[r] = -1, with no write past the stack.  work: b * (16 * levels + 8 * max_leaf_d) bytes of
 * scratch, 8-byte aligned: per row the stack of `levels` (float64, int32) entries, one more int32 per level for the
 * leaf carried upward, and the 2 * max_leaf_d floats of the leaf pass.  b = 0 writes nothing. */
int dpc_cnq_mpe(const float *x, const uint8_t *codes, int64_t b, int d, int n_nodes, const int32_t *node_col,
                const int32_t *node_child, const int32_t *node_parent, const double *node_logw, const int32_t *leaf_meta,
                const int32_t *leaf_ints, const float *leaf_params, int levels, int max_leaf_d, void *work, float *out,
                int32_t *choice, void *stream);
int dpc_cnq_sample(const float *x, const uint8_t *codes, int64_t b, int d, int n_nodes, const int32_t *node_col,
                   const int32_t *node_child, const int32_t *node_parent, const double *node_logw, const int32_t *leaf_meta,
                   const int32_t *leaf_ints, const float *leaf_params, int levels, int max_leaf_d, uint64_t seed, int64_t row0,
                   void *work, float *out, int32_t *choice, void *stream);

/* ---- Posterior marginals: p(x_j = 1 | the row's observed entries) for every NaN entry, exact, one launch each ----
 *
 * x: [b, d] float32 row major, NaN = unknown; codes: the output of dpc_pack_query for the same rows.  out: [b, d]
 * float32: an observed entry comes back bit for bit (its 0.0 or 1.0 is its own marginal), a NaN entry becomes the
 * posterior probability that it is 1.  A row whose evidence has probability zero (tables that hold -inf) gets NaN in
 * its unobserved entries.  b = 0 writes nothing.
 *
 * The tree (dpc_mar_clt; float32 throughout).  A row with NaN runs the upward pass above with R = lse: t_j[l] for every
 * j but the root, the same expressions in the same order as dpc_clt_log_likelihood.  Then, in `bfs` order, every j gets
 * its normalised log belief b_j[k] = log p(x_j = k | e):
 *   ev_j[k]  = 0, or -inf where x_j is observed and is not k;
 *   the root:            a_k = (params[root][0][k] + m_root[k]) + ev_root[k];
 *   a child j of pa:     cav[l] = b_pa[l] - t_j[l], taken as -inf where b_pa[l] is -inf (the belief of pa without
 *                        what j sent it; the plain difference would be -inf - (-inf)),
 *                        a_k = (lse(cav[0] + params[j][0][k], cav[1] + params[j][1][k]) + m_j[k]) + ev_j[k];
 *   b_j[k]   = a_k - lse(a_0, a_1), and a NaN entry j becomes expf(b_j[1]).
 * m_j is pulled from the children's t as above; b_j takes the slot of t_j, which nothing reads after j (the children's
 * slots still hold their t when j pulls them), so work is the [2 * d * b] float32 scratch of dpc_clt_log_likelihood. */
int dpc_mar_clt(const float *x, const uint8_t *codes, int64_t b, int d, const int32_t *bfs, const int32_t *parent,
                const float *params, const int32_t *child_off, const int32_t *child_idx, float *work, float *out,
                void *stream);

/* The network (dpc_mar_cnet): the tables of dpc_cnet_log_likelihood, trusted; the result is a marginal only if every
 * path from the root to a leaf accounts for every column, as a cut or in the leaf's scope (the binding checks it).  A row
 * with NaN walks the OR tree depth first twice, each walk exactly the walk of dpc_cnet_log_likelihood for a row with NaN.
 *   First walk:   log P(e) = V(root), KEPT IN float64 (V(leaf) float32 as there: the gather path if none of the leaf's
 *                 columns is NaN, else the upward pass with R = lse).  log P(e) = -inf: NaN in every unobserved entry.
 *   Second walk:  node k is entered with the prefix weight p_k in float64, p_root = 0; the child for side c is entered
 *                 with p_k + node_logw[k][c].  Every node returns S = the sum of pi_l over the leaves below it that
 *                 are consistent with the row:
 *     a leaf l        pi_l = exp((p_l + V(l)) - log P(e)) in float64; S = pi_l.  If pi_l > 0 and the leaf holds NaN
 *                     columns, the downward pass of dpc_mar_clt follows the leaf's upward pass (float32, over the
 *                     leaf's columns) and every NaN position j of the leaf adds pi_l * (double)expf(b_j[1]) to the
 *                     accumulator of its column;
 *     x_col observed  S = S(child x);
 *     x_col NaN       child 0, then child 1; the accumulator of `col` gets += S(child 1); S = S(child 0) + S(child 1).
 *   The accumulators are float64, zero before the second walk, added to in the order of the walk; a NaN entry of the row
 *   becomes its accumulator rounded to float32.
 * levels, max_leaf_d: as for dpc_cnet_log_likelihood; a row whose stack would grow past `levels` gets NaN in its
 * unobserved entries, with no write past the stack.  work: b * (20 * levels + 8 * max_leaf_d + 8 * d) bytes of scratch,
 * 8-byte aligned: per row the stack of `levels` (float64, float64, int32) entries -- the left side's value or sum, the
 * prefix weight, the node -- the d float64 accumulators and the 2 * max_leaf_d floats of the leaf passes. */
int dpc_mar_cnet(const float *x, const uint8_t *codes, int64_t b, int d, int n_nodes, const int32_t *node_col,
                 const int32_t *node_child, const double *node_logw, const int32_t *leaf_meta, const int32_t *leaf_ints,
                 const float *leaf_params, int levels, int max_leaf_d, void *work, float *out, void *stream);

/* ---- Scored cutset learners (deeprob.spn.learning.cnet_bayesian; reference spn/learning/cnet_bayesian.py) ----
 *
 * learn_cnet_bd / learn_cnet_bic try several candidate cut columns per task and fit a Chow-Liu tree to each
 * side of every candidate.  All a fit needs is the co-occurrence counts of the task's rows CONDITIONED on
 * the candidate column.  An entry e names a task entry_task[e] of the generation (an index into word_off)
 * and a cut column entry_col[e]:
 *   ones1[e][i][j] = rows of the task with x_i = x_j = x_c = 1
 *                  = popcount(P_i & P_j & P_c) over the words word_off[task] .. word_off[task + 1)
 * of the planes of dpc_cnet_gather_pack, exact integers.  The side x_c = 0 is the caller's subtraction
 * dpc_cnet_pair_counts[task] - ones1[e]; the side sizes are ones[task][c][c] and n_task minus it.
 * ones1: [n_entries, d, d] int32, n_entries <= 65535; every element is written, each [d, d] block is
 * symmetric, and it is all zero for an entry whose task owns no word -- or whose task is outside
 * 0 .. n_tasks - 1 or whose column is outside 0 .. d - 1: such an entry reads nothing.  Row i = c and column
 * j = c hold ones[task][c][.], the diagonal holds popcount(P_i & P_c).  word_off: the generation's
 * [n_tasks + 1] offsets (trusted, as above).  Entries may name the tasks in any order, any number of times. */
int dpc_cut_pair_counts(const uint64_t *planes, int64_t n_words, int d, const int32_t *word_off, int n_tasks,
                        const int32_t *entry_task, const int32_t *entry_col, int n_entries, int32_t *ones1, void *stream);

/* ---- XPC learners (deeprob.spn.learning.xpc; reference spn/learning/xpc.py, spn/utils/partitioning.py) ----
 *
 * An XPC splits the rows of a partition by a CONJUNCTION of conj_len binary variables, 2^conj_len ways at most.  Both
 * entries read the bit planes of the WHOLE training matrix, planes [d, n_words] from dpc_pack_bits for the n rows
 * (n_words = (n + 63) / 64), through a row index: task t owns rows[seg_off[t] .. seg_off[t+1]) (indices into the
 * training matrix, the convention of the dpc_cnet_* section) and the conj_len columns conj_cols[t][0 .. conj_len).
 * The code of a row r is
 *     code(r) = sum over i < conj_len of bit(x[r][conj_cols[t][i]]) << i,
 * one word read per column and 64 consecutive rows.  A row index outside 0 .. n-1 and a column outside 0 .. d-1 read
 * as zeros.  A task's segment is cut into chunks of DPC_XPC_CHUNK rows, one work-group each:
 *     chunk_off[t+1] - chunk_off[t] = (n_t + DPC_XPC_CHUNK - 1) / DPC_XPC_CHUNK,  chunk_off[0] = 0,
 *     chunk_off[n_tasks] = n_chunks; a task of 0 rows owns no chunk.
 * seg_off, chunk_off: [n_tasks + 1] int32, trusted like `rows`.  conj_cols: [n_tasks, conj_len] int32.  Integer results
 * only; no global atomics; no work-group waits on another. */
#define DPC_XPC_MAX_CONJ 8 /* the longest conjunction: 256 codes, one per thread of a work-group */
#define DPC_XPC_CHUNK 1024 /* rows per work-group                                                  */

/* hist[t][code] = rows of task t with that code; chunk_hist[c][code] = the same for chunk c alone (dpc_xpc_partition
 * reads it), so that hist[t] is the sum of chunk_hist over the chunks chunk_off[t] .. chunk_off[t+1).
 * hist: [n_tasks, 2^conj_len] int32, all zero for a task of 0 rows; chunk_hist: [n_chunks, 2^conj_len] int32 (may be
 * null when n_chunks = 0). */
int dpc_xpc_code_counts(const uint64_t *planes, int64_t n_words, int64_t n, int d, const int32_t *rows,
                        const int32_t *seg_off, const int32_t *chunk_off, const int32_t *conj_cols, int conj_len,
                        int n_tasks, int n_chunks, int32_t *chunk_hist, int32_t *hist, void *stream);

/* Stable k-way split of every task.  child_of_code[t][code] in 0 .. 2^conj_len - 1 names the child a row with that code
 * goes to (anything else is taken as child 0); the rows of child k of task t are written to
 * rows_out[out_off[t][k] ..] IN THE ORDER THEY HAVE IN `rows`, so an ascending segment gives ascending children.  The
 * caller lays the children out so that they tile rows_out: out_off[t][k + 1] - out_off[t][k] = the sum of hist[t][code]
 * over the codes of child k; a child without rows writes nothing.  chunk_hist: the output of dpc_xpc_code_counts for the
 * SAME tasks and columns: a work-group starts each child at out_off plus the rows of that child in the task's chunks in
 * front of it, and ranks its own rows with wave ballots and popcounts.
 * child_of_code, out_off: [n_tasks, 2^conj_len] int32; rows_out: int32, sum of n_t entries. */
int dpc_xpc_partition(const uint64_t *planes, int64_t n_words, int64_t n, int d, const int32_t *rows, const int32_t *seg_off,
                      const int32_t *chunk_off, const int32_t *conj_cols, int conj_len, const int32_t *chunk_hist,
                      const int32_t *child_of_code, const int32_t *out_off, int n_tasks, int n_chunks, int32_t *rows_out,
                      void *stream);

/* ---- Mixtures of Chow-Liu trees (deeprob.spn.structure.cltmix.BinaryCLTMixture): likelihoods, responsibilities and
 * the sufficient statistics of tied-CPT batch EM (reference spn/structure/cltree.py:117-155, node.py:91-111), for all
 * n_comp components in one call.  ABI version 5.
 *
 * The n_comp trees are over the same d positions and are STACKED: bfs[n_comp][d], parent[n_comp][d],
 * params[n_comp][d][2][2], child_off[n_comp][d + 1], child_idx[n_comp][d - 1], each slice the tables of one tree as
 * above (trusted).  codes: [d, b] from dpc_pack_query.  rows: [nb] int32 or null: position i of the batch is row rows[i]
 * of `codes` (null: nb = b must hold and position i is row i).  A row index outside 0 .. b-1 reads nothing: the
 * likelihood outputs of that position are NaN, and it adds nothing to the statistics. */
#define DPC_MIX_MAX_K 64    /* the largest number of components                                                    */
#define DPC_MIX_CHUNK 1024  /* batch positions per work-group of dpc_mix_em_stats, and per chunk sum of its order  */

/* comp_ll[i][k] = the value dpc_clt_log_likelihood gives tree k on that row, bit for bit (the same device function:
 * the float64 gather for a complete row, the pulled upward pass for a row with NaN).  Then, in float32,
 *   a_k = logw[k] + comp_ll[i][k];  M = max over k;  L = logf(sum over k INCREASING FROM 0.0f of expf(a_k - M));
 *   ll[i] = M + L,  -inf when M = -inf;
 *   resp[i][k] = expf((a_k - M) - L), which is expf(a_k - ll[i]) without the rounding of M + L (half an ulp of |ll|
 *                would otherwise be a relative error of every responsibility);  0 when ll[i] = -inf (the row has no
 *                responsibility).
 * comp_ll, resp: [nb, n_comp] float32; ll: [nb] float32; logw: [n_comp] float32 (-inf allowed).
 * work: [n_comp * 2 * d * nb] float32 scratch: the state of the upward pass of component k at position i.  Only a row with
 * NaN touches it.  work may be NULL when the caller knows that every row is complete (EM checks it on the host): a row
 * with NaN then gets NaN in comp_ll, ll and resp, and nothing is read or written through work. */
int dpc_mix_log_likelihood(const uint8_t *codes, int64_t b, int d, const int32_t *rows, int64_t nb, int n_comp,
                           const int32_t *bfs, const int32_t *parent, const float *params, const int32_t *child_off,
                           const int32_t *child_idx, const float *logw, float *work, float *comp_ll, float *ll,
                           float *resp, void *stream);

/* stats[k][0] = sum over i of g_ik;  stats[k][1 + j] = sum of g_ik x_ij;  stats[k][1 + d + j] = sum of
 * g_ik x_ij x_i,parent[k][j] (0.0 at the root, and where parent[k][j] is outside 0 .. d-1), with g_ik = (double)resp[i][k]
 * and x = 1 where the code is 1, else 0 (DPC_MISSING counts as 0).  Every term is g_ik or 0.0, exact.  Order of every
 * float64 sum: the batch is cut into chunks of DPC_MIX_CHUNK positions; in a chunk, partial l (l < 256) takes the
 * positions l, l + 256, ... of the chunk in order, starting from 0.0; the chunk sum adds the 256 partials in order of
 * l, starting from partial 0; stats adds the chunk sums in increasing chunk order, starting from chunk 0.  The grid
 * has no part in it: a second call gives the same bits.
 * resp: [nb, n_comp] float32; parent: [n_comp, d] int32; stats: [n_comp, 1 + 2 d] float64;
 * part: [n_chunks, n_comp, 1 + 2 d] float64 scratch (the chunk sums), n_chunks = (nb + DPC_MIX_CHUNK - 1) / DPC_MIX_CHUNK.
 * nb = 0 gives stats = 0. */
int dpc_mix_em_stats(const uint8_t *codes, int64_t b, int d, const int32_t *rows, int64_t nb, int n_comp,
                     const float *resp, const int32_t *parent, double *part, double *stats, void *stream);

/* ---- Posterior queries of a mixture of Chow-Liu trees (BinaryCLTMixture.marginals / sample / mpe): posterior marginals,
 * conditional sampling and max-product MPE, one launch each.  ABI version 6.
 *
 * x: [b, d] float32 row major, NaN = unknown; codes: the output of dpc_pack_query for the same rows.  The model is the
 * stacked tables of dpc_mix_log_likelihood (trusted) and logw [n_comp] float32 (-inf allowed); n_comp <= DPC_MIX_MAX_K,
 * d <= DPC_MAX_D.  out: [b, d] float32: an observed entry comes back bit for bit.  b = 0 writes nothing.
 *
 * The mixture level, common to the three, is float64:
 *   a_k  = (double)logw[k] + (double)V_k;   M = max over k of a_k;
 *   S    = the sum over k INCREASING FROM 0.0 of exp(a_k - M);   T = M + log(S);   pi_k = exp(a_k - T).
 * V_k is the float32 value of tree k on the row.  For the marginals and for sampling it is the value
 * dpc_clt_log_likelihood gives: the float64 gather for a row without NaN, the upward pass with R = lse otherwise.  For
 * MPE it is the same with R = max.  pi_k is the posterior probability of component k given the row's observed entries.
 * The trees are visited one at a time, in increasing k, through ONE [2 * d] float32 message table per row; a tree that is
 * needed again is passed again, so that the scratch does not grow with n_comp * d.
 * work is scratch, 8-byte aligned: b * (16 * d + 8 * n_comp) bytes for the marginals (per row the 2 * d floats of the
 * messages, d float64 accumulators and the n_comp values a_k), b * (8 * d + 8 * n_comp) bytes for the two fills (the
 * messages and the a_k).
 *
 * dpc_mixq_marginals.  A row without NaN is a copy.  Otherwise the accumulators of the row start at 0.0 and, for k
 * increasing, every component with pi_k > 0 runs the two passes of dpc_mar_clt (the same expressions in the same order)
 * and adds pi_k * (double)expf(b_j[1]) to the accumulator of every NaN entry j; the entry becomes its accumulator rounded to
 * float32.  M = -inf (the evidence is impossible under every component, or every weight is zero): NaN in the NaN entries.
 * With n_comp = 1 and M finite, pi_0 = 1 exactly and the result is that of dpc_mar_clt bit for bit. */
int dpc_mixq_marginals(const float *x, const uint8_t *codes, int64_t b, int d, int n_comp, const int32_t *bfs,
                       const int32_t *parent, const float *params, const int32_t *child_off, const int32_t *child_idx,
                       const float *logw, void *work, float *out, void *stream);

/* dpc_mixq_sample: an exact draw of (component, the NaN entries) given the observed entries.  u(i) = the generator of
 * dpc_clt_sample with ctr = (row0 + r) * (1 + d) + i, so that a row's output depends only on (seed, row0 + r, the row);
 * `row0` lets a caller sample a long batch in pieces.  The component is the smallest k with (double)u(0) < c_k, c_k the
 * running sum pi_0 + ... + pi_k added in increasing k from 0.0; if rounding leaves none, the largest k with pi_k > 0.
 * Then tree k's upward pass (R = lse) is run again and its NaN columns are filled in `bfs` order by the rule of
 * dpc_cnq_sample: for position j with parent value xp (row 0 at the root), a_v = params[j][xp][v] + m_j[v] in float32 and
 * the entry is 1 iff u(1 + j) < expf(a_1 - lse(a_0, a_1)): the normalised conditional (NOT the expression of
 * dpc_clt_sample).  A row without NaN is a copy, and its component is still drawn: a posterior draw of the row's
 * cluster.  M = -inf: the NaN entries stay NaN and component[r] = -1.  component: [b] int32 or null. */
int dpc_mixq_sample(const float *x, const uint8_t *codes, int64_t b, int d, int n_comp, const int32_t *bfs,
                    const int32_t *parent, const float *params, const int32_t *child_off, const int32_t *child_idx,
                    const float *logw, uint64_t seed, int64_t row0, void *work, float *out, int32_t *component, void *stream);

/* dpc_mixq_mpe: the (component, completion) that maximises logw[k] + log p_k(x) over the completions of the row AND the
 * components -- the max-product MPE of the mixture's circuit.  (It is NOT the MAP of the mixture density, the completion
 * that maximises the SUM over k, which is NP-hard.)  The component is the smallest k that attains max over k of a_k (V_k
 * with R = max); tree k's upward pass (R = max) is run again and its NaN columns are filled in `bfs` order by the rule of
 * dpc_clt_mpe: 1 iff a_1 > a_0.  With n_comp = 1 and M finite the result is that of dpc_clt_mpe bit for bit.  M = -inf: the
 * NaN entries stay NaN and component[r] = -1.  component: [b] int32 or null. */
int dpc_mixq_mpe(const float *x, const uint8_t *codes, int64_t b, int d, int n_comp, const int32_t *bfs, const int32_t *parent,
                 const float *params, const int32_t *child_off, const int32_t *child_idx, const float *logw, void *work,
                 float *out, int32_t *component, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPROB_CLT_H */
