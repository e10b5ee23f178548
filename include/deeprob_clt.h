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

#ifdef __cplusplus
}
#endif
#endif /* DEEPROB_CLT_H */
