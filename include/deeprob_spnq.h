/*
 * deeprob_spnq.h -- C ABI of libdeeprob_spnq.so (gfx950 / MI355X): posterior queries on a node-graph SPN
 * (deeprob.spn.structure.io.FlatSpn) -- conditional moments of the unobserved entries
 * (deeprob.spn.algorithms.moments) and the posterior of one discrete variable
 * (deeprob.spn.algorithms.inference.posterior) -- in one launch.
 *
 * The identity.  In a smooth and decomposable circuit the root polynomial is linear in the leaves of any one
 * variable j.  With e the evidence of a row (its non-NaN entries), P_N the value of node N under e and
 *   r_L = (dP_root / dP_L) * P_L / P_root            the posterior flow into leaf L,
 * summed over the leaves L over j:
 *   E[x_j^k | e]   = sum_L r_L * m_k(L)              m_k(L) the order-k non-central moment of leaf L
 *   p(x_j = v | e) = sum_L r_L * p_L(v)
 * and sum_L r_L = 1.  For a variable that is NaN in the row every leaf over it has P_L = 1, so
 * r_L = exp(g_L) / P_root with g_L = log dP_root / dP_L.
 *
 * The passes, per row (a 64-lane wave takes 64 rows, lane = row; tables are [node id][row]):
 *   1. bottom-up: the node values of dpk_flat_spn_forward (include/deeprob_hip.h): float32, every value
 *      clamped at -1e31, children in child order.  Every node keeps its row.
 *   2. top-down log-gradients, the recurrences of dpk_flat_spn_backward: g_root = 0, every other node
 *      -inf; over the evaluation order reversed (parents before children) a sum node passes
 *      g + log w_k (child_logw) to child k, a product node (g + value_node) - value_child, children in
 *      child order; a child's row is the running log-add-exp m + log1p(exp(-|a - b|)), m = max(a, b), of
 *      what its parents pass (m = -inf stays -inf), so a child of several parents accumulates from each
 *      of them in the order the parents are visited.
 *   3. per variable j that has leaves (var_leaf_off / var_leaf below) and is NaN in the row: with
 *      L_0 < L_1 < .. the leaves over j in increasing node id,
 *        M   = max_i g_{L_i}                                    (float32)
 *        e_i = (double)expf(g_{L_i} - M)                        (float32 exponential, widened)
 *        Z   = ((e_0 + e_1) + e_2) + ..                         (float64, increasing node id)
 *        S   = ((e_0 t_0 + e_1 t_1) + e_2 t_2) + ..             (float64, t_i = m_k(L_i) or p_{L_i}(v))
 *        result = (float)(S / Z)
 *      The flows are normalised by their own sum Z, not by the root's value: they sum to 1 whatever the
 *      float32 passes rounded.  No product is contracted into a fused multiply-add.  In a smooth and
 *      decomposable circuit sum_i exp(g_{L_i}) is the root's value, so above the floor some g_{L_i} is
 *      finite; for a table that breaks this (every g_{L_i} = -inf, M = -inf) the result is NaN = 0 / 0.
 *
 * Leaf moments m_k, k = 1..4, in float64 from the leaves' own parameters (raw0 / raw1, cat_prob, cat_value):
 *   Bernoulli p                p
 *   Categorical                ((v_0^k p_0 + v_1^k p_1) + ..) in category order, v^k = v * v * ..
 *   Uniform (s, w), b = s + w  (b^(k+1) - s^(k+1)) / ((k + 1) w), the powers by repeated multiplication
 *   Gaussian (mu, sd)          mu;  mu^2 + sd^2;  mu^3 + 3 mu sd^2;  mu^4 + 6 mu^2 sd^2 + 3 sd^4
 * Leaf probabilities p_L(v): Bernoulli p at v == 1, 1 - p at v == 0; Categorical cat_prob of the category
 * equal to (int64)v (the rule of the forward pass); 0 outside the support and for a continuous leaf.
 *
 * Two routes, identical output bits.  On chip: the value table and the gradient table of a wave
 * (256 bytes per node each, 512 bytes per node together; there is no other per-wave bookkeeping) live
 * in LDS when they fit in DPQ_LDS_BUDGET_BYTES = 65536, i.e. for circuits of up to 128 nodes; then
 * dpq_flat_spn_posterior_workspace_bytes is 0.  Otherwise, or with DPQ_FLAG_FORCE_WORKSPACE, the same code
 * runs on a caller-supplied workspace of two [n_nodes, B] float32 tables.
 *
 * The circuit travels as the record deeprob_hip.h calls dpk_flat_spn_circuit; dpq_flat_spn_circuit below
 * is layout-identical (the library asserts it at compile time), so one record serves both libraries.
 *   var_leaf_off [n_vars + 1], var_leaf [n_leaves]  int32, DEVICE memory: the node ids of the leaves over
 *   variable j are var_leaf[var_leaf_off[j] .. var_leaf_off[j + 1]), increasing.  A variable without leaves
 *   is outside the circuit's scope.  n_leaves = var_leaf_off[n_vars] is the length of var_leaf; the tables
 *   live in device memory, so the entry point checks only n_leaves > 0 and trusts their contents as it
 *   trusts the circuit's other index arrays.
 *
 * Every pointer is a DEVICE pointer except the circuit record itself; `stream` is a hipStream_t passed as
 * void*; the kernel is enqueued asynchronously on it and the entry point neither synchronises nor allocates.
 *
 * Buffer contract (the one of include/deeprob_hip.h, repeated):
 *   1. an entry point writes only its output arguments and its workspace, over their documented extent;
 *   2. it writes every element of every output, for every legal shape (B = 0 writes nothing);
 *   3. nothing it does depends on what the outputs or the workspace held on entry;
 *   4. it leaves its `const` inputs alone.
 * No floating-point value is accumulated atomically and no kernel waits on another work-group: a row's
 * output depends on the row and the circuit only, and two calls give the same bits.
 *
 * The return value is 0 on success (a size for *_workspace_bytes) and a negative DPQ_E* code otherwise;
 * dpq_last_error() returns a thread-local message for the last failure.
 */
#ifndef DEEPROB_SPNQ_H
#define DEEPROB_SPNQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPQ_OK 0
#define DPQ_EINVAL (-1)     /* bad argument (null pointer, size or mode out of domain) */
#define DPQ_EWORKSPACE (-2) /* workspace too small                                     */
#define DPQ_ELAUNCH (-3)    /* hipLaunch / runtime error                               */

#define DPQ_MODE_MOMENTS 0          /* conditional non-central moments of every variable          */
#define DPQ_MODE_VALUES 1           /* posterior probabilities of given values of one variable    */
#define DPQ_MAX_ORDERS 4            /* moments of order 1 .. 4                                    */
#define DPQ_LDS_BUDGET_BYTES 65536  /* on-chip route: 512 bytes per node per wave within this     */
#define DPQ_FLAG_FORCE_WORKSPACE 1u /* take the workspace route whatever the circuit's size       */

typedef struct dpq_flat_spn_circuit {
    int32_t n_nodes, root, n_sum, n_vars, n_child, n_cat, n_slots, max_children;
    const int32_t *order, *kind, *arg0, *arg1, *arg2, *sum_index;
    const int32_t *child_index, *child_slot, *node_slot, *cat_value;
    float *child_weight, *child_logw, *cat_logp;
    double *par0, *par1, *raw0, *raw1, *cat_prob;
} dpq_flat_spn_circuit;

const char *dpq_last_error(void);
int dpq_abi_version(void);

/* Bytes of workspace dpq_flat_spn_posterior needs for B rows of this circuit under `flags`: 0 on the on-chip
 * route, else two [n_nodes, B] float32 tables (each rounded up to 256 bytes). */
int64_t dpq_flat_spn_posterior_workspace_bytes(int64_t B, const dpq_flat_spn_circuit *c, uint32_t flags);

/* x [B, D] float32, D >= n_vars, NaN = not observed.
 * mode DPQ_MODE_MOMENTS: out [n_orders, B, D] float32, 1 <= n_orders <= DPQ_MAX_ORDERS; plane k - 1 holds, per
 *   entry (b, j): x[b, j] NaN and j inside the scope -- E[x_j^k | the row's evidence]; observed and inside the
 *   scope -- x^k as the float32 products x, x * x, (x * x) * x, ((x * x) * x) * x (a point mass; order 1 is x bit
 *   for bit); outside the scope (j >= n_vars or no leaf over j) -- x[b, j] as given, in every plane.
 *   `var`, `values`, `n_values` are not read.
 * mode DPQ_MODE_VALUES: out [B, n_values] float32, 0 <= var < n_vars, n_values >= 1, values [n_values] float32;
 *   x[b, var] NaN -- out[b, v] = p(x_var = values[v] | the row's evidence); observed -- 1 where
 *   values[v] == x[b, var], else 0.  `n_orders` is not read.
 * Evidence of probability zero (the root's value on the -1e31 floor): NaN in every in-scope NaN entry of the row
 *   (moments), in the whole row (values). */
int dpq_flat_spn_posterior(const float *x, int64_t B, int32_t D, const dpq_flat_spn_circuit *c,
                           const int32_t *var_leaf_off, const int32_t *var_leaf, int32_t n_leaves, int32_t mode,
                           int32_t n_orders, int32_t var, const float *values, int32_t n_values, float *out,
                           uint32_t flags, void *ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPROB_SPNQ_H */
